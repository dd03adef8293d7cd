"""The tail kernel in the code object of the built libctrefine.so (CPU only): both instantiations
of refine_tail_kernel<2, ISO> are there, with a workgroup of 128 threads and LDS that fits a CU.

No register or scratch bound is asserted: a call launches a few hundred of its workgroups, so
its occupancy does not matter (tail_kernel.h).  The figures are printed (pytest -s) for
profiles/README.md."""
import pytest

import _resources

LDS_CU = 160 * 1024


def _mangled(iso):
    return '_ZN12_GLOBAL__N_118refine_tail_kernelILi2ELb%dEEEv5KArgs8TailArgsPi' % (1 if iso else 0)


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    try:
        out = _resources.metadata('refine_tail_kernel', tmp_path_factory.mktemp('co'))
    except _resources.Unavailable as e:
        pytest.skip(str(e))
    return out


@pytest.mark.parametrize('iso', [True, False], ids=['iso', 'aniso'])
def test_tail_kernel_is_in_the_code_object(kernels, iso):
    name = _mangled(iso)
    k = kernels.get(name)
    assert k is not None, '%s is not in the code object; it holds %s' % (name, sorted(kernels))
    print('%s: %s VGPRs, %s AGPRs, %s SGPRs, %s B scratch per lane, %s B static LDS' % (
        name, k['.vgpr_count'], k['.agpr_count'], k['.sgpr_count'], k['.private_segment_fixed_size'],
        k['.group_segment_fixed_size']))
    assert int(k['.max_flat_workgroup_size']) == 128
    # (the dynamic LDS, the largest of its bodies' needs, is set at the launch; what the code
    # object records is the static part: none)
    assert int(k['.group_segment_fixed_size']) <= LDS_CU


def test_only_the_2d_instantiations(kernels):
    assert sorted(kernels) == sorted(_mangled(iso) for iso in (True, False))
