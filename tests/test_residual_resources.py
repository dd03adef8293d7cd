"""The kernels of the residual stage (residual_kernels.h) use no scratch memory -- a pixel's sums, the
staged row it is working on and a feature's partial sums stay in registers -- and leave room for two
workgroups on a CU: read from the metadata of the gfx950 code object in the built libctrefine.so (CPU
only), as tests/test_twopoint_resources.py reads the two-point kernels'.  Only those metadata fields are
read."""
import re

import pytest

import _resources

PREFIX = 'resid_'
# the name as the source has it, what follows it in the mangled name (a plain kernel takes its argument
# next, a template its arguments) and the number of instantiations: the frame pass is FIT x ND x ISO
KERNELS = {'resid_check_kernel': (r'E', 1), 'resid_frame_kernel': (r'ILi[0-3]ELi[23]ELb[01]EE', 16),
           'resid_feature_kernel': (r'ILi[23]EE', 2), 'resid_cluster_kernel': (r'E', 1)}
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    return _resources.metadata(PREFIX, tmp_path_factory.mktemp('resid_co'))


def _find(kernels, name):
    return [k for k in kernels if re.search(r'\d+%s%s' % (name, KERNELS[name][0]), k)]


@pytest.mark.parametrize('name', sorted(KERNELS))
def test_kernel_has_no_scratch_and_two_workgroups_fit(kernels, name):
    found = _find(kernels, name)
    assert len(found) == KERNELS[name][1], (name, sorted(kernels))
    for f in sorted(found):
        k = kernels[f]
        print(f, 'VGPRs', k['.vgpr_count'], 'AGPRs', k['.agpr_count'], 'SGPRs', k['.sgpr_count'],
              'LDS bytes', k['.group_segment_fixed_size'], 'scratch', k['.private_segment_fixed_size'])
        assert int(k['.private_segment_fixed_size']) == 0, '%s uses %s B of scratch per lane' % (f, k['.private_segment_fixed_size'])
        assert int(k['.max_flat_workgroup_size']) == 256
        # two workgroups of 4 wavefronts on a CU: by LDS and by registers (512 per lane and SIMD)
        assert int(k['.group_segment_fixed_size']) <= 64 * 1024
        assert 2 * int(k['.group_segment_fixed_size']) <= LDS_PER_CU
        assert 2 * (int(k['.vgpr_count']) + int(k['.agpr_count'])) <= 512


def test_every_kernel_of_the_unit_is_listed(kernels):
    listed = sorted(k for name in KERNELS for k in _find(kernels, name))
    assert listed == sorted(kernels) and len(listed) == sum(n for _, n in KERNELS.values()), sorted(kernels)


def test_frame_pass_lds_is_what_the_plan_reports(kernels):
    import importlib
    import numpy as np
    from clustertracking_amd import _lib
    residual = importlib.import_module('clustertracking_amd.residual')
    plan = _lib.residual_plan(residual.descriptor((16, 16), np.uint8, 1, 1, 7))
    assert {int(kernels[k]['.group_segment_fixed_size']) for k in _find(kernels, 'resid_frame_kernel')} == {plan.lds_bytes}
