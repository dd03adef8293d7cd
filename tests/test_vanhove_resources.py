"""The kernels of the van Hove stage (vanhove_kernels.h, compiled in the MSD unit) use no scratch
memory and leave room for two workgroups on a CU: read from the metadata of the gfx950 code object in
the built libctrefine.so (CPU only), as tests/test_msd_resources.py reads the MSD kernels'."""
import re

import pytest

import _resources

KERNELS = ['vanhove_clear_kernel', 'vanhove_bin_kernel', 'vanhove_finish_kernel']
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    return _resources.metadata('vanhove_', tmp_path_factory.mktemp('vanhove_co'))


@pytest.mark.parametrize('name', KERNELS)
def test_kernel_has_no_scratch(kernels, name):
    found = [k for k in kernels if re.search(r'\d+%s' % name, k)]
    assert len(found) == 1, (name, sorted(kernels))
    k = kernels[found[0]]
    print(name, 'VGPRs', k['.vgpr_count'], 'AGPRs', k['.agpr_count'], 'SGPRs', k['.sgpr_count'],
          'LDS bytes', k['.group_segment_fixed_size'], 'scratch', k['.private_segment_fixed_size'])
    assert int(k['.private_segment_fixed_size']) == 0, '%s uses %s B of scratch per lane' % (name, k['.private_segment_fixed_size'])
    assert int(k['.max_flat_workgroup_size']) == 256
    # two workgroups of 4 wavefronts on a CU: by LDS and by registers (512 per lane and SIMD)
    assert 2 * int(k['.group_segment_fixed_size']) <= LDS_PER_CU
    assert 2 * (int(k['.vgpr_count']) + int(k['.agpr_count'])) <= 512


def test_every_kernel_of_the_stage_is_listed(kernels):
    assert len(kernels) == len(KERNELS), sorted(kernels)
    assert not [k for k in kernels if 'msd_' in k]            # the MSD unit's own count of 'msd_' kernels stays five
