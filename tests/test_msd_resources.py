"""The kernels of the MSD stage (msd_kernels.h) use no scratch memory and leave room for several
workgroups on a CU: read from the metadata of the gfx950 code object in the built libctrefine.so
(CPU only), as tests/test_kernel_resources.py reads the block kernels'."""
import re

import pytest

import _resources

KERNELS = ['msd_check_kernel', 'msd_rows_kernel', 'msd_particle_kernel', 'msd_chunk_kernel', 'msd_pool_kernel']
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    return _resources.metadata('msd_', tmp_path_factory.mktemp('msd_co'))


@pytest.mark.parametrize('name', KERNELS)
def test_kernel_has_no_scratch(kernels, name):
    found = [k for k in kernels if re.search(r'\d+%s' % name, k)]
    assert len(found) == 1, (name, sorted(kernels))
    k = kernels[found[0]]
    print(name, 'VGPRs', k['.vgpr_count'], 'AGPRs', k['.agpr_count'], 'SGPRs', k['.sgpr_count'],
          'LDS bytes', k['.group_segment_fixed_size'], 'scratch', k['.private_segment_fixed_size'])
    assert int(k['.private_segment_fixed_size']) == 0, '%s uses %s B of scratch per lane' % (name, k['.private_segment_fixed_size'])
    assert int(k['.max_flat_workgroup_size']) == 256
    # several workgroups of 4 wavefronts on a CU: by LDS and by registers (512 per lane and SIMD)
    assert 2 * int(k['.group_segment_fixed_size']) <= LDS_PER_CU
    assert 2 * (int(k['.vgpr_count']) + int(k['.agpr_count'])) <= 512


def test_every_kernel_of_the_unit_is_listed(kernels):
    assert len(kernels) == len(KERNELS), sorted(kernels)
