"""The kernels of the neighbours stage (neighbors_kernels.h) use no scratch memory -- the list of the
best (d2, j) of a thread stays in registers at every capacity -- and leave room for two workgroups on a
CU: read from the metadata of the gfx950 code object in the built libctrefine.so (CPU only), as
tests/test_pcf_resources.py reads the pair correlation kernels'.  Only those metadata fields are read."""
import re

import pytest

import _resources

PREFIX = 'nbr_'
# the name as the source has it and what follows it in the mangled name: a plain kernel takes its
# argument next, an instantiation its capacity
KERNELS = {'nbr_check_kernel': r'E', 'nbr_defaults_kernel': r'E', 'nbr_items_kernel': r'E', 'nbr_particles_kernel': r'E',
           'nbr_pairs_kernel<1>': r'ILi1E', 'nbr_pairs_kernel<4>': r'ILi4E', 'nbr_pairs_kernel<16>': r'ILi16E'}
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    return _resources.metadata(PREFIX, tmp_path_factory.mktemp('nbr_co'))


def _find(kernels, name):
    base = name.split('<')[0]
    return [k for k in kernels if re.search(r'\d+%s%s' % (base, KERNELS[name]), k)]


@pytest.mark.parametrize('name', sorted(KERNELS))
def test_kernel_has_no_scratch_and_two_workgroups_fit(kernels, name):
    found = _find(kernels, name)
    assert len(found) == 1, (name, sorted(kernels))
    k = kernels[found[0]]
    print(name, 'VGPRs', k['.vgpr_count'], 'AGPRs', k['.agpr_count'], 'SGPRs', k['.sgpr_count'],
          'LDS bytes', k['.group_segment_fixed_size'], 'scratch', k['.private_segment_fixed_size'])
    assert int(k['.private_segment_fixed_size']) == 0, '%s uses %s B of scratch per lane' % (name, k['.private_segment_fixed_size'])
    assert int(k['.max_flat_workgroup_size']) == 256
    # two workgroups of 4 wavefronts on a CU: by LDS and by registers (512 per lane and SIMD)
    assert int(k['.group_segment_fixed_size']) <= 64 * 1024
    assert 2 * int(k['.group_segment_fixed_size']) <= LDS_PER_CU
    assert 2 * (int(k['.vgpr_count']) + int(k['.agpr_count'])) <= 512


def test_every_kernel_of_the_unit_is_listed(kernels):
    listed = sorted(k for name in KERNELS for k in _find(kernels, name))
    assert listed == sorted(kernels) and len(listed) == len(KERNELS), sorted(kernels)
