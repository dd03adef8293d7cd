"""The kernels of the contacts stage (contacts_kernels.h) use no scratch memory -- a thread's row, a lane's
part of a chain and the scans stay in registers and LDS -- and leave room for two workgroups on a CU:
read from the metadata of the gfx950 code object in the built libctrefine.so (CPU only), as
tests/test_twopoint_resources.py reads the two-point kernels'.  Only those metadata fields are read."""
import re

import pytest

import _resources

PREFIX = 'cont_'
# the name as the source has it and what follows it in the mangled name: a plain kernel takes its argument next
KERNELS = {name: r'E' for name in (
    'cont_check_kernel', 'cont_count_defaults_kernel', 'cont_items_kernel', 'cont_count_kernel', 'cont_fill_defaults_kernel',
    'cont_fill_kernel', 'cont_episode_defaults_kernel', 'cont_scan_sums_kernel', 'cont_scan_top_kernel', 'cont_scan_apply_kernel',
    'cont_chains_kernel', 'cont_episodes_kernel', 'cont_pairs_kernel', 'cont_active_kernel')}
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    return _resources.metadata(PREFIX, tmp_path_factory.mktemp('cont_co'))


def _find(kernels, name):
    return [k for k in kernels if re.search(r'\d+%s%s' % (name, KERNELS[name]), k)]


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
