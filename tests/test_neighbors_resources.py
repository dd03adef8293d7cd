"""The kernels of the neighbours stage (neighbors_kernels.h) use no scratch memory -- the list of the
best (d2, j) of a thread stays in registers at every capacity -- and leave room for two workgroups on a
CU: read from the metadata of the gfx950 code object in the built libctrefine.so (CPU only), as
tests/test_pcf_resources.py reads the pair correlation kernels'.  Only those metadata fields are read."""
import os
import re
import shutil
import subprocess

import pytest

LLVM_BIN = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
PREFIX = 'nbr_'
# the name as the source has it and what follows it in the mangled name: a plain kernel takes its
# argument next, an instantiation its capacity
KERNELS = {'nbr_check_kernel': r'E', 'nbr_defaults_kernel': r'E', 'nbr_items_kernel': r'E', 'nbr_particles_kernel': r'E',
           'nbr_pairs_kernel<1>': r'ILi1E', 'nbr_pairs_kernel<4>': r'ILi4E', 'nbr_pairs_kernel<16>': r'ILi16E'}
LDS_PER_CU = 160 * 1024


def _tool(name):
    p = os.path.join(LLVM_BIN, name)
    return p if os.path.exists(p) else shutil.which(name)


def _metadata(tmp):
    """{kernel name: its metadata fields} of every kernel whose name holds 'nbr_'"""
    from clustertracking_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), 'libctrefine.so is not built'
    objcopy, bundler, readelf = _tool('llvm-objcopy'), _tool('clang-offload-bundler'), _tool('llvm-readelf')
    assert objcopy and bundler and readelf, 'llvm-objcopy / clang-offload-bundler / llvm-readelf not found'
    fatbin = str(tmp / 'fatbin')
    subprocess.check_call([objcopy, '--dump-section', '.hip_fatbin=' + fatbin, _lib.LIB_PATH, str(tmp / 'lib.so')])
    data = open(fatbin, 'rb').read()
    starts = [m.start() for m in re.finditer(re.escape(b'__CLANG_OFFLOAD_BUNDLE__'), data)]
    assert starts, 'the fat binary holds no uncompressed offload bundles'
    out = {}
    for j, (s, e) in enumerate(zip(starts, starts[1:] + [len(data)])):
        if PREFIX.encode() not in data[s:e]:
            continue
        bundle, co = str(tmp / ('bundle%d' % j)), str(tmp / ('gfx950_%d.co' % j))
        with open(bundle, 'wb') as f:
            f.write(data[s:e])
        subprocess.check_call([bundler, '--type=o', '--unbundle', '--targets=' + TARGET, '--input=' + bundle, '--output=' + co])
        notes = subprocess.check_output([readelf, '--notes', co], text=True)
        for block in re.split(r'\n\s+- \.agpr_count:', notes)[1:]:
            fields = dict(re.findall(r'^\s*(\.[a-z_]+):\s+(\S+)\s*$', '.agpr_count:' + block, re.M))
            if PREFIX in fields.get('.name', ''):
                out[fields['.name']] = fields
    return out


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    return _metadata(tmp_path_factory.mktemp('nbr_co'))


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
