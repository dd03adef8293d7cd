"""The kernels of the van Hove stage (vanhove_kernels.h, compiled in the MSD unit) use no scratch
memory and leave room for two workgroups on a CU: read from the metadata of the gfx950 code object in
the built libctrefine.so (CPU only), as tests/test_msd_resources.py reads the MSD kernels'."""
import os
import re
import shutil
import subprocess

import pytest

LLVM_BIN = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
KERNELS = ['vanhove_clear_kernel', 'vanhove_bin_kernel', 'vanhove_finish_kernel']
LDS_PER_CU = 160 * 1024


def _tool(name):
    p = os.path.join(LLVM_BIN, name)
    return p if os.path.exists(p) else shutil.which(name)


def _metadata(tmp):
    """{kernel name: its metadata fields} of every kernel whose name holds 'vanhove_'"""
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
        if b'vanhove_' not in data[s:e]:
            continue
        bundle, co = str(tmp / ('bundle%d' % j)), str(tmp / ('gfx950_%d.co' % j))
        with open(bundle, 'wb') as f:
            f.write(data[s:e])
        subprocess.check_call([bundler, '--type=o', '--unbundle', '--targets=' + TARGET, '--input=' + bundle, '--output=' + co])
        notes = subprocess.check_output([readelf, '--notes', co], text=True)
        for block in re.split(r'\n\s+- \.agpr_count:', notes)[1:]:
            fields = dict(re.findall(r'^\s*(\.[a-z_]+):\s+(\S+)\s*$', '.agpr_count:' + block, re.M))
            if 'vanhove_' in fields.get('.name', ''):
                out[fields['.name']] = fields
    return out


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    return _metadata(tmp_path_factory.mktemp('vanhove_co'))


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
