"""Register and scratch budget of the tuned block-kernel instantiations, read from the code object
of the built libctrefine.so (CPU only).

The 3-4-feature cells of the throughput table (refine_block_kernel<2, ISO, NT=1, W=2>, gaussian,
unconstrained, no lowpass) run at 3 wavefronts per SIMD (block_kernel.h: block_occ), the NT = 2
cells of that table at one.  They must do so without scratch memory: a later edit that brings
spills back, or that needs more registers than their wavefronts per SIMD leave, fails here instead
of silently costing throughput."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'

# refine_block_kernel<ND, ISO, NT, W, CONS, LP, FIT> -> mangled name (anonymous namespace)
def _mangled(nd, iso, nt, w, cons=False, lp=False, fit=0):
    b = lambda x: 'Lb1E' if x else 'Lb0E'
    return ('_ZN12_GLOBAL__N_119refine_block_kernelILi%dE%sLi%dELi%dE%s%sLi%dEEEv5KArgs'
            % (nd, b(iso), nt, w, b(cons), b(lp), fit))


# (kernel, waves per SIMD asked of the compiler)
TUNED = [
    (_mangled(2, True, 1, 2), 3),    # gauss_tp NT = 1, 2D isotropic
    (_mangled(2, False, 1, 2), 3),   # gauss_tp NT = 1, 2D anisotropic
    (_mangled(2, True, 2, 2), 1),    # gauss_tp NT = 2
    (_mangled(2, False, 2, 2), 1),
]
VGPRS_PER_SIMD = 512                 # per lane, CDNA3/4: VGPRs and AGPRs from one file
GRANULE = 8


def _tool(name):
    p = os.path.join(LLVM_BIN, name)
    return p if os.path.exists(p) else shutil.which(name)


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    from clustertracking_amd import _lib
    lib = _lib.LIB_PATH
    if not os.path.exists(lib):
        pytest.skip('libctrefine.so is not built')
    objcopy, bundler, readelf = _tool('llvm-objcopy'), _tool('clang-offload-bundler'), _tool('llvm-readelf')
    if not (objcopy and bundler and readelf):
        pytest.skip('llvm-objcopy / clang-offload-bundler / llvm-readelf not found')
    d = tmp_path_factory.mktemp('co')
    fatbin = str(d / 'fatbin')
    subprocess.check_call([objcopy, '--dump-section', '.hip_fatbin=' + fatbin, lib, str(d / 'lib.so')])
    # one offload bundle per translation unit, back to back in the section
    data = open(fatbin, 'rb').read()
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    starts = [m.start() for m in re.finditer(re.escape(magic), data)]
    if not starts:
        pytest.skip('the fat binary holds no uncompressed offload bundles')
    out = {}
    for j, (s, e) in enumerate(zip(starts, starts[1:] + [len(data)])):
        bundle, co = str(d / ('bundle%d' % j)), str(d / ('gfx950_%d.co' % j))
        with open(bundle, 'wb') as f:
            f.write(data[s:e])
        subprocess.check_call([bundler, '--type=o', '--unbundle', '--targets=' + TARGET,
                               '--input=' + bundle, '--output=' + co])
        notes = subprocess.check_output([readelf, '--notes', co], text=True)
        # the amdhsa.kernels list of the metadata note: one "- .agpr_count: ..." block per kernel
        for block in re.split(r'\n\s+- \.agpr_count:', notes)[1:]:
            block = '.agpr_count:' + block
            fields = dict(re.findall(r'^\s*(\.[a-z_]+):\s+(\S+)\s*$', block, re.M))
            if '.name' in fields:
                out[fields['.name']] = fields
    assert out, 'no kernel metadata found in the gfx950 code object'
    return out


@pytest.mark.parametrize('name,waves', TUNED, ids=['nt1-iso', 'nt1-aniso', 'nt2-iso', 'nt2-aniso'])
def test_tuned_block_kernel_has_no_scratch(kernels, name, waves):
    k = kernels.get(name)
    assert k is not None, '%s is not in the code object' % name
    assert int(k['.private_segment_fixed_size']) == 0, \
        '%s uses %s B of scratch per lane' % (name, k['.private_segment_fixed_size'])
    # budget of `waves` wavefronts per SIMD, in allocation granules
    budget = (VGPRS_PER_SIMD // waves) // GRANULE * GRANULE
    regs = int(k['.vgpr_count'])
    assert regs <= budget, '%s: %d VGPRs, %d wavefronts per SIMD allow %d' % (name, regs, waves, budget)
