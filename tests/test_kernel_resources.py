"""Register and scratch budget of the tuned block-kernel instantiations, read from the code object
of the built libctrefine.so (CPU only).

The 3-4-feature cells of the throughput table (refine_block_kernel<2, ISO, NT=1, W=2>, gaussian,
unconstrained, no lowpass) run at 3 wavefronts per SIMD (block_kernel.h: block_occ), the NT = 2
cells of that table at one.  They must do so without scratch memory: a later edit that brings
spills back, or that needs more registers than their wavefronts per SIMD leave, fails here instead
of silently costing throughput."""
import pytest

import _resources

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


@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    try:
        out = _resources.metadata('', tmp_path_factory.mktemp('co'))
    except _resources.Unavailable as e:
        pytest.skip(str(e))
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
