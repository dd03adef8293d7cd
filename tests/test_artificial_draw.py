"""``clustertracking_amd.artificial.draw_feature`` / ``draw_gaussian`` -- the generator of every
synthetic frame of the tests, fixtures and benchmarks -- against the REFERENCE's
``artificial.draw_feature`` (artificial.py:81-141): tests/golden/draw_cases.npz holds images the
reference drew (tests/golden/make_golden_draw.py); gaussian, ring and disc features, 2D / 3D,
isotropic / anisotropic, uint8 / uint16 / float64, overlaps with integer wrap-around, patches
clipped at edges and corners.  Bit for bit for the integer pixel types."""
import json
import os

import numpy as np
from numpy.testing import assert_equal

import _cases
from clustertracking_amd import artificial


def test_drawn_features_equal_the_references_bit_for_bit():
    z = np.load(os.path.join(_cases.GOLDEN, 'draw_cases.npz'))
    cases = json.loads(str(z['cases']))
    assert len(cases) >= 9
    for name, shape, dtype, feats in cases:
        im = np.zeros(tuple(shape), dtype=dtype)
        for pos, size, max_value, feat_func, kw in feats:
            size = tuple(size) if isinstance(size, list) else size
            artificial.draw_feature(im, tuple(pos), size, max_value, feat_func, **kw)
            if feat_func == 'gauss':       # the two entry points are one function for the gaussian
                im2 = np.zeros(tuple(shape), dtype=dtype)
                artificial.draw_gaussian(im2, tuple(pos), size, max_value)
        if np.dtype(dtype).kind == 'f':
            # (the restatement takes exp(r2 ...) where the reference takes exp(sqrt(r2)**2 ...): the last bit;
            #  every synthetic frame of the tests and benchmarks is an integer image, where truncation decides)
            np.testing.assert_allclose(im, z[name], rtol=1e-14, atol=1e-300, err_msg=name)
        else:
            assert_equal(im, z[name], err_msg=name)


def test_against_the_reference_itself_when_it_is_here():
    """Seeded random gaussian, ring and disc features, 2D / 3D, against the images the reference drew
    for exactly these inputs (tests/golden/draw_random.npz, make_golden_draw.py:random_cases)."""
    z = np.load(os.path.join(_cases.GOLDEN, 'draw_random.npz'))
    rng = np.random.RandomState(5)
    n = 0
    for feat_func, kw in (('gauss', {}), ('ring', dict(thickness=0.25)), ('disc', dict(disc_size=0.4))):
        for ndim in (2, 3):
            shape = (36, 40) if ndim == 2 else (18, 26, 24)
            for i in range(4):
                pos = tuple(rng.uniform(0, np.array(shape) - 1e-9))
                size = tuple(rng.uniform(2., 4.5, ndim))
                name = '%s%dd_%d' % (feat_func, ndim, i)
                assert_equal(np.array(pos), z[name + '_pos'], err_msg=name)     # the inputs it was drawn for
                assert_equal(np.array(size), z[name + '_size'], err_msg=name)
                got = artificial.draw_feature(np.zeros(shape, np.uint8), pos, size, 150, feat_func, **kw)
                assert_equal(got, z[name], err_msg=name)
                n += 1
    assert n == len([k for k in z.files if not k.endswith(('_pos', '_size'))]) == 24
