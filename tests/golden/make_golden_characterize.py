"""Generate tests/golden/characterize/characterize_cases.npz: mass, signal and size computed by
the REFERENCE's ``find_link.characterize`` (find_link.py:44-79, run through oracle/refshim.py) --
what pins ``clustertracking_amd.find.characterize`` / ``locate``.

    python tests/golden/make_golden_characterize.py     (build container only: needs the reference)

What NumPy 2 and the absent trackpy need is supplied here, the reference's arithmetic is
untouched: trackpy's two weight tables (``r_squared_mask``, ``x_squared_masks``, restated in
tests/_characterize.py: PARITY UNPINNED for these two) are bound onto the loaded ``find_link``
module, and ``masks.slice_pad``'s list index (masks.py:23,25) is served by viewing the image, and
what ``np.pad`` returns, as ``refshim.ListIndexArray``.

Layout: ``names`` (JSON list); per case ``i``: ``image_i`` (one frame), ``coords_i`` (float64
[N, ndim]), ``args_i`` (JSON: radius, isotropic, scale_factor), ``mass_i``, ``signal_i`` ([N])
and ``size_i`` ([N], or [N, ndim] when not isotropic), as the reference returns them.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import refshim  # noqa: E402
import _characterize  # noqa: E402
from clustertracking_amd import artificial  # noqa: E402

DTYPES = ('uint8', 'uint16', 'int16', 'int32', 'float32', 'float64')


class _PadProxy(object):
    """``np`` for the reference's masks module: ``pad`` returns an array its list index works on."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def pad(*args, **kwargs):
        return np.pad(*args, **kwargs).view(refshim.ListIndexArray)


def reference_characterize():
    ref = refshim.load()
    import clustertracking.find_link  # noqa: F401  (the package attribute of that name is the function)
    mod = sys.modules['clustertracking.find_link']
    mod.r_squared_mask = _characterize.r_squared_mask
    mod.x_squared_masks = _characterize.x_squared_masks
    sys.modules['clustertracking.masks'].np = _PadProxy()

    def run(coords, image, radius, isotropic, scale_factor):
        with np.errstate(divide='ignore', invalid='ignore'):
            return mod.characterize(coords, np.asarray(image).view(refshim.ListIndexArray), radius, isotropic,
                                    scale_factor)
    return ref, run


def blobs(shape, n, size, seed, dtype, scale=1., offset=0., noise=5.):
    """Gaussian blobs plus noise, scaled into the pixel type."""
    rng = np.random.RandomState(seed)
    ndim = len(shape)
    im = np.zeros(shape, dtype=np.float64)
    grid = np.indices(shape).astype(np.float64)
    for _ in range(n):
        c = [rng.uniform(0, s) for s in shape]
        r2 = sum(((g - ci) / size) ** 2 for g, ci in zip(grid, c))
        im += rng.uniform(50, 100) * np.exp(-r2 * ndim / 2)
    im += rng.uniform(0, noise, shape)
    im = im * scale + offset
    if np.dtype(dtype).kind in 'ui':
        info = np.iinfo(dtype)
        im = np.clip(np.round(im), info.min, info.max)
    return im.astype(dtype)


def border_points(shape):
    """Every corner, the middle of every edge / face, and the centre of the frame."""
    axes = [(0, (n - 1) // 2, n - 1) for n in shape]
    return np.array(np.meshgrid(*axes, indexing='ij'), dtype=np.float64).reshape(len(shape), -1).T


def cases(ref):
    out = []
    for k, dt in enumerate(DTYPES):
        scale = {'uint8': 2., 'uint16': 300., 'int16': 200., 'int32': 1e6}.get(dt, 1.)
        off = -100. * scale if dt in ('int16', 'int32') else 0.
        rng = np.random.RandomState(100 + k)
        im = blobs((30, 36), 8, 2.5, k, dt, scale, off)
        pts = np.vstack([border_points(im.shape),                      # padding on one and two sides
                         rng.uniform(-3, 33, (12, 2)),                  # anywhere, outside too
                         np.round(rng.uniform(4, 26, (6, 2))) + 0.5,    # x.5: the half-even corner
                         np.round(rng.uniform(6, 24, (6, 2))),          # pixels exactly on the mask edge
                         np.round(rng.uniform(6, 24, (4, 2))) + [0.25, 0.]])
        out.append(('2d_iso_%s' % dt, im, pts, (5, 5), True, 1.))
        out.append(('2d_aniso_%s' % dt, im, pts, (3, 5), False, 1.))
        im = blobs((9, 14, 16), 5, 2., 10 + k, dt, scale, off)
        pts = np.vstack([border_points(im.shape),                      # ... and three sides
                         rng.uniform(-2, 12, (8, 3)),
                         np.round(rng.uniform(2, 8, (4, 3))) + 0.5,
                         np.round(rng.uniform(3, 7, (4, 3)))])
        out.append(('3d_aniso_%s' % dt, im, pts, (2, 4, 4), False, 1.))
        out.append(('3d_iso_%s' % dt, im, pts[:12], (3, 3, 3), True, 1.))
    im = blobs((40, 40), 6, 3., 20, 'uint16', 100.)
    pts = np.array([[20., 20.], [13., 26.], [0., 5.], [39., 39.], [20.5, 19.5], [12.3, 30.9]])
    out.append(('r13_edge_u16', im, pts, (13, 13), True, 1.))            # 5-12-13: pixels on the edge
    out.append(('r10_r5_u16', im, pts, (10, 5), False, 1.))              # 6-8-10 and 3-4-5
    for r in ((0, 0), (1, 1), (0, 2), (1, 3)):
        out.append(('r%d%d_u8' % r, blobs((12, 12), 3, 2., 21, 'uint8', 2.), np.array([[5., 6.], [0., 0.], [6.5, 3.5], [11., 4.2]]),
                    r, r[0] == r[1], 1.))
        out.append(('r%d%d_f32_aniso' % r, blobs((12, 12), 3, 2., 22, 'float32'), np.array([[5., 6.], [0., 0.], [6.5, 3.5]]),
                    r, False, 1.))
    out.append(('r011_i16_3d', blobs((5, 8, 8), 2, 2., 23, 'int16', 10.), np.array([[2., 4., 4.], [0., 0., 7.], [2.5, 3.5, 1.5]]),
                (0, 1, 1), False, 1.))
    for dt in ('uint8', 'float32', 'float64', 'int32'):                  # all-zero window: size NaN
        im = blobs((20, 20), 2, 2., 24, dt, 2.)
        im[4:15, 4:15] = 0
        out.append(('zero_window_%s' % dt, im, np.array([[9., 9.], [9.5, 9.], [3., 9.], [0., 0.]]), (4, 4), True, 1.))
        out.append(('zero_window_aniso_%s' % dt, im, np.array([[9., 9.], [9.5, 9.], [3., 9.]]), (4, 3), False, 1.))
    out.append(('zeros_u16', np.zeros((10, 10), np.uint16), np.array([[5., 5.], [0., 9.]]), (3, 3), True, 1.))
    # negative floats: the masked-out zeros are the maximum, size is the root of a negative number
    for dt in ('float32', 'float64'):
        im = -blobs((24, 24), 4, 2., 25, dt) - 1
        out.append(('negative_%s' % dt, im, np.array([[12., 12.], [0., 3.], [7.5, 8.25], [23., 23.]]), (4, 4), True, 1.))
        out.append(('negative_aniso_%s' % dt, im, np.array([[12., 12.], [0., 3.], [7.5, 8.25]]), (2, 4), False, 1.))
    im = blobs((24, 24), 4, 2., 26, 'int16', 50., -3000.)               # mixed signs, integer
    out.append(('mixed_sign_i16', im, np.array([[12., 12.], [1., 22.], [7.5, 8.25]]), (4, 4), True, 1.))
    for dt in ('float32', 'float64', 'int16'):   # positive mass, negative weighted sum: size NaN
        im = np.full((16, 16), -1, dtype=dt)
        im[8, 8] = im[3, 12] = 1000
        out.append(('negative_quotient_%s' % dt, im, np.array([[8., 8.], [8.5, 8.5], [3., 12.], [0., 0.]]), (3, 3), True, 1.))
        out.append(('negative_quotient_aniso_%s' % dt, im, np.array([[8., 8.], [3.25, 12.]]), (2, 3), False, 1.))
    # a frame smaller than the window
    out.append(('tiny_u8', blobs((5, 4), 1, 2., 27, 'uint8', 2.), np.array([[2., 2.], [0., 3.], [4.5, 1.5], [-2., 6.]]), (6, 6), True, 1.))
    out.append(('tiny_f64_3d', blobs((3, 4, 5), 1, 2., 28, 'float64'), np.array([[1., 2., 2.], [0., 0., 0.], [2.5, 3.5, 4.5]]),
                (3, 4, 4), False, 1.))
    im = blobs((30, 30), 5, 2.5, 29, 'uint8', 2.)
    pts = np.array([[10., 12.], [15.5, 20.25], [0., 29.], [28., 3.]])
    out.append(('scale_u8', im, pts, (5, 5), True, 2.5))
    out.append(('scale_aniso_f32', im.astype(np.float32) * 0.37, pts, (4, 6), False, 0.125))
    # cfg-2-like and cfg-3-like crops (workloads.cfg2 / cfg3 geometry and statistics) with the
    # positions the reference's grey_dilation gives
    im, _, _ = artificial.random_frame((96, 96), 12, 3., 100, 10, seed=73, margin=13)
    pts = ref.find.grey_dilation(im, 13, percentile=64, margin=6, precise=True)
    out.append(('cfg2_crop', im, np.asarray(pts, dtype=np.float64), (6, 6), True, 1.))
    im, _, _ = artificial.random_frame((24, 48, 48), 10, (2., 4., 4.), 100, 10, seed=74, margin=(9, 17, 17))
    pts = ref.find.grey_dilation(im, (9, 17, 17), percentile=64, margin=(4, 8, 8), precise=True)
    out.append(('cfg3_crop', im, np.asarray(pts, dtype=np.float64), (4, 8, 8), False, 1.))
    return out


def main():
    ref, characterize = reference_characterize()
    arrays, names = {}, []
    for i, (name, image, coords, radius, isotropic, scale) in enumerate(cases(ref)):
        res = characterize(coords, image, radius, isotropic, scale)
        keys = _characterize.size_keys(image.ndim, isotropic)
        size = res['size'] if isotropic else np.stack([res[k] for k in keys], 1)
        names.append(name)
        arrays['image_%d' % i] = image
        arrays['coords_%d' % i] = np.asarray(coords, dtype=np.float64)
        arrays['args_%d' % i] = np.array(json.dumps(dict(radius=list(radius), isotropic=isotropic, scale_factor=scale)))
        arrays['mass_%d' % i] = res['mass']
        arrays['signal_%d' % i] = res['signal']
        arrays['size_%d' % i] = size
        print('%-26s %-8s %3d features, %3d NaN sizes' % (name, image.dtype, len(coords), np.isnan(size).sum()))
    arrays['names'] = np.array(json.dumps(names))
    np.savez_compressed(os.path.join(HERE, 'characterize', 'characterize_cases.npz'), **arrays)


if __name__ == '__main__':
    main()
