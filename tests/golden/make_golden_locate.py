"""Generate tests/golden/locate/locate_cases.npz: local maxima found by the REFERENCE's
``find.grey_dilation`` (find.py:219-277, run through oracle/refshim.py) -- what pins
``clustertracking_amd.find.grey_dilation`` / ``locate_maxima``.

    python tests/golden/make_golden_locate.py        (build container only: needs the reference)

The file lies in a directory of its own: tests/_cases.py takes every .npz of tests/golden as a
refinement case.  Layout of the file: ``names`` (JSON list); per case ``i``: ``frame_i`` (the frame, its own
dtype and shape), ``args_i`` (JSON: separation, percentile, margin or null, precise),
``pos_i`` (the reference's output as it is: int64 [n, ndim], or float64 [0, ndim] when empty)
and ``thr_i`` (``percentile_threshold`` as float64, NaN when there is none).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import refshim  # noqa: E402
from clustertracking_amd import artificial  # noqa: E402

DTYPES = ('uint8', 'uint16', 'int16', 'int32', 'float32', 'float64')


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


def cases():
    out = []
    for k, dt in enumerate(DTYPES):
        scale = {'uint8': 2., 'uint16': 300., 'int16': 200., 'int32': 1e6}.get(dt, 1.)
        off = -100. * scale if dt in ('int16', 'int32') else 0.
        out.append(('2d_odd_%s' % dt, blobs((40, 48), 8, 2.5, k, dt, scale, off), 5, 64, None, True))
        out.append(('2d_even_%s' % dt, blobs((40, 48), 8, 2.5, 10 + k, dt, scale, off), 6, 64, None, True))
        out.append(('2d_aniso_%s' % dt, blobs((36, 52), 10, 2., 20 + k, dt, scale, off), (4, 7), 50, (2, 0), True))
        out.append(('2d_loose_%s' % dt, blobs((32, 40), 10, 2., 30 + k, dt, scale, off), 6, 64, None, False))
        out.append(('3d_%s' % dt, blobs((12, 20, 24), 6, 2., 40 + k, dt, scale, off), (3, 5, 5), 64, None, True))
        out.append(('3d_even_%s' % dt, blobs((10, 18, 20), 6, 2., 50 + k, dt, scale, off), (4, 6, 7), 64, (1, 2, 3), True))
    # a saturated plateau above the threshold: every plateau pixel is a maximum, ties decided by
    # sum(pos / separation) and by list order
    im = blobs((40, 40), 6, 2., 60, 'uint8', 1.)
    im[10:18, 12:20] = 255
    out.append(('plateau_u8', im, 6, 64, None, True))
    out.append(('plateau_u8_loose', im, 6, 64, None, False))
    im = np.zeros((30, 30), np.uint16)
    im[10, 14] = im[14, 10] = 900      # equal values, equal sum(pos / separation), close
    im[20, 20] = im[20, 24] = 700      # equal values, different sums
    im += blobs((30, 30), 0, 1., 61, 'uint16', 1., 0., 20.)
    out.append(('ties_u16', im, 6, 30, 0, True))
    # negative float frames: the zero border takes part in the maximum
    out.append(('negative_f32', blobs((30, 34), 6, 2., 62, 'float32', 1., -200.), 5, 64, None, True))
    out.append(('negative_f64', blobs((30, 34), 6, 2., 63, 'float64', -1., 0.), 5, 40, 0, True))
    out.append(('zeros_u8', np.zeros((20, 20), np.uint8), 5, 64, None, True))
    im = blobs((24, 24), 4, 2., 64, 'float32')
    im[3, 4] = np.nan
    out.append(('nan_f32', im, 5, 64, None, True))
    im = blobs((24, 24), 4, 2., 65, 'float32')
    im[12, 12] = np.inf
    out.append(('inf_f32', im, 5, 64, None, True))
    out.append(('small_u8', blobs((6, 5), 2, 2., 66, 'uint8', 2.), 13, 64, 0, True))
    out.append(('small3d_i16', blobs((3, 5, 4), 2, 2., 67, 'int16', 3.), (9, 17, 17), 64, 0, True))
    out.append(('sep_below_1_u8', blobs((16, 16), 4, 1., 68, 'uint8', 2.), 0.9, 64, None, True))
    out.append(('sep_half_f32', blobs((16, 16), 4, 1., 69, 'float32'), 0.5, 64, None, True))
    out.append(('big_margin_u8', blobs((20, 20), 4, 2., 70, 'uint8', 2.), 5, 64, 10, True))
    # wide integer values: NumPy's b - a wraps in the pixel type
    im = np.zeros((20, 20), np.int16)
    im[::2, ::3] = -30000
    im[1::2, 1::3] = 30000
    out.append(('wrap_i16', im, 3, 50, None, True))
    im = np.zeros((20, 20), np.int32)
    im[::2, ::3] = -2000000000
    im[1::2, 1::3] = 2000000000
    out.append(('wrap_i32', im, 3, 50, None, True))
    for p in (0, 33.3, 99.9, 100):
        out.append(('pct_%g_f32' % p, blobs((24, 24), 5, 2., 71, 'float32'), 5, p, None, True))
        out.append(('pct_%g_u16' % p, blobs((24, 24), 5, 2., 72, 'uint16', 50.), 5, p, None, True))
    # cfg-2-like and cfg-3-like crops (workloads.cfg2 / cfg3 geometry and statistics)
    im, _, _ = artificial.random_frame((96, 96), 12, 3., 100, 10, seed=73, margin=13)
    out.append(('cfg2_crop', im, 13, 64, None, True))
    im, _, _ = artificial.random_frame((24, 48, 48), 10, (2., 4., 4.), 100, 10, seed=74, margin=(9, 17, 17))
    out.append(('cfg3_crop', im, (9, 17, 17), 64, None, True))
    return out


def main():
    ref = refshim.load()
    arrays, names = {}, []
    for i, (name, frame, sep, pct, margin, precise) in enumerate(cases()):
        pos = ref.find.grey_dilation(frame, sep, percentile=pct, margin=margin, precise=precise)
        thr = ref.find.percentile_threshold(frame, pct)
        names.append(name)
        arrays['frame_%d' % i] = frame
        arrays['args_%d' % i] = np.array(json.dumps(dict(
            separation=list(sep) if isinstance(sep, tuple) else sep, percentile=pct,
            margin=list(margin) if isinstance(margin, tuple) else margin, precise=precise)))
        arrays['pos_%d' % i] = np.asarray(pos)
        arrays['thr_%d' % i] = np.array(thr, dtype=np.float64)
        print('%-22s %-8s %3d maxima' % (name, frame.dtype, len(pos)))
    arrays['names'] = np.array(json.dumps(names))
    np.savez_compressed(os.path.join(HERE, 'locate', 'locate_cases.npz'), **arrays)


if __name__ == '__main__':
    main()
