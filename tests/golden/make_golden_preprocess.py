"""Generate tests/golden/preprocess/preprocess_cases.npz: frames run through the REFERENCE's own
``lowpass`` and ``preprocess`` (preprocessing.py:13-75, loaded through oracle/refshim.py) -- what
pins ``clustertracking_amd.preprocessing`` and tests/_preprocess.py.

    python tests/golden/make_golden_preprocess.py     (build container only: needs the reference)

The reference imports ``bandpass``, ``scalefactor_to_gamut`` and ``scale_to_gamut`` from trackpy,
which is not installed: the restated ones of tests/_preprocess.py (PARITY UNPINNED) are bound
onto the loaded ``clustertracking.preprocessing`` module; the reference's arithmetic is untouched.

Layout: ``names`` (JSON list); per case ``i``: ``raw_i`` (one frame), ``args_i`` (JSON:
noise_size, smoothing_size, threshold), ``image_i`` and ``scale_factor_i`` as the reference's
``preprocess`` returns them and, where noise_size is given, ``bandpass_i`` (the restated bandpass
with these arguments) and ``lowpass_i`` (the reference's ``lowpass(raw, noise_size)``).
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
import _preprocess  # noqa: E402
from clustertracking_amd import artificial  # noqa: E402

DTYPES = ('uint8', 'uint16', 'int16', 'int32', 'float32', 'float64')


def reference_preprocessing():
    refshim.load()
    import clustertracking.preprocessing  # noqa: F401
    mod = sys.modules['clustertracking.preprocessing']
    mod.bandpass = _preprocess.bandpass
    mod.scalefactor_to_gamut = _preprocess.scalefactor_to_gamut
    mod.scale_to_gamut = _preprocess.scale_to_gamut
    return mod


def blobs(shape, n, size, seed, dtype, scale=1., offset=0., noise=8., slope=0.):
    """Gaussian blobs plus noise plus a ramp along the last axis, scaled into the pixel type."""
    rng = np.random.RandomState(seed)
    ndim = len(shape)
    im = np.zeros(shape, dtype=np.float64)
    grid = np.indices(shape).astype(np.float64)
    for _ in range(n):
        c = [rng.uniform(0, s) for s in shape]
        r2 = sum(((g - ci) / size) ** 2 for g, ci in zip(grid, c))
        im += rng.uniform(50, 100) * np.exp(-r2 * ndim / 2)
    im += rng.uniform(0, noise, shape)
    im += slope * grid[-1]
    im = im * scale + offset
    if np.dtype(dtype).kind in 'ui':
        info = np.iinfo(dtype)
        im = np.clip(np.round(im), info.min, info.max)
    return im.astype(dtype)


def cases():
    out = []   # (name, raw, noise_size, smoothing_size, threshold)
    for k, dt in enumerate(DTYPES):
        scale = {'uint8': 1.5, 'uint16': 300., 'int16': 150., 'int32': 1e6, 'float32': 0.01, 'float64': 0.01}[dt]
        im2 = blobs((18, 23), 4, 2., k, dt, scale)
        im3 = blobs((6, 11, 13), 3, 1.5, 10 + k, dt, scale)
        out.append(('2d_%s' % dt, im2, 1, 7, None))
        out.append(('2d_axes_%s' % dt, im2, (0.5, 1.5), (5, 9), None))      # per-axis sizes
        out.append(('3d_%s' % dt, im3, 1, (3, 5, 5), None))
        out.append(('3d_axes_%s' % dt, im3, (0.7, 1, 1.2), (3, 7, 5), None))
        out.append(('none_2d_%s' % dt, im2, None, None, None))              # the noise_size=None branches
        out.append(('sigma0_%s' % dt, im2, (0, 1), (3, 5), None))           # no Gaussian along y
    out.append(('none_3d_f32', blobs((5, 8, 9), 2, 1.5, 30, 'float32', 0.02), None, None, None))
    out.append(('none_negative_f64', blobs((12, 12), 2, 2., 31, 'float64', 0.02, -0.5), None, None, None))
    out.append(('sigma0_all_u8', blobs((14, 15), 3, 2., 32, 'uint8', 2.), 0, 5, None))
    out.append(('sigma0_z_u16', blobs((5, 10, 12), 2, 1.5, 33, 'uint16', 100.), (0, 1, 1), (1, 5, 5), None))
    out.append(('sigma4_u8', blobs((20, 25), 3, 3., 34, 'uint8', 2.), 4, 19, None))     # 33 taps on a 20 x 25 frame
    out.append(('sigma4_f64_3d', blobs((5, 9, 10), 2, 2., 35, 'float64', 0.01), (4, 1, 4), (11, 3, 11), None))
    out.append(('wide_box_u8', blobs((9, 12), 2, 2., 36, 'uint8', 2.), 1, 31, None))    # box wider than the frame
    out.append(('wide_box_i16_3d', blobs((4, 6, 7), 2, 1.5, 37, 'int16', 100., -3000.), 1, (9, 13, 21), None))
    out.append(('wide_box_f32', blobs((8, 10), 2, 2., 38, 'float32', 0.01), 1, (25, 3), None))
    out.append(('box1_u16', blobs((16, 18), 3, 2., 39, 'uint16', 200.), (0, 0.5), (1, 3), None))   # box 1: axis skipped
    out.append(('box1_all_u8', blobs((16, 18), 3, 2., 40, 'uint8', 2.), 0, 1, -300))
    for thr in (20, 0, -15, 2.5):
        out.append(('threshold_%s_u8' % thr, blobs((16, 20), 3, 2., 41, 'uint8', 2.), 1, 7, thr))
    out.append(('threshold_neg_i32', blobs((16, 20), 3, 2., 42, 'int32', 5e5, -3e7), 1, 5, -1e6))
    out.append(('threshold_f32', blobs((16, 20), 3, 2., 43, 'float32', 0.01), 1, 7, 0.05))
    out.append(('threshold_neg_f64', blobs((16, 20), 3, 2., 44, 'float64', 0.01), 1, 7, -0.02))
    for dt in ('uint8', 'uint16', 'float32'):     # sloped background
        scale = {'uint8': 1., 'uint16': 200., 'float32': 0.004}[dt]
        out.append(('slope_%s' % dt, blobs((24, 40), 5, 2., 45, dt, scale, 10 * scale, slope=3.), 1, 9, None))
    for dt in ('int16', 'int32'):                 # signed frames with negative pixels
        scale = {'int16': 100., 'int32': 1e6}[dt]
        out.append(('negative_%s' % dt, blobs((17, 19), 3, 2., 46, dt, scale, -60 * scale), 1, 7, None))
        out.append(('negative_3d_%s' % dt, blobs((5, 9, 11), 2, 1.5, 47, dt, scale, -60 * scale), (1, 1, 1), (3, 5, 7), None))
    out.append(('row_u8', blobs((1, 40), 3, 2., 48, 'uint8', 2.), (0, 1), (1, 7), None))          # 1 x n
    out.append(('column_u16', blobs((40, 1), 3, 2., 49, 'uint16', 200.), (1, 0), (7, 1), None))   # n x 1
    out.append(('row_dark_u8', blobs((1, 40), 3, 2., 48, 'uint8', 2.), 1, 7, None))     # the y taps leave 0.4 of the row
    out.append(('row_f64', blobs((1, 33), 3, 2., 50, 'float64', 0.01), (0, 1), (1, 9), None))
    out.append(('one_pixel_planes_i16', blobs((1, 1, 30), 2, 2., 51, 'int16', 100.), (0, 0, 1), (1, 1, 7), None))
    for dt in ('uint8', 'int32', 'float32'):      # nothing above the threshold
        out.append(('all_zero_%s' % dt, np.zeros((10, 12), dtype=dt), 1, 5, None))
    # cfg-2-like (noisy) and cfg-3-like crops (workloads.cfg2 / cfg3 geometry and statistics)
    im, _, _ = artificial.random_frame((64, 64), 6, 3., 100, 10, seed=73, margin=13)
    out.append(('cfg2_crop', im, 1, 13, None))
    im, _, _ = artificial.random_frame((12, 30, 30), 4, (2., 4., 4.), 100, 10, seed=74, margin=(4, 8, 8))
    out.append(('cfg3_crop', im, 1, (9, 17, 17), None))
    return out


def main():
    ref = reference_preprocessing()
    arrays, names = {}, []
    for i, (name, raw, noise, smooth, thr) in enumerate(cases()):
        with np.errstate(divide='ignore', invalid='ignore'):
            frame = ref.preprocess(raw, noise, smooth, thr)
        names.append(name)
        arrays['raw_%d' % i] = raw
        listed = lambda v: list(v) if isinstance(v, tuple) else v
        arrays['args_%d' % i] = np.array(json.dumps(dict(noise_size=listed(noise), smoothing_size=listed(smooth), threshold=thr)))
        arrays['image_%d' % i] = np.asarray(frame)
        arrays['scale_factor_%d' % i] = np.float64(frame.metadata['scale_factor'])
        if noise is not None:
            arrays['bandpass_%d' % i] = np.asarray(ref.bandpass(raw, noise, smooth, thr))
            arrays['lowpass_%d' % i] = np.asarray(ref.lowpass(raw, noise))
        print('%-24s %-8s %-14s -> %s, scale %.6g' % (name, raw.dtype, raw.shape, np.asarray(frame).dtype,
                                                      frame.metadata['scale_factor']))
    arrays['names'] = np.array(json.dumps(names))
    os.makedirs(os.path.join(HERE, 'preprocess'), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, 'preprocess', 'preprocess_cases.npz'), **arrays)


if __name__ == '__main__':
    main()
