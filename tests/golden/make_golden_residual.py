"""Generate tests/golden/residual/residual_reference.npz from the REFERENCE (build container only; needs
the reference tree, see oracle/refshim.py).  The file lies in a directory of its own, as the fixtures of
the other stages do: every ``.npz`` directly under tests/golden/ is taken for a refine fixture
(tests/_cases.py:case_names).

    python tests/golden/make_golden_residual.py

Every case is one cluster of one frame: the reference's ``prepare_subimage`` on the mask centres and
``FitFunctions.get_residual(..., norm=1.)`` on the parameters.  Stored, data only: the frame (uint8),
the parameters ``[n, n_params]``, the mask centres ``[n, ndim]``, the diameter, the name of the fit
function, and the reference's value and pixel count.  tests/test_residual_rule.py compares the NumPy
restatement with them, tests/test_gpu_residual.py the device.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import refshim  # noqa: E402

ct = refshim.load()
from clustertracking import refine as ct_refine  # noqa: E402
from clustertracking.fitfunc import FitFunctions, vect_from_params  # noqa: E402

# (name, fit_function, frame shape, diameter, profile parameters, features, what it is there for)
CASES = [
    ('gauss_2d_iso', 'gauss', (32, 32), 9, [], 2, None),
    ('gauss_2d_aniso', 'gauss', (32, 32), (7, 11), [], 3, None),
    ('gauss_3d_aniso', 'gauss', (12, 24, 24), (5, 9, 9), [], 2, None),
    ('gauss_3d_iso', 'gauss', (12, 24, 24), 7, [], 4, None),
    ('gauss_2d_edge', 'gauss', (32, 32), 11, [], 2, 'edge'),
    ('gauss_2d_moved_mask', 'gauss', (32, 32), 9, [], 3, 'moved'),
    ('ring_2d_iso', 'ring', (32, 32), 11, [0.4], 2, None),
    ('ring_2d_near_pixel', 'ring', (32, 32), 11, [0.5], 2, 'near'),
    ('ring_3d_aniso', 'ring', (12, 24, 24), (5, 9, 9), [0.6], 2, None),
    ('disc_0_2d', 'disc', (32, 32), 9, [0.], 2, None),
    ('disc_half_2d_aniso', 'disc', (32, 32), (9, 11), [0.5], 3, None),
    ('disc_clamped_3d', 'disc', (12, 24, 24), 7, [1.25], 2, None),
    ('inv_series_2_2d', 'inv_series_2', (32, 32), 9, [1.5, 0.75, 2.], 3, None),
    ('inv_series_2_3d_aniso', 'inv_series_2', (12, 24, 24), (5, 7, 7), [0.75, 1.25, 0.5], 2, None),
]


def make_case(rng, fit, shape, diameter, extra, n, what):
    ndim = len(shape)
    diam = tuple(diameter) if hasattr(diameter, '__iter__') else (diameter,) * ndim
    radius = tuple(d // 2 for d in diam)
    isotropic = all(d == diam[0] for d in diam)
    ff = FitFunctions(fit, ndim, isotropic)
    # centres a few pixels apart so that the masks overlap, away from the edge unless asked for
    base = np.array([s / 2. for s in shape]) + rng.uniform(-1, 1, ndim)
    step = np.zeros(ndim)
    step[-1] = radius[-1] * 0.9
    pos = np.array([base + (k - (n - 1) / 2.) * step + rng.uniform(-0.5, 0.5, ndim) for k in range(n)])
    if what == 'edge':
        pos[:, -2] = rng.uniform(0.6, 2.4, n)            # the masks stick out of the frame
    if what == 'near':
        pos[0] = np.round(pos[0]) + rng.uniform(-0.3, 0.3, ndim)   # pixels within one pixel of the centre
    centres = pos + rng.uniform(-0.6, 0.6, pos.shape) if what == 'moved' else pos.copy()
    sizes = rng.uniform(0.25, 0.4, (n, 1 if isotropic else ndim)) * np.array(radius[:1] if isotropic else radius)
    params = np.concatenate([np.full((n, 1), 10.25), rng.uniform(60, 150, (n, 1)), pos, sizes,
                             np.tile(np.array(extra, dtype=np.float64), (n, 1)).reshape(n, len(extra))], axis=1)
    assert params.shape[1] == len(ff.params)
    # the frame: blobs where the features are, on a noisy background
    grid = np.indices(shape, dtype=np.float64)
    frame = rng.uniform(5, 25, shape)
    for k in range(n):
        r2 = sum(((grid[a] - pos[k, a]) / (0.35 * radius[a])) ** 2 for a in range(ndim))
        frame += params[k, 1] * np.exp(-0.5 * ndim * r2)
    frame = np.clip(np.round(frame), 0, 255).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sub, mesh, masks = ct_refine.prepare_subimage(centres, frame, radius)
        residual, _ = ff.get_residual([sub], [mesh], [masks], params, None, 1.)
        vect = vect_from_params(params, ff.modes, None, operation=np.mean)
        value = float(residual(vect))
    return dict(frame=frame, params=params, centres=centres, diameter=np.array(diam, dtype=np.int64),
                fit=np.array(fit), value=np.array(value), n_pix=np.array(len(sub), dtype=np.int64))


def main():
    rng = np.random.RandomState(20261020)
    out = {'names': np.array([c[0] for c in CASES])}
    for name, fit, shape, diameter, extra, n, what in CASES:
        case = make_case(rng, fit, shape, diameter, extra, n, what)
        assert np.isfinite(case['value']), name
        for key, val in case.items():
            out['%s__%s' % (name, key)] = val
        print('%-24s n_pix %5d value %.17g' % (name, case['n_pix'], case['value']))
    os.makedirs(os.path.join(HERE, 'residual'), exist_ok=True)
    path = os.path.join(HERE, 'residual', 'residual_reference.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
