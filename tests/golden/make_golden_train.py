"""Generate tests/golden/train/train_cases.npz from the REFERENCE: what its own global-mode
``refine_leastsq`` (the body of ``train_leastsq``, refine.py:491-515, without the trackpy
``refine_com`` step that is not part of its tree) returns for small training problems.

Run in the build container only (needs /root/reference; see oracle/refshim.py):

    python tests/golden/make_golden_train.py

Positions, signal and background are ``'const'``, everything else ``'global'``, and
``size_rel_diff = (0.9, 9)`` as ``train_leastsq`` adds it.  Every case runs with ``tol=1e-7`` (A,
the default of ``train_leastsq``) and with ``make_golden.TIGHT`` (B).  The file holds data only:
per case the frames, the parameter rows in (frame, cluster) order with their offsets, the call
(JSON), the globals and cost of A and B, the reference's packed start vector and bounds, its
objective and gradient at the start, and the relative A-vs-B scatter of the globals and of the
cost.  A scatter is recorded as at least one unit in the last place of a float64 (2.2e-16): two
float64 results cannot be said to agree more closely than that.

Ring, disc and inv_series cases carry explicit bounds on the profile's own parameters and a
``signal`` that matches what was drawn: without them SLSQP wanders off (thickness to 1.9,
disc_size to 18).  A case's SOLUTION is kept (``solution`` = 1) only when A and B agree within ten
times the scatter that the reference showed on such problems (globals 1e-9 gauss / 1e-8 others,
cost 1.4e-15) or both fail; a case that misses that stays in the file as a start-only entry
(``solution`` = 0): its inputs, packed start and bounds, objective and gradient at the start do not
depend on SLSQP and pin the rule all the same.
"""
import json
import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (loads the reference through oracle/refshim.py)
from make_golden import ct, ct_refine, FitFunctions, vect_from_params, find_clusters, TIGHT  # noqa: E402
from clustertracking_amd import artificial  # noqa: E402

EPS = float(np.finfo(np.float64).eps)
KEEP_GLOBALS = {'gauss': 1e-9 * 10}
KEEP_GLOBALS_OTHER = 1e-8 * 10
KEEP_COST = 1.4e-15 * 10


def draw(shape, truth, size, signal, fit_function, noise, seed, **kw):
    im = np.zeros(shape, np.uint8)
    func = fit_function if fit_function in ('gauss', 'ring', 'disc') else 'inv_series'
    for p in truth:
        artificial.draw_feature(im, p, size, signal, func, **kw)
    return artificial.add_poisson_noise(im, noise, np.random.RandomState(seed + 1000))


def scattered(shape, n, margin, min_dist, seed):
    """n positions at least min_dist apart: cells of a grid of pitch min_dist + 2, each jittered by
    up to a pixel"""
    rng = np.random.RandomState(seed)
    pitch = min_dist + 2.
    axes = [np.arange(m + 1., s - 1. - m - 1., pitch) for s, m in zip(shape, margin)]
    cells = np.stack(np.meshgrid(*axes, indexing='ij'), -1).reshape(-1, len(shape))
    if len(cells) < n:
        raise ValueError("%d cells for %d positions" % (len(cells), n))
    pick = rng.permutation(len(cells))[:n]
    return cells[np.sort(pick)] + rng.uniform(-1., 1., (n, len(shape)))


def make_table(pos, frame, signal, sizes, extras, background):
    ndim = pos.shape[1]
    f = pd.DataFrame(pos, columns=['z', 'y', 'x'][-ndim:])
    f['frame'] = frame
    f['signal'] = float(signal)
    f['background'] = float(background)
    for k, v in list(sizes.items()) + list(extras.items()):
        f[k] = float(v)
    return f


class Reader(object):
    def __init__(self, frames):
        self.frames = frames
        self.frame_shape = frames.shape[1:]

    def __getitem__(self, i):
        return self.frames[i]


def run_case(name, frames, f0, call):
    ndim = frames.ndim - 1
    diameter = call['diameter']
    dia = tuple(diameter) if hasattr(diameter, '__iter__') else (diameter,) * ndim
    radius = tuple(int(d) // 2 for d in dia)
    isotropic = all(d == dia[0] for d in dia)
    fit = call['fit_function']
    plain = FitFunctions(fit, ndim, isotropic)
    param_mode = {p: ('const' if p in plain.pos_columns + ['signal', 'background'] else 'global')
                  for p in plain.params}
    bounds = dict(call.get('bounds') or {})
    for col in plain.size_columns:
        bounds.setdefault(col + '_rel_diff', (0.9, 9))
    ff = FitFunctions(fit, ndim, isotropic, param_mode)
    sep = call.get('separation') or dia
    # rows in (frame, cluster) order, so that the reference's order of summation is the table's
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        f = find_clusters(f0.copy(), sep, ff.pos_columns)
    f = f.sort_values(['frame', 'cluster'], kind='stable').reset_index(drop=True)
    f0 = f.drop(columns=['cluster', 'cluster_size'])
    for col in ff.params:
        if col not in f0:
            f0[col] = ff.default[col]
            f[col] = ff.default[col]
    params = f[ff.params].values.astype(np.float64)
    key = f['frame'].values.astype(np.int64) * (int(f['cluster'].max()) + 1) + f['cluster'].values
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    feat_offset = np.append(starts, len(f)).astype(np.int32)
    frame_index = f['frame'].values[starts].astype(np.int32)

    kwargs = dict(fit_function=fit, param_mode=param_mode, bounds=bounds, separation=call.get('separation'),
                  max_rms_dev=call.get('max_rms_dev', 1.))
    reader = Reader(frames)
    res = {}
    for tag, extra in (('A', dict(tol=1e-7)), ('B', TIGHT)):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            out = ct.refine_leastsq(f0.copy(), reader, diameter, **dict(kwargs, **extra))
        cols = [p for p in ff.params if param_mode[p] == 'global']
        cost = float(out['cost'].iloc[0])
        res[tag] = (np.array([out[c].mean() for c in cols]) if np.isfinite(cost) else np.full(len(cols), np.nan), cost)

    # the reference's packed start, bounds, objective and gradient at the start (refine.py:345-371)
    f_temp = f.reset_index()
    groups = [list(f_temp.groupby('cluster').indices.values())]
    frame_nos = f['frame'].values
    norm = max(float(frames[int(i)].max()) for i in np.unique(frame_nos)) ** 2 / 100000.
    vect = vect_from_params(params, ff.modes, groups, operation=np.mean)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        bnds = ff.compute_bounds(ff.validate_bounds(bounds, radius=radius), params, groups)
    sub, meshes, masks = ct_refine.prepare_subimages(params[:, 2:2 + ndim], groups, frame_nos, reader, radius)
    residual, jacobian = ff.get_residual(sub, meshes, masks, params, groups, norm)
    case = {'frames': frames, 'params': params, 'feat_offset': feat_offset, 'frame_index': frame_index,
            'call': np.array(json.dumps(dict(call, bounds=bounds))),
            'A_globals': res['A'][0], 'A_cost': np.array(res['A'][1]),
            'B_globals': res['B'][0], 'B_cost': np.array(res['B'][1]),
            'start': vect, 'low': bnds[:, 0], 'high': bnds[:, 1], 'F_start': np.array(residual(vect))}
    if jacobian is not None:     # (the disc profile has none: fitfunc.py:451-452)
        case['grad_start'] = jacobian(vect)
    fails = not np.isfinite(res['A'][1])
    case['solution'] = np.array(1)
    if fails != (not np.isfinite(res['B'][1])):
        print('%-22s START ONLY: A and B disagree on failure' % name)
        fails, case['solution'] = False, np.array(0)
    case['fails'] = np.array(int(fails))
    if fails or not np.isfinite(res['A'][1] + res['B'][1]):
        sg = sc = EPS
    else:
        sg = float(np.max(np.abs(res['A'][0] - res['B'][0]) / np.abs(res['B'][0])))
        sc = abs(res['A'][1] - res['B'][1]) / abs(res['B'][1])
        if sg > KEEP_GLOBALS.get(fit, KEEP_GLOBALS_OTHER) or sc > KEEP_COST:
            # SLSQP's two runs end too far apart to pin a solution; what does not depend on SLSQP (inputs,
            # packed start and bounds, objective and gradient at the start) is kept
            print('%-22s START ONLY: A-vs-B scatter globals %.2e cost %.2e' % (name, sg, sc))
            case['solution'] = np.array(0)
    case['scatter_globals'] = np.array(max(sg, EPS))
    case['scatter_cost'] = np.array(max(sc, EPS))
    print('%-22s features=%d clusters=%d  B=%s cost=%.6g  scatter %.1e / %.1e' % (
        name, len(f), len(starts), np.array2string(res['B'][0], precision=5), res['B'][1], sg, sc))
    return case


def main():
    cases = {}

    def add(name, frames, f0, call):
        case = run_case(name, np.asarray(frames), f0, call)
        if case is not None:
            cases[name] = case

    shape = (144, 144)
    # gauss, 2D isotropic
    truth = scattered(shape, 16, (14, 14), 16., 1)
    im = draw(shape, truth, 3., 100, 'gauss', 5, 1)
    p0 = truth + np.random.RandomState(11).uniform(-0.3, 0.3, truth.shape)
    add('gauss2d_iso', im[None], make_table(p0, 0, 100., dict(size=3.6), {}, 2.5),
        dict(diameter=13, fit_function='gauss'))
    # gauss, 2D anisotropic
    truth = scattered(shape, 14, (16, 16), 20., 2)
    im = draw(shape, truth, (2.5, 3.5), 110, 'gauss', 4, 2)
    p0 = truth + np.random.RandomState(12).uniform(-0.3, 0.3, truth.shape)
    add('gauss2d_aniso', im[None], make_table(p0, 0, 110., dict(size_y=3., size_x=3.), {}, 2.),
        dict(diameter=(11, 15), fit_function='gauss'))
    # gauss, 3D anisotropic
    shape3 = (24, 64, 64)
    truth = scattered(shape3, 6, (7, 11, 11), 10., 3)
    im = draw(shape3, truth, (1.5, 2.5, 2.5), 120, 'gauss', 3, 3)
    p0 = truth + np.random.RandomState(13).uniform(-0.2, 0.2, truth.shape)
    add('gauss3d_aniso', im[None], make_table(p0, 0, 120., dict(size_z=1.8, size_y=2.2, size_x=2.9), {}, 1.5),
        dict(diameter=(7, 11, 11), fit_function='gauss'))
    # ring, 2D: two globals
    truth = scattered(shape, 10, (20, 20), 26., 4)
    im = draw(shape, truth, 5., 160, 'ring', 3, 4, thickness=0.3)
    p0 = truth + np.random.RandomState(14).uniform(-0.2, 0.2, truth.shape)
    add('ring2d', im[None], make_table(p0, 0, 160., dict(size=5.5), dict(thickness=0.35), 1.5),
        dict(diameter=19, fit_function='ring', bounds=dict(thickness=(0.1, 0.9))))
    # disc, 2D
    truth = scattered(shape, 12, (16, 16), 22., 5)
    im = draw(shape, truth, 4., 160, 'disc', 3, 5, disc_size=0.5)
    p0 = truth + np.random.RandomState(15).uniform(-0.2, 0.2, truth.shape)
    add('disc2d', im[None], make_table(p0, 0, 160., dict(size=4.4), dict(disc_size=0.45), 1.5),
        dict(diameter=15, fit_function='disc', bounds=dict(disc_size=(0.1, 0.9))))
    # inv_series_2
    truth = scattered(shape, 12, (16, 16), 22., 6)
    im = draw(shape, truth, 3., 150, 'inv_series_2', 3, 6, p=[1., 1.5, 1.])
    p0 = truth + np.random.RandomState(16).uniform(-0.2, 0.2, truth.shape)
    add('inv2_2d', im[None],
        make_table(p0, 0, 150., dict(size=3.3), dict(signal_mult=1., param_a=1.2, param_b=1.), 1.5),
        dict(diameter=15, fit_function='inv_series_2',
             bounds=dict(signal_mult=(0.5, 2.), param_a=(0.2, 5.), param_b=(0.2, 5.))))
    # two frames with different maxima: the norm is the problem's, not the frame's
    t0, t1 = scattered(shape, 8, (14, 14), 18., 7), scattered(shape, 8, (14, 14), 18., 8)
    im0, im1 = draw(shape, t0, 3., 100, 'gauss', 4, 7), draw(shape, t1, 3., 180, 'gauss', 4, 8)
    p0 = np.concatenate([t0, t1]) + np.random.RandomState(17).uniform(-0.3, 0.3, (16, 2))
    f0 = make_table(p0, np.repeat([0, 1], 8), 100., dict(size=3.5), {}, 2.)
    f0.loc[f0['frame'] == 1, 'signal'] = 180.
    add('two_frames', np.stack([im0, im1]), f0, dict(diameter=13, fit_function='gauss'))
    # a close pair in one cluster: overlapping masks
    truth = scattered(shape, 9, (14, 14), 24., 9)
    truth = np.concatenate([truth, truth[:2] + [[4.5, 3.5], [-3., 5.]]])
    im = draw(shape, truth, 3., 90, 'gauss', 4, 9)
    p0 = truth + np.random.RandomState(18).uniform(-0.2, 0.2, truth.shape)
    add('close_pair', im[None], make_table(p0, 0, 90., dict(size=3.5), {}, 2.), dict(diameter=13, fit_function='gauss'))
    # windows clipped at the frame edge, in each axis
    truth = np.concatenate([scattered(shape, 8, (14, 14), 20., 10), [[3.2, 60.4], [80.7, 141.1], [2.4, 139.8]]])
    im = draw(shape, truth, 3., 100, 'gauss', 4, 10)
    p0 = truth + np.random.RandomState(19).uniform(-0.2, 0.2, truth.shape)
    add('edge_clipped', im[None], make_table(p0, 0, 100., dict(size=3.3), {}, 2.), dict(diameter=13, fit_function='gauss'))
    # the solution on a bound: 10 x the mean start size is below the drawn size
    truth = scattered(shape, 10, (14, 14), 18., 11)
    im = draw(shape, truth, 3., 100, 'gauss', 4, 11)
    p0 = truth + np.random.RandomState(20).uniform(-0.2, 0.2, truth.shape)
    add('on_bound', im[None], make_table(p0, 0, 100., dict(size=0.29), {}, 2.), dict(diameter=13, fit_function='gauss'))
    # fails by max_rms_dev
    add('fail_rms', im[None], make_table(p0, 0, 100., dict(size=3.4), {}, 2.),
        dict(diameter=13, fit_function='gauss', max_rms_dev=1e-3))

    out = {'names': np.array(json.dumps(list(cases)))}
    for name, case in cases.items():
        for key, val in case.items():
            out[name + '/' + key] = val
    os.makedirs(os.path.join(HERE, 'train'), exist_ok=True)
    path = os.path.join(HERE, 'train', 'train_cases.npz')
    np.savez_compressed(path, **out)
    print('%s: %d cases, %.1f KB' % (path, len(cases), os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
