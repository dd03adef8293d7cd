"""Generate tests/golden/global/global_cases.npz from the REFERENCE: what its own
``refine_leastsq`` returns for small problems with a ``param_mode`` ``'global'`` (refine.py:317-332):
shared columns fitted together with per-feature and per-cluster ones.

Run where the reference's tree is present (oracle/refshim.py finds it):

    python tests/golden/make_golden_global.py

Every case runs with ``tol=1e-7`` (A) and with ``make_golden.TIGHT`` (B).  The file holds data only:
per case the frames, the parameter rows in (frame, cluster) order with their offsets, the call
(JSON), the parameter tables, cost and number of window rounds of A and B, the reference's packed
start vector and bounds, its objective and gradient at the start, the relative A-vs-B scatter of
the cost and the A-vs-B scatter of every column: the largest absolute difference over the column's
scale (the frame maximum for background and signal, 1 px for positions, the value itself for sizes
and profile columns).  A scatter is recorded as at least one unit in the last place (2.2e-16).

A case's SOLUTION is kept (``solution`` = 1) only when A and B take the same number of rounds and
agree within ten times what the reference showed on such problems (cost 2.7e-10, positions 1e-6 px,
sizes and profile columns 2e-6, signal 2e-4, background 1e-4), or both fail; any other case stays
in the file as a start-only entry (``solution`` = 0): its inputs, packed start and bounds,
objective and gradient at the start do not depend on SLSQP and pin the rule all the same.
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402,F401  (loads the reference through oracle/refshim.py)
from make_golden import ct, ct_refine, FitFunctions, vect_from_params, find_clusters, TIGHT  # noqa: E402
from make_golden_train import draw, make_table, Reader  # noqa: E402

EPS = float(np.finfo(np.float64).eps)
KEEP_COST = 2.7e-10 * 10
KEEP_COLUMN = dict(background=1e-4 * 10, signal=2e-4 * 10, pos=1e-6 * 10, other=2e-6 * 10)


def column_kind(name, ff):
    if name in ('background', 'signal'):
        return name
    return 'pos' if name in ff.pos_columns else 'other'


def counted_refine(f0, reader, diameter, kwargs):
    """the reference's result and the number of window rounds it took (calls of prepare_subimages)"""
    rounds = [0]
    inner = ct_refine.prepare_subimages

    def counting(*a, **k):
        rounds[0] += 1
        return inner(*a, **k)
    ct_refine.prepare_subimages = counting
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            out = ct.refine_leastsq(f0.copy(), reader, diameter, **kwargs)
    finally:
        ct_refine.prepare_subimages = inner
    return out, rounds[0]


def run_case(name, frames, f0, call):
    ndim = frames.ndim - 1
    diameter = call['diameter']
    dia = tuple(diameter) if hasattr(diameter, '__iter__') else (diameter,) * ndim
    radius = tuple(int(d) // 2 for d in dia)
    isotropic = all(d == dia[0] for d in dia)
    fit, param_mode, bounds = call['fit_function'], call['param_mode'], dict(call.get('bounds') or {})
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ff = FitFunctions(fit, ndim, isotropic, param_mode)
        # rows in (frame, cluster) order, so that the reference's order of the clusters is the table's
        f = find_clusters(f0.copy(), call.get('separation') or dia, ff.pos_columns)
    f = f.sort_values(['frame', 'cluster'], kind='stable').reset_index(drop=True)
    f0 = f.drop(columns=['cluster', 'cluster_size'])
    for col in ff.params:
        if col not in f0:
            f0[col] = ff.default[col]
            f[col] = ff.default[col]
    params = f[ff.params].values.astype(np.float64)
    starts = np.flatnonzero(np.r_[True, f['cluster'].values[1:] != f['cluster'].values[:-1]])
    feat_offset = np.append(starts, len(f)).astype(np.int32)
    frame_index = f['frame'].values[starts].astype(np.int32)
    fmax = max(float(frames[int(i)].max()) for i in np.unique(f['frame'].values))

    kwargs = dict(fit_function=fit, param_mode=param_mode, bounds=bounds, separation=call.get('separation'),
                  max_rms_dev=call.get('max_rms_dev', 1.))
    reader = Reader(frames)
    res = {}
    for tag, extra in (('A', dict(tol=1e-7)), ('B', TIGHT)):
        out, rounds = counted_refine(f0, reader, diameter, dict(kwargs, **extra))
        # (find_clusters gives the rows back frame by frame, in the table's order)
        res[tag] = (out[ff.params].values.astype(np.float64), float(out['cost'].iloc[0]), rounds)

    # the reference's packed start, bounds, objective and gradient at the start (refine.py:345-371)
    groups = [list(f.reset_index().groupby('cluster').indices.values())]
    assert [int(g[0]) for g in groups[0]] == [int(s) for s in starts]
    frame_nos = f['frame'].values
    norm = fmax ** 2 / 100000.
    vect = vect_from_params(params, ff.modes, groups, operation=np.mean)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        bnds = ff.compute_bounds(ff.validate_bounds(bounds, radius=radius), params, groups)
    sub, meshes, masks = ct_refine.prepare_subimages(params[:, 2:2 + ndim], groups, frame_nos, reader, radius)
    residual, jacobian = ff.get_residual(sub, meshes, masks, params, groups, norm)
    case = {'frames': frames, 'params': params, 'feat_offset': feat_offset, 'frame_index': frame_index,
            'call': np.array(json.dumps(dict(call, bounds=bounds))),
            'A_params': res['A'][0], 'A_cost': np.array(res['A'][1]), 'A_rounds': np.array(res['A'][2]),
            'B_params': res['B'][0], 'B_cost': np.array(res['B'][1]), 'B_rounds': np.array(res['B'][2]),
            'start': vect, 'low': bnds[:, 0], 'high': bnds[:, 1], 'F_start': np.array(residual(vect)),
            'grad_start': jacobian(vect)}
    a_fail, b_fail = not np.isfinite(res['A'][1]), not np.isfinite(res['B'][1])
    case['solution'] = np.array(1)
    case['fails'] = np.array(int(a_fail and b_fail))
    sc, cols = EPS, np.full(len(ff.params), EPS)
    if a_fail != b_fail:
        print('%-18s START ONLY: A and B disagree on failure' % name)
        case['solution'] = np.array(0)
    elif not a_fail:
        sc = max(abs(res['A'][1] - res['B'][1]) / abs(res['B'][1]), EPS)
        keep = res['A'][2] == res['B'][2] and sc <= KEEP_COST
        for k, col in enumerate(ff.params):
            kind = column_kind(col, ff)
            diff = np.abs(res['A'][0][:, k] - res['B'][0][:, k])
            scale = fmax if kind in ('background', 'signal') else (1. if kind == 'pos' else np.abs(res['B'][0][:, k]))
            with np.errstate(divide='ignore', invalid='ignore'):
                cols[k] = max(float(np.nanmax(np.where(diff > 0, diff / scale, 0.))), EPS)
            keep = keep and cols[k] <= KEEP_COLUMN[kind]
        if not keep:
            print('%-18s START ONLY: rounds %d / %d, scatter cost %.2e columns %s' % (
                name, res['A'][2], res['B'][2], sc, np.array2string(cols, precision=1)))
            case['solution'] = np.array(0)
    case['scatter_cost'] = np.array(sc)
    case['scatter_columns'] = cols
    print('%-18s features=%d clusters=%d rounds=%d/%d cost=%.6g  scatter cost %.1e columns %s' % (
        name, len(f), len(starts), res['A'][2], res['B'][2], res['B'][1], sc, np.array2string(cols, precision=1)))
    return case


def main():
    cases = {}

    def add(name, frames, f0, call):
        cases[name] = run_case(name, np.asarray(frames), f0, call)

    shape = (64, 64)
    rng = np.random.RandomState
    SIZE = dict(size='global')
    # 8 Gaussians of size 3, two pairs 6.5 px apart (clusters of two at separation 11)
    truth = np.array([[12., 12.], [12., 18.5], [13., 44.], [32., 30.], [36.6, 34.6], [50., 12.], [50., 50.], [30., 52.]])
    im = draw(shape, truth, 3., 100, 'gauss', 4, 1)
    p0 = truth + rng(11).uniform(-0.3, 0.3, truth.shape)
    add('gauss2d_size', im[None], make_table(p0, 0, 90., dict(size=3.4), {}, 2.),
        dict(diameter=11, fit_function='gauss', param_mode=SIZE))
    add('size_background', im[None], make_table(p0, 0, 90., dict(size=3.4), {}, 2.),
        dict(diameter=11, fit_function='gauss', param_mode=dict(size='global', background='global')))
    add('size_signal_cluster', im[None], make_table(p0, 0, 90., dict(size=3.4), {}, 2.),
        dict(diameter=11, fit_function='gauss', param_mode=dict(size='global', signal='cluster')))
    # ring: two globals, explicit bounds on the thickness.  The positions are constant: the ring's hole
    # (r2_*_safe) makes the objective jump where a centre moves past a pixel, and with free positions
    # neither SLSQP nor any other minimiser ends at a point that a second one finds again
    truth_r = np.array([[14., 14.], [14., 46.], [34., 30.], [50., 14.], [50., 48.]])
    im_r = draw(shape, truth_r, 3.2, 150, 'ring', 3, 2, thickness=0.3)
    p0_r = truth_r + rng(12).uniform(-0.2, 0.2, truth_r.shape)
    add('ring2d', im_r[None], make_table(p0_r, 0, 150., dict(size=3.4), dict(thickness=0.35), 1.5),
        dict(diameter=11, fit_function='ring', param_mode=dict(size='global', thickness='global', pos='const'),
             bounds=dict(thickness=(0.1, 0.9))))
    # two frames of different maxima: the norm is the problem's
    t0 = np.array([[14., 14.], [14., 44.], [40., 20.], [46., 48.]])
    t1 = np.array([[16., 30.], [36., 12.], [40., 44.], [42., 50.5]])
    im0, im1 = draw(shape, t0, 3., 100, 'gauss', 4, 3), draw(shape, t1, 3., 170, 'gauss', 4, 4)
    p01 = np.concatenate([t0, t1]) + rng(13).uniform(-0.3, 0.3, (8, 2))
    f01 = make_table(p01, np.repeat([0, 1], 4), 100., dict(size=3.3), {}, 2.)
    f01.loc[f01['frame'] == 1, 'signal'] = 170.
    add('two_frames', np.stack([im0, im1]), f01, dict(diameter=11, fit_function='gauss', param_mode=SIZE))
    # a start 1.6 px off: a second window round
    off = truth[[0, 2, 3, 5, 6, 7]]
    im_o = draw(shape, off, 3., 100, 'gauss', 4, 5)
    p0_o = off + np.array([[1.6, 0.], [0., -1.6], [1.15, 1.1], [-1.6, 0.], [0., 1.6], [1.1, -1.15]])
    add('off_start', im_o[None], make_table(p0_o, 0, 90., dict(size=3.3), {}, 2.),
        dict(diameter=11, fit_function='gauss', param_mode=SIZE))
    # a window clipped by the frame, on each axis
    truth_e = np.array([[3.2, 30.4], [30.7, 61.1], [60.3, 28.], [30., 2.6], [32., 32.]])
    im_e = draw(shape, truth_e, 3., 100, 'gauss', 4, 6)
    p0_e = truth_e + rng(14).uniform(-0.2, 0.2, truth_e.shape)
    add('edge_clipped', im_e[None], make_table(p0_e, 0, 90., dict(size=3.3), {}, 2.),
        dict(diameter=11, fit_function='gauss', param_mode=SIZE))
    # the global ends on its bound: the drawn size is above it
    add('global_on_bound', im[None], make_table(p0, 0, 90., dict(size=2.0), {}, 2.),
        dict(diameter=11, fit_function='gauss', param_mode=SIZE, bounds=dict(size=(0., 2.6))))
    # a position ends on its pos_diff bound
    p0_b = p0.copy()
    p0_b[2] = truth[2] + [0.5, 0.1]
    add('pos_on_bound', im[None], make_table(p0_b, 0, 90., dict(size=3.3), {}, 2.),
        dict(diameter=11, fit_function='gauss', param_mode=SIZE, bounds=dict(pos_diff=(0.3, 0.3))))
    # fails by max_rms_dev
    add('fail_rms', im[None], make_table(p0, 0, 90., dict(size=3.4), {}, 2.),
        dict(diameter=11, fit_function='gauss', param_mode=SIZE, max_rms_dev=1e-3))
    # a pure training problem: no locals
    add('training', im[None], make_table(p0, 0, 100., dict(size=3.4), {}, 2.),
        dict(diameter=11, fit_function='gauss',
             param_mode=dict(size='global', signal='const', background='const', pos='const')))

    out = {'names': np.array(json.dumps(list(cases)))}
    for name, case in cases.items():
        for key, val in case.items():
            out[name + '/' + key] = val
    os.makedirs(os.path.join(HERE, 'global'), exist_ok=True)
    path = os.path.join(HERE, 'global', 'global_cases.npz')
    np.savez_compressed(path, **out)
    kept = [n for n in cases if int(cases[n]['solution'])]
    print('%s: %d cases, %d with a solution, %.1f KB' % (path, len(cases), len(kept), os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
