"""``ctr_train_device`` on the GPU: against the reference's fixtures (convergence, cost, status),
against the NumPy yardstick of ``tests/_train.py`` at the edges of the kernels, in batches, on
streams, and end to end through ``train_leastsq``.

Tolerances against the yardstick.  The device runs to the rounding floor (train.py: xtol 1e-15,
ftol 1e-30, flat trials judged by the projected gradient); the yardstick is the less converged
side: SciPy's ``least_squares`` judges a step by F, whose sum rounds at eps F while F - Fmin is
quadratic in the distance, so it cannot resolve the minimum more closely than a relative
sqrt(eps) = 1.5e-8, times the conditioning of the problem (several shared values, a flat valley).
RTOL_GLOBALS = 1e-7 allows a factor 7 for that; the cost is stationary at the minimum, so it
differs in second order (1e-14) and by the rounding of a sum of a few thousand squares (1e-13):
RTOL_COST = 1e-10 is far above both and far below any error of the rule."""
import numpy as np
import pandas as pd
import pytest

import _train
import clustertracking_amd as ct
from clustertracking_amd import _abi, artificial, train

pytestmark = pytest.mark.gpu

CASES = _train.load_cases()
NAMES = sorted(n for n in CASES if CASES[n]['solution'])      # (the others are start-only entries)
R = 8          # train_kernels.h: TRN_R, clusters summed side by side by the step kernel
RTOL_GLOBALS, RTOL_COST = 1e-7, 1e-10


def _bounds(case):
    return {k: tuple(v) for k, v in case['call']['bounds'].items()}


def _run_case(case, **kw):
    call = case['call']
    off = np.array([0, len(case['frame_index'])], dtype=np.int32)
    return ct.train_arrays(case['frames'], case['params'], case['feat_offset'], case['frame_index'], off,
                           call['diameter'], call['fit_function'], bounds=_bounds(case),
                           max_rms_dev=call.get('max_rms_dev', 1.), **kw)


@pytest.fixture(scope='module')
def fixture_results():
    return {name: _run_case(CASES[name]) for name in NAMES}


@pytest.mark.parametrize('name', NAMES)
def test_fixture_convergence_cost_and_status(fixture_results, name):
    """at least as converged as the reference's tight run; cost within ten times the reference's own
    A-vs-B scatter of the case; the failed case fails alike.
    Measured: see DESIGN.md 7b (the figures are printed here before they are asserted)."""
    case, res = CASES[name], fixture_results[name]
    if case['fails']:
        assert res.status[0] == _abi.STATUS_RMS_DEV and np.isnan(res.cost[0]) and np.isnan(res.globals[0]).all()
        return
    assert res.status[0] == _abi.STATUS_OK
    prob = _train.problem_of(case)
    pg_dev = np.abs(prob.projected_gradient(res.globals[0], case['low'], case['high'])).max()
    pg_ref = np.abs(prob.projected_gradient(case['B_globals'], case['low'], case['high'])).max()
    rel_cost = abs(res.cost[0] - float(case['B_cost'])) / float(case['B_cost'])
    x = prob.solve(case['low'], case['high'])
    print('%s: projected gradient device %.3e reference B %.3e; cost vs B %.2e (allowed %.2e); globals vs yardstick '
          '%.2e, cost vs yardstick %.2e; iterations %d'
          % (name, pg_dev, pg_ref, rel_cost, 10 * float(case['scatter_cost']),
             np.max(np.abs(res.globals[0] - x) / np.abs(x)), abs(res.cost[0] - prob.cost(x)) / prob.cost(x),
             res.n_iter[0]))
    assert pg_dev <= pg_ref
    assert rel_cost <= 10 * float(case['scatter_cost'])


def seeded(seed, grid, pitch, diameter, size, fit='gauss', dtype=np.uint8, signal=100, noise=3, start=1.15,
           extras=None, per_cluster=1, shift=None):
    """A drawn problem: features on a grid (``grid`` cells of ``pitch`` pixels per axis), groups of
    ``per_cluster`` consecutive features forming a cluster; returns what train_arrays takes."""
    nd = len(grid)
    rng = np.random.RandomState(seed)
    dia = tuple(diameter) if hasattr(diameter, '__iter__') else (diameter,) * nd
    size = tuple(size) if hasattr(size, '__iter__') else (size,) * nd
    iso = all(d == dia[0] for d in dia)
    margin = [d // 2 + 2 for d in dia]
    shape = tuple(int(2 * m + (g - 1) * pitch + 1) for m, g in zip(margin, grid))
    cells = np.stack(np.meshgrid(*[m + pitch * np.arange(g) for m, g in zip(margin, grid)], indexing='ij'),
                     -1).reshape(-1, nd).astype(np.float64)
    truth = cells + rng.uniform(-0.4, 0.4, cells.shape)
    if shift is not None:
        truth = truth + np.asarray(shift)
    im = np.zeros(shape, np.uint8 if np.dtype(dtype) == np.float64 else dtype)
    for p in truth:
        artificial.draw_feature(im, p, size, signal, fit if fit in ('gauss', 'ring', 'disc') else 'inv_series',
                                **(extras or {}))
    im = artificial.add_poisson_noise(im, noise, rng, saturation=np.iinfo(im.dtype).max).astype(dtype)
    names = _train.param_names(fit, nd, iso)
    params = np.zeros((len(truth), len(names)))
    params[:, 0], params[:, 1] = noise, signal
    params[:, 2:2 + nd] = truth + rng.uniform(-0.1, 0.1, truth.shape)
    nsz = 1 if iso else nd
    params[:, 2 + nd:2 + nd + nsz] = np.array(size[:nsz]) * start
    ex = extras or {}
    vals = list(ex.get('p', [])) or list(ex.values())
    for q, v in enumerate(vals):
        params[:, 2 + nd + nsz + q] = v * 1.1
    n_cl = -(-len(truth) // per_cluster)
    feat_offset = np.minimum(np.arange(n_cl + 1) * per_cluster, len(truth)).astype(np.int32)
    return dict(frames=im[None], params=params, feat_offset=feat_offset, frame_index=np.zeros(n_cl, np.int32),
                diameter=diameter, fit=fit)


def run(prob, bounds=None, **kw):
    off = np.array([0, len(prob['frame_index'])], dtype=np.int32)
    return ct.train_arrays(prob['frames'], prob['params'], prob['feat_offset'], prob['frame_index'], off,
                           prob['diameter'], prob['fit'], bounds=train_bounds(prob, bounds), **kw)


def train_bounds(prob, bounds):
    nd = prob['frames'].ndim - 1
    dia = prob['diameter'] if hasattr(prob['diameter'], '__iter__') else (prob['diameter'],) * nd
    iso = all(d == dia[0] for d in dia)
    return train.training_bounds(bounds, ['size'] if iso else ['size_' + c for c in 'zyx'[-nd:]])


def check_against_yardstick(prob, bounds=None, param_mode=None, **kw):
    res = run(prob, bounds, param_mode=param_mode, **kw)
    nd = prob['frames'].ndim - 1
    dia = prob['diameter'] if hasattr(prob['diameter'], '__iter__') else (prob['diameter'],) * nd
    ff = train.training_param_mode(prob['fit'], nd, all(d == dia[0] for d in dia), param_mode)
    off = np.array([0, len(prob['frame_index'])])
    _, low, high = train.pack_problems(ff, prob['params'], prob['feat_offset'], off, train_bounds(prob, bounds),
                                       tuple(int(d) // 2 for d in dia))
    y = _train.Problem(prob['frames'], prob['params'], prob['feat_offset'], prob['frame_index'], prob['diameter'],
                       prob['fit'], modes=ff.modes)
    x = y.solve(low[0], high[0])
    assert res.status[0] == _abi.STATUS_OK, res
    np.testing.assert_allclose(res.globals[0], x, rtol=RTOL_GLOBALS)
    np.testing.assert_allclose(res.cost[0], y.cost(x), rtol=RTOL_COST)
    return res, x, low[0], high[0]


@pytest.mark.parametrize('n_clusters', [1, R - 1, R, R + 1, 2 * R + 1])
def test_cluster_counts_around_the_chunk_of_the_reduce(n_clusters):
    check_against_yardstick(seeded(40 + n_clusters, (1, n_clusters), 16, 11, 2.5))


def test_window_of_nine_pixels():
    check_against_yardstick(seeded(50, (3, 3), 8, 3, 0.7, start=1.2, noise=1))


def test_union_box_larger_than_the_workgroup():
    prob = seeded(51, (2, 2), 30, 25, 5.)       # 25 x 25 = 625 pixels, 256 lanes
    check_against_yardstick(prob)
    check_against_yardstick(seeded(52, (2, 3), 9, 11, 2.5, per_cluster=3))     # overlapping masks in one window


def test_cluster_of_64_features_and_65_refused():
    prob = seeded(53, (8, 8), 9, 9, 2., per_cluster=64)
    assert np.diff(prob['feat_offset']).tolist() == [64]
    check_against_yardstick(prob)
    big = seeded(54, (5, 13), 9, 9, 2., per_cluster=65)
    with pytest.raises(NotImplementedError) as e:
        run(big)
    assert 'cluster 0 has 65 features' in str(e.value)
    check_against_yardstick(seeded(55, (1, 2), 16, 11, 2.5))     # a small correct call after it


@pytest.mark.parametrize('axis,side', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_clipped_window_in_each_axis(axis, side):
    prob = seeded(56 + 2 * axis + side, (2, 2), 16, 11, 2.5)
    # move the frame's edge into the windows of the features next to it
    cut = 4
    fr = prob['frames']
    sl = [slice(None)] * 3
    sl[1 + axis] = slice(cut, None) if side == 0 else slice(None, fr.shape[1 + axis] - cut)
    prob['frames'] = np.ascontiguousarray(fr[tuple(sl)])
    if side == 0:
        prob['params'][:, 2 + axis] -= cut
    check_against_yardstick(prob)


def test_3d_anisotropic_with_one_size_on_its_bound():
    prob = seeded(60, (1, 2, 2), 12, (5, 9, 9), (1.2, 2., 2.), noise=2)
    res, x, low, high = check_against_yardstick(prob, bounds=dict(size_z=(0.1, 1.0)))
    assert res.globals.shape == (1, 3) and res.globals[0, 0] == 1.0 and high[0] == 1.0


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float64])
def test_pixel_types(dtype):
    check_against_yardstick(seeded(61, (2, 2), 16, 11, 2.5, dtype=dtype, signal=100 if dtype == np.uint8 else 1000))


@pytest.mark.parametrize('fit,extras,bounds,param_mode', [
    ('ring', dict(thickness=0.3), dict(thickness=(0.1, 0.9)), None),
    ('disc', dict(disc_size=0.5), dict(disc_size=(0.1, 0.9)), None),
    # signal_mult / (r2^2 + a r2 + b) with r2 = r^2 / size^2 does not change along (mult k^4, size k, a k^2,
    # b k^4): with all four free the minimisers are a curve, so one of them is held constant
    ('inv_series_2', dict(p=[1., 1.5, 1.]), dict(param_a=(0.2, 5.), param_b=(0.2, 5.)), dict(signal_mult='const')),
])
def test_other_profiles(fit, extras, bounds, param_mode):
    prob = seeded(62, (2, 3), 24, 19, 4.5, fit=fit, extras=extras, signal=160, start=1.05)
    if param_mode:
        prob['params'][:, -3] = 1.       # signal_mult as drawn
    check_against_yardstick(prob, bounds=bounds, param_mode=param_mode)


@pytest.mark.parametrize('grid,pitch,diameter,size,fit,extras,bounds,param_mode', [
    ((2, 3), 18, (11, 15), (2., 3.), 'gauss', None, None, None),                                   # <2, aniso, gauss>
    ((2, 2), 26, (17, 21), (4., 5.), 'ring', dict(thickness=0.3), dict(thickness=(0.1, 0.9)), None),  # <2, aniso, ring>
    ((2, 2, 2), 12, 9, 2., 'gauss', None, None, None),                                             # <3, iso, gauss>
    ((1, 2, 2), 16, 13, 3., 'disc', dict(disc_size=0.5), dict(disc_size=(0.1, 0.9)), None),        # <3, iso, disc>
    ((1, 2, 2), 14, (9, 11, 11), (2., 2.5, 2.5), 'inv_series_2', dict(p=[1., 1.5, 1.]),
     dict(param_a=(0.2, 5.), param_b=(0.2, 5.)), dict(signal_mult='const')),                       # <3, aniso, inv_series>
], ids=['2d-aniso-gauss', '2d-aniso-ring', '3d-iso-gauss', '3d-iso-disc', '3d-aniso-inv2'])
def test_anisotropic_2d_and_isotropic_3d_instantiations(grid, pitch, diameter, size, fit, extras, bounds, param_mode):
    prob = seeded(90, grid, pitch, diameter, size, fit=fit, extras=extras, signal=160, start=1.05, noise=2)
    if param_mode:
        prob['params'][:, -3] = 1.       # signal_mult as drawn
    check_against_yardstick(prob, bounds=bounds, param_mode=param_mode)


def _batch(problems):
    """five problems of one geometry as one call"""
    frames = np.concatenate([p['frames'] for p in problems])
    params = np.concatenate([p['params'] for p in problems])
    n_cl = [len(p['frame_index']) for p in problems]
    feat_offset = np.concatenate([[0]] + [p['feat_offset'][1:] + o for p, o in
                                          zip(problems, np.cumsum([0] + [len(p['params']) for p in problems[:-1]]))])
    frame_index = np.repeat(np.arange(len(problems)), n_cl)
    return frames, params, feat_offset.astype(np.int32), frame_index.astype(np.int32), np.cumsum([0] + n_cl).astype(np.int32)


def _bytes(res):
    return [np.asarray(a).tobytes() for a in res]


def test_batch_equals_single_calls_bit_for_bit():
    import torch
    # frames of one shape: the same grid, different seeds and cluster counts
    problems = [seeded(70 + i, (2, 3), 16, 11, 2.5) for i in range(5)]
    for i, p in enumerate(problems):      # different cluster counts: drop features from the end
        keep = len(p['params']) - i
        p['params'], p['feat_offset'], p['frame_index'] = p['params'][:keep], p['feat_offset'][:keep + 1], p['frame_index'][:keep]
    singles = [run(p) for p in problems]
    frames, params, feat_offset, frame_index, problem_offset = _batch(problems)
    bounds = train_bounds(problems[0], None)
    both = ct.train_arrays(frames, params, feat_offset, frame_index, problem_offset, 11, 'gauss', bounds=bounds)
    assert (both.status == 0).all()
    for i, s in enumerate(singles):
        assert _bytes(s) == _bytes(type(both)(*[a[i:i + 1] for a in both]))
    # a failing problem in the middle leaves the others' bytes as they are
    bad = params.copy()
    bad[feat_offset[problem_offset[2]], 1] = np.nan
    hurt = ct.train_arrays(frames, bad, feat_offset, frame_index, problem_offset, 11, 'gauss', bounds=bounds)
    assert hurt.status.tolist() == [0, 0, _abi.STATUS_NONFINITE, 0, 0] and np.isnan(hurt.cost[2])
    for i in (0, 1, 3, 4):
        assert _bytes(type(both)(*[a[i:i + 1] for a in both])) == _bytes(type(both)(*[a[i:i + 1] for a in hurt]))
    # two calls on different streams
    out = []
    for _ in range(2):
        with torch.cuda.stream(torch.cuda.Stream()):
            out.append(ct.train_arrays(frames, params, feat_offset, frame_index, problem_offset, 11, 'gauss', bounds=bounds))
    assert _bytes(out[0]) == _bytes(out[1]) == _bytes(both)
    # reading a flag every few iterations instead of queueing blind changes nothing
    assert _bytes(ct.train_arrays(frames, params, feat_offset, frame_index, problem_offset, 11, 'gauss', bounds=bounds,
                                  check_every=4)) == _bytes(both)
    assert _bytes(ct.train_arrays(frames, params, feat_offset, frame_index, problem_offset, 11, 'gauss', bounds=bounds,
                                  check_every=0)) == _bytes(both)


def _table_of(case):
    nd = case['frames'].ndim - 1
    dia = case['call']['diameter']
    names = _train.param_names(case['call']['fit_function'], nd, not hasattr(dia, '__iter__'))
    f = pd.DataFrame(case['params'], columns=names)
    f['frame'] = np.repeat(case['frame_index'], np.diff(case['feat_offset']))
    return f


def test_train_leastsq_on_a_fixture(fixture_results):
    case = CASES['ring2d']
    got = ct.train_leastsq(_table_of(case), ct.ArrayReader(case['frames']), case['call']['diameter'], None, 'ring',
                           refine_com=False, bounds=dict(thickness=(0.1, 0.9)))
    assert list(got) == ['size', 'thickness']
    np.testing.assert_allclose([got['size'], got['thickness']], case['B_globals'], rtol=10 * float(case['scatter_globals']))
    with pytest.raises(ct.RefineException):
        c = CASES['fail_rms']
        ct.train_leastsq(_table_of(c), ct.ArrayReader(c['frames']), 13, None, 'gauss', refine_com=False, max_rms_dev=1e-3)


def test_per_frame_equals_single_frame_calls():
    case = CASES['two_frames']
    f, reader = _table_of(case), ct.ArrayReader(case['frames'])
    both = ct.train_leastsq(f, reader, 13, None, 'gauss', refine_com=False, per_frame=True)
    assert list(both.index) == [0, 1] and list(both.columns) == ['size']
    for t in (0, 1):
        one = ct.train_leastsq(f[f['frame'] == t], reader, 13, None, 'gauss', refine_com=False)
        assert one['size'] == both.loc[t, 'size']


def test_refine_com_recovers_the_drawn_size_as_the_yardstick_does():
    prob = seeded(80, (3, 3), 18, 13, 3., noise=2)
    nd = 2
    f = pd.DataFrame(prob['params'][:, 2:4] + 1., columns=['y', 'x'])      # starts a pixel off
    got = ct.train_leastsq(f, prob['frames'][0], 13, None, 'gauss', refine_com=True)
    # the yardstick from the same starts: the engine's own centre of mass and characterisation
    pos, _, _ = ct.refine_com_arrays(prob['frames'], f[['y', 'x']].values, [0, len(f)], (6, 6))
    _, signal, size = ct.characterize_arrays(prob['frames'], pos, [0, len(f)], (6, 6))
    params = np.column_stack([np.zeros(len(f)), signal, pos, size])
    y = _train.Problem(prob['frames'], params, np.arange(len(f) + 1), np.zeros(len(f), int), 13)
    x0 = y.start()
    x = y.solve(x0 * 0.1, x0 * 10.)
    np.testing.assert_allclose(got['size'], x[0], rtol=RTOL_GLOBALS)
    assert abs(got['size'] - 3.) <= abs(x[0] - 3.) + RTOL_GLOBALS * 3.
