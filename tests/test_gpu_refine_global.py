"""``ctr_refine_global_device`` on the GPU: against the reference's fixtures (status, rounds,
convergence, cost, every column), against the NumPy yardstick of ``tests/_global.py`` at the edges
of the kernels, in batches, on streams, and end to end through ``refine_global``.

Tolerances against the yardstick, derived as the head of ``tests/test_gpu_train.py`` derives its
own.  The device runs to the rounding floor (xtol 1e-15, ftol 1e-30, flat trials judged by the
projected gradient); the yardstick is the less converged side: SciPy's ``least_squares`` judges a
step by F, whose sum rounds at eps F while F - Fmin is quadratic in the distance, so it resolves the
minimum to a relative sqrt(eps) = 1.5e-8 times the conditioning of the problem.  With positions,
signals and backgrounds free that conditioning is the valley between background, signal and size:
the Jacobian of these problems, its columns in the units of the tolerance (the frame maximum for
background and signal, 1 px for positions, the value for sizes and profile columns), has singular
values over a range of up to 90 (``_global.conditioning``, printed per problem as ``cond``: 90 for the
inv_series problem, 43 for the cluster of 48 columns, at most 30 elsewhere).  RTOL_COLUMNS = 2e-6 of
the column's scale is sqrt(eps) times that range, rounded up.  The cost is stationary at the
minimum, differs in second order (1e-12) and by the rounding of a sum of a few thousand squares
(1e-13): RTOL_COST = 1e-10 is far above both and far below any error of the rule.  Measured: every
column within 7e-10 of the yardstick, the cost within 7e-16 (every check prints its
figures before it asserts)."""
import importlib

import numpy as np
import pandas as pd
import pytest

import _global
import clustertracking_amd as ct
from clustertracking_amd import _abi, artificial

rg = importlib.import_module('clustertracking_amd.refine_global')    # (the function shadows the submodule)

pytestmark = pytest.mark.gpu

CASES = _global.load_cases()
NAMES = sorted(n for n in CASES if CASES[n]['solution'])      # (the others are start-only entries)
R = 8          # global_kernels.h: GLB_R, clusters summed side by side by the problem kernels
RTOL_COLUMNS, RTOL_COST = 2e-6, 1e-10
SIZE = dict(size='global')


def _bounds(case):
    return {k: tuple(v) for k, v in case['call']['bounds'].items()}


def _run_case(case, **kw):
    call = case['call']
    off = np.array([0, len(case['frame_index'])], dtype=np.int32)
    return ct.refine_global_arrays(case['frames'], case['params'], case['feat_offset'], case['frame_index'], off,
                                   call['diameter'], call['fit_function'], param_mode=call['param_mode'],
                                   bounds=_bounds(case), max_rms_dev=call.get('max_rms_dev', 1.), **kw)


@pytest.fixture(scope='module')
def fixture_results():
    return {name: _run_case(CASES[name]) for name in NAMES}


@pytest.mark.parametrize('name', NAMES)
def test_fixture_status_rounds_convergence_cost_and_columns(fixture_results, name):
    """status and round count are B's; at least as converged as the reference's tight run; cost and
    every column within ten times the reference's own A-vs-B scatter of the case; the failed case
    fails alike and keeps its rows bit for bit.
    Measured: see DESIGN.md 7b (the figures are printed here before they are asserted)."""
    case, res = CASES[name], fixture_results[name]
    if case['fails']:
        assert res.status[0] == _abi.STATUS_RMS_DEV and np.isnan(res.cost[0]) and np.isnan(res.globals[0]).all()
        assert res.params.tobytes() == case['params'].tobytes()
        return
    prob = _global.problem_of(case)
    low, high = case['low'], case['high']
    if int(case['B_rounds']) > 1:      # the gradient is judged on the windows of the last round: the masks sit on
        x1 = prob.refine(low, high, int(case['B_rounds']) - 1)[0]      # the positions of the round before it
        prob.set_windows(prob.rows_of(x1)[:, 2:2 + prob.ndim])
    pg_dev = np.abs(prob.projected_gradient(prob.pack(res.params, np.mean), low, high)).max()
    pg_ref = np.abs(prob.projected_gradient(prob.pack(case['B_params'], np.mean), low, high)).max()
    rel_cost = abs(res.cost[0] - float(case['B_cost'])) / float(case['B_cost'])
    err = _global.column_error(prob, res.params, case['B_params'], float(case['frames'].max()))
    print('%s: status %d rounds %d (B %d) iterations %d; projected gradient device %.3e reference B %.3e; cost vs B '
          '%.2e (allowed %.2e); columns vs B %s (allowed %s)'
          % (name, res.status[0], res.n_rounds[0], int(case['B_rounds']), res.n_iter[0], pg_dev, pg_ref, rel_cost,
             10 * float(case['scatter_cost']), np.array2string(err, precision=1),
             np.array2string(10 * case['scatter_columns'], precision=1)))
    assert res.status[0] == _abi.STATUS_OK and res.n_rounds[0] == int(case['B_rounds'])
    assert pg_dev <= pg_ref
    assert rel_cost <= 10 * float(case['scatter_cost'])
    assert (err <= 10 * case['scatter_columns']).all()
    g = [k for k, m in enumerate(prob.modes) if m == _global.GLOBAL]
    assert res.global_names == [prob.names[k] for k in g] and np.array_equal(res.globals[0], res.params[0, g])


# ---- drawn problems against the yardstick ---------------------------------------------------------

OFFSETS = np.array([[0., 0.], [0., 5.5], [5.5, 0.3], [5.2, 5.6]])


def drawn(seed, clusters, diameter, size, fit='gauss', dtype=np.uint8, shape=None, signal=100, noise=3, start=1.1,
          extras=None, jitter=0.1, frames=1):
    """A drawn problem: ``clusters`` a list of [k, ndim] position arrays, one cluster each (cluster c in
    frame c % frames); returns what refine_global_arrays takes."""
    nd = len(clusters[0][0])
    rng = np.random.RandomState(seed)
    dia = tuple(diameter) if hasattr(diameter, '__iter__') else (diameter,) * nd
    size = tuple(size) if hasattr(size, '__iter__') else (size,) * nd
    iso = all(d == dia[0] for d in dia)
    truth = np.concatenate(clusters).astype(np.float64)
    if shape is None:
        shape = tuple(int(truth[:, a].max() + dia[a] // 2 + 3) for a in range(nd))
    kind = np.uint8 if np.dtype(dtype) == np.float64 else dtype
    ims = [np.zeros(shape, kind) for _ in range(frames)]
    for c, cl in enumerate(clusters):
        for p in cl:
            artificial.draw_feature(ims[c % frames], p, size, signal,
                                    fit if fit in ('gauss', 'ring', 'disc') else 'inv_series', **(extras or {}))
    ims = [artificial.add_poisson_noise(im, noise, rng, saturation=np.iinfo(kind).max).astype(dtype) for im in ims]
    names = _global.param_names(fit, nd, iso)
    params = np.zeros((len(truth), len(names)))
    params[:, 0], params[:, 1] = noise, signal * 0.9
    params[:, 2:2 + nd] = truth + rng.uniform(-jitter, jitter, truth.shape)
    nsz = 1 if iso else nd
    params[:, 2 + nd:2 + nd + nsz] = np.array(size[:nsz]) * start
    ex = extras or {}
    vals = list(ex.get('p', [])) or list(ex.values())
    for q, v in enumerate(vals):
        params[:, 2 + nd + nsz + q] = v * 1.1
    feat_offset = np.concatenate([[0], np.cumsum([len(c) for c in clusters])]).astype(np.int32)
    return dict(frames=np.stack(ims), params=params, feat_offset=feat_offset,
                frame_index=(np.arange(len(clusters)) % frames).astype(np.int32), diameter=diameter, fit=fit)


def singles(n, pitch, margin, nd=2):
    return [np.array([[margin + 0.3] * (nd - 1) + [margin + pitch * i + 0.2]]) for i in range(n)]


def run(prob, param_mode, bounds=None, **kw):
    off = np.array([0, len(prob['frame_index'])], dtype=np.int32)
    return ct.refine_global_arrays(prob['frames'], prob['params'], prob['feat_offset'], prob['frame_index'], off,
                                   prob['diameter'], prob['fit'], param_mode=param_mode, bounds=bounds, **kw)


def yardstick(prob, param_mode, bounds=None):
    nd = prob['frames'].ndim - 1
    dia = prob['diameter'] if hasattr(prob['diameter'], '__iter__') else (prob['diameter'],) * nd
    iso = all(d == dia[0] for d in dia)
    ff = rg.global_param_mode(prob['fit'], nd, iso, param_mode)
    off = np.array([0, len(prob['frame_index'])])
    start, low, high, ls, ll, lh, _ = rg.pack_problems(ff, prob['params'], prob['feat_offset'], off, bounds,
                                                       tuple(int(d) // 2 for d in dia))
    y = _global.Problem(prob['frames'], prob['params'], prob['feat_offset'], prob['frame_index'], prob['diameter'],
                        prob['fit'], modes=ff.modes)
    return y, _global.host_vector(y, low[0], ll), _global.host_vector(y, high[0], lh)


def check_against_yardstick(prob, param_mode=SIZE, bounds=None, rounds=None, **kw):
    res = run(prob, param_mode, bounds, **kw)
    y, low, high = yardstick(prob, param_mode, bounds)
    x, cost, n_rounds = y.refine(low, high, kw.get('max_iter', 10), kw.get('max_shift', 1.))
    fmax = float(prob['frames'].max())
    err = _global.column_error(y, res.params, y.rows_of(x), fmax)
    print('status %d rounds %d (yardstick %d) iterations %d cond %.1f; cost vs yardstick %.2e; columns %s'
          % (res.status[0], res.n_rounds[0], n_rounds, res.n_iter[0], _global.conditioning(y, x, fmax),
             abs(res.cost[0] - cost) / cost, np.array2string(err, precision=1)))
    assert res.status[0] == _abi.STATUS_OK, res
    assert res.n_rounds[0] == n_rounds and (rounds is None or n_rounds == rounds)
    np.testing.assert_allclose(res.cost[0], cost, rtol=RTOL_COST)
    assert (err <= RTOL_COLUMNS).all(), err
    return res, y, x, low, high


@pytest.mark.parametrize('n_clusters', [1, R - 1, R, R + 1, 2 * R + 1])
def test_cluster_counts_around_the_chunk_of_the_reduce(n_clusters):
    check_against_yardstick(drawn(40 + n_clusters, singles(n_clusters, 14, 8), 11, 2.5, shape=(20, 14 * n_clusters + 6)))


def cluster_at(anchor, k):
    return np.asarray(anchor, dtype=np.float64) + OFFSETS[:k]


def test_cluster_sizes_one_to_four_in_one_problem():
    """4, 7, 10 and 13 locals: clusters of different length share one scratch row size"""
    clusters = [cluster_at((8, 8 + 22 * i), k) for i, k in enumerate((3, 1, 4, 2, 1))]
    res, y, x, _, _ = check_against_yardstick(drawn(60, clusters, 11, 2.6))
    assert y.nvar == 1 + 5 + 3 * 11


def grid_cluster(n, pitch=4.5, margin=7.):
    return np.array([[margin + pitch * (i // 4), margin + pitch * (i % 4) + 0.2 * (i // 4)] for i in range(n)])


def test_a_cluster_of_48_columns_and_one_beyond():
    """15 features: 1 + 45 locals, a global and the residual fill three tiles of 16 columns"""
    prob = drawn(61, [grid_cluster(15)], 9, 2.2, noise=2, shape=(36, 36))
    res, y, _, _, _ = check_against_yardstick(prob)
    assert y.nvar + 1 == 48
    # 16 features are 51 columns: with max_locals stated as 46 the device refuses that problem alone
    big = drawn(62, [grid_cluster(16)], 9, 2.2, noise=2, shape=(36, 36))
    small = drawn(63, singles(2, 14, 8), 9, 2.2, shape=(36, 36))
    frames = np.concatenate([small['frames'], big['frames'], small['frames']])
    params = np.concatenate([small['params'], big['params'], small['params']])
    feat_offset = np.array([0, 1, 2, 18, 19, 20], dtype=np.int32)
    out = ct.refine_global_arrays(frames, params, feat_offset, [0, 0, 1, 2, 2], [0, 2, 3, 5], 9, param_mode=SIZE, max_locals=46)
    alone = run(small, SIZE, max_locals=46)
    assert list(out.status) == [_abi.STATUS_OK, _abi.STATUS_TOO_LARGE, _abi.STATUS_OK]
    assert out.params[2:18].tobytes() == big['params'].tobytes() and np.isnan(out.cost[1])
    assert out.params[:2].tobytes() == alone.params.tobytes() == out.params[18:].tobytes()
    assert out.cost[0].tobytes() == alone.cost[0].tobytes() == out.cost[2].tobytes()


def test_window_of_nine_pixels():
    check_against_yardstick(drawn(50, [np.array([[3.2, 3.1 + 8 * i]]) for i in range(6)], 3, 0.7, noise=1, start=1.15,
                                  jitter=0.05, shape=(8, 50)), param_mode=dict(size='global', pos='const'))


def test_window_of_25_by_25():
    check_against_yardstick(drawn(51, singles(3, 30, 15), 25, 5., shape=(32, 92)))


@pytest.mark.parametrize('corner', ['low', 'high'])
def test_windows_clipped_by_the_frame(corner):
    """on each axis, at the low and at the high side"""
    if corner == 'low':
        clusters = [np.array([[2.3, 20.4]]), np.array([[21.2, 1.8]]), np.array([[20., 20.]])]
    else:
        clusters = [np.array([[37.6, 20.4]]), np.array([[20.3, 38.1]]), np.array([[20., 20.]])]
    check_against_yardstick(drawn(52, clusters, 11, 2.5, shape=(40, 40)))


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float64])
def test_pixel_types(dtype):
    check_against_yardstick(drawn(53, singles(4, 14, 8), 11, 2.5, dtype=dtype, signal=100 if dtype == np.uint8 else 180))


def test_gauss_2d_anisotropic():
    check_against_yardstick(drawn(54, singles(4, 18, 10), (9, 13), (2., 3.)), param_mode=dict(size='global'))


def test_gauss_3d_isotropic():
    clusters = [np.array([[7.2, 7.4, 7.1 + 13 * i]]) for i in range(3)]
    check_against_yardstick(drawn(55, clusters, 9, 2., shape=(15, 15, 41), noise=2))


@pytest.mark.parametrize('fit,extras,mode', [
    ('ring', dict(thickness=0.3), dict(size='global', thickness='global', pos='const')),
    ('disc', dict(disc_size=0.5), dict(size='global', disc_size='global', pos='const')),
    ('inv_series_2', dict(p=[1., 1.5, 1.]), dict(param_a='global', param_b='global')),
    ('ring', dict(thickness=0.3), dict(size='var', thickness='global', pos='const')),
])
def test_profiles(fit, extras, mode):
    """ring and disc with constant positions (their hole makes the objective jump where a centre passes a
    pixel); inv_series_2 with ``signal_mult`` and ``size`` constant (the series absorbs a rescaled r2: with
    the size free as well the problem is singular); ``size`` per feature beside a global ``thickness``"""
    bounds = dict(thickness=(0.1, 0.9), disc_size=(0.1, 0.9), param_a=(0.2, 5.), param_b=(0.2, 5.))
    bounds = {k: v for k, v in bounds.items() if k in _global.param_names(fit, 2, True)}
    check_against_yardstick(drawn(56, singles(4, 18, 10), 15, 3.2, fit=fit, extras=extras, signal=150, jitter=0.05),
                            param_mode=mode, bounds=bounds)


@pytest.mark.parametrize('mode', [dict(background='global'), dict(signal='global'),
                                  dict(size='global', background='global', signal='cluster')])
def test_global_background_and_signal(mode):
    clusters = [cluster_at((8, 8 + 20 * i), k) for i, k in enumerate((2, 1, 1))]
    check_against_yardstick(drawn(57, clusters, 11, 2.5, start=1.), param_mode=mode)


def test_a_local_and_a_global_on_their_bounds():
    prob = drawn(58, singles(4, 14, 8), 11, 2.5, start=0.8)
    prob['params'][1, 3] += 0.5
    res, y, x, low, high = check_against_yardstick(prob, bounds=dict(size=(0., 2.3), pos_diff=(0.3, 0.3)))
    at = (x <= low) | (x >= high)
    assert at[y.global_vars[0]] and at.sum() >= 2
    dev = y.pack(res.params, np.mean)
    assert np.array_equal(dev[at], x[at])      # on a bound means the bound's own bytes


def test_a_forced_second_round():
    prob = drawn(59, singles(4, 14, 9), 11, 2.5, shape=(22, 62))
    prob['params'][:, 2:4] += [[1.6, 0.], [0., -1.6], [1.15, 1.1], [-1.6, 0.]]
    check_against_yardstick(prob, rounds=2)
    one = run(prob, SIZE, max_iter=1)
    assert one.status[0] == _abi.STATUS_OK and one.n_rounds[0] == 1      # refine.py:365: the last round's result stands


def test_an_all_constant_problem_is_a_training_problem():
    prob = drawn(64, singles(9, 14, 8), 11, 2.5)
    mode = dict(size='global', signal='const', background='const', pos='const')
    bounds = dict(size_rel_diff=(0.9, 9))
    res, _, _, _, _ = check_against_yardstick(prob, param_mode=mode, bounds=bounds)
    off = np.array([0, len(prob['frame_index'])], dtype=np.int32)
    tr = ct.train_arrays(prob['frames'], prob['params'], prob['feat_offset'], prob['frame_index'], off, 11, bounds=bounds)
    np.testing.assert_allclose(res.globals[0], tr.globals[0], rtol=1e-7)      # tests/test_gpu_train.py: RTOL_GLOBALS
    np.testing.assert_allclose(res.cost[0], tr.cost[0], rtol=RTOL_COST)


# ---- batches, streams, check_every ----------------------------------------------------------------

def _three():
    probs = [drawn(70 + i, [cluster_at((8, 8 + 20 * j), k) for j, k in enumerate(ks)], 11, 2.4 + 0.2 * i, shape=(24, 64))
             for i, ks in enumerate(((1, 2, 1), (2, 1), (1, 1, 3)))]
    frames = np.concatenate([p['frames'] for p in probs])
    params = np.concatenate([p['params'] for p in probs])
    sizes = np.concatenate([np.diff(p['feat_offset']) for p in probs])
    feat_offset = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    frame_index = np.repeat(np.arange(3), [len(p['frame_index']) for p in probs]).astype(np.int32)
    problem_offset = np.concatenate([[0], np.cumsum([len(p['frame_index']) for p in probs])]).astype(np.int32)
    return probs, (frames, params, feat_offset, frame_index, problem_offset)


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[:6], b[:6]))


def test_three_problems_in_one_call_equal_three_calls():
    probs, tables = _three()
    both = ct.refine_global_arrays(*tables, 11, param_mode=SIZE, max_locals=13)
    assert list(both.status) == [0, 0, 0]
    at = 0
    for i, p in enumerate(probs):
        one = run(p, SIZE, max_locals=13)
        n = len(p['params'])
        assert both.params[at:at + n].tobytes() == one.params.tobytes()
        for a, b in zip(both[1:6], one[1:6]):
            assert a[i].tobytes() == b[0].tobytes()
        at += n
    # a NaN row in the middle problem fails that problem alone
    frames, params, feat_offset, frame_index, problem_offset = tables
    bad = params.copy()
    r = len(probs[0]['params']) + 1
    bad[r, 1] = np.nan
    out = ct.refine_global_arrays(frames, bad, feat_offset, frame_index, problem_offset, 11, param_mode=SIZE, max_locals=13)
    assert list(out.status) == [_abi.STATUS_OK, _abi.STATUS_NONFINITE, _abi.STATUS_OK]
    n0, n1 = len(probs[0]['params']), len(probs[1]['params'])
    assert out.params[:n0].tobytes() == both.params[:n0].tobytes() and out.params[n0 + n1:].tobytes() == both.params[n0 + n1:].tobytes()
    assert out.params[n0:n0 + n1].tobytes() == bad[n0:n0 + n1].tobytes() and np.isnan(out.cost[1])
    assert out.cost[[0, 2]].tobytes() == both.cost[[0, 2]].tobytes()


def test_clusters_of_one_two_and_three_tiles_in_one_call_equal_their_own_calls():
    """The largest cluster of a CALL chooses the kernel instantiation (16-column tiles of a row,
    wavefronts per cluster); the bytes of a problem must not depend on it.  Three problems whose largest
    clusters need 1, 2 and 3 tiles (4, 19 and 34 locals), each with a single as well: batched they all
    run in the three-tile instantiation, alone each in its own."""
    probs = [drawn(80 + i, [grid_cluster(k), np.array([[8., 40.3]])], 9, 2.2, noise=2, shape=(36, 52))
             for i, k in enumerate((1, 6, 11))]
    frames = np.concatenate([p['frames'] for p in probs])
    params = np.concatenate([p['params'] for p in probs])
    sizes = np.concatenate([np.diff(p['feat_offset']) for p in probs])
    feat_offset = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    frame_index = np.repeat(np.arange(3), 2).astype(np.int32)
    batch = ct.refine_global_arrays(frames, params, feat_offset, frame_index, [0, 2, 4, 6], 9, param_mode=SIZE)
    assert list(batch.status) == [0, 0, 0]
    y = yardstick(probs[2], SIZE)[0]
    assert [(rg.n_locals(rg.global_param_mode('gauss', 2, True, SIZE), k) + 2 + 15) // 16 for k in (1, 6, 11)] == [1, 2, 3]
    assert y.nvar == 1 + 2 + 3 * 12
    at = 0
    for i, p in enumerate(probs):
        one = run(p, SIZE)
        n = len(p['params'])
        assert batch.params[at:at + n].tobytes() == one.params.tobytes(), i
        for a, b in zip(batch[1:6], one[1:6]):
            assert a[i].tobytes() == b[0].tobytes(), i
        at += n
    # the table form: frames that differ in their largest cluster, per_frame against one call per frame
    f = pd.DataFrame(params[:, 2:4], columns=['y', 'x'])
    f['signal'], f['size'], f['background'] = params[:, 1], params[:, 4], params[:, 0]
    f['frame'] = np.repeat(np.arange(3), [len(p['params']) for p in probs])
    reader = ct.ArrayReader(frames)
    out = ct.refine_global(f, reader, 9, param_mode=SIZE, per_frame=True)
    cols = ['background', 'signal', 'y', 'x', 'size', 'cost']
    for t in range(3):
        one = ct.refine_global(f[f['frame'] == t], reader, 9, param_mode=SIZE)
        assert out[out['frame'] == t][cols].values.tobytes() == one[cols].values.tobytes(), t


def test_streams_and_check_every_give_the_same_bytes():
    import torch
    _, tables = _three()
    ref = ct.refine_global_arrays(*tables, 11, param_mode=SIZE)
    for k in (1, 4):
        assert _same(ref, ct.refine_global_arrays(*tables, 11, param_mode=SIZE, check_every=k))
    dev = torch.device('cuda', 0)
    t = [torch.from_numpy(x).to(dev) for x in tables]
    for _ in range(2):
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            out = ct.refine_global_arrays(*t, 11, param_mode=SIZE)
        s.synchronize()
        assert isinstance(out.params, torch.Tensor) and out.params.device == dev
        assert _same(ref, [x.cpu().numpy() for x in out[:6]])


# ---- the table forms ------------------------------------------------------------------------------

def _table(case):
    nd = case['frames'].ndim - 1
    names = _global.param_names(case['call']['fit_function'], nd, True)
    f = pd.DataFrame(case['params'], columns=names)
    f['frame'] = np.repeat(case['frame_index'], np.diff(case['feat_offset']))
    return f


def test_refine_global_end_to_end():
    case = CASES['gauss2d_size']
    call = case['call']
    f = _table(case)
    out = ct.refine_global(f, case['frames'][0], call['diameter'], param_mode=call['param_mode'], bounds=_bounds(case))
    assert {'cluster', 'cluster_size', 'cost'} <= set(out.columns) and len(out) == len(f)
    assert out['cost'].nunique() == 1 and out['size'].nunique() == 1
    assert list(out['cluster_size']) == list(np.repeat(np.diff(case['feat_offset']), np.diff(case['feat_offset'])))
    res = _run_case(case)
    assert out[list(f.columns[:5])].values.tobytes() == res.params.tobytes() and out['cost'].iloc[0] == res.cost[0]
    # positions under other names: read from and written to the table's own columns
    named = ct.refine_global(f.rename(columns=dict(y='row', x='col')), case['frames'][0], call['diameter'],
                             param_mode=call['param_mode'], bounds=_bounds(case), pos_columns=['row', 'col'])
    assert 'y' not in named.columns and \
        named[['background', 'signal', 'row', 'col', 'size', 'cost']].values.tobytes() == \
        out[['background', 'signal', 'y', 'x', 'size', 'cost']].values.tobytes()
    failed = ct.refine_global(f, case['frames'][0], call['diameter'], param_mode=call['param_mode'], max_rms_dev=1e-3)
    assert failed['cost'].isna().all() and failed[list(f.columns[:5])].values.tobytes() == case['params'].tobytes()


def test_per_frame_equals_one_call_per_frame():
    case = CASES['two_frames']
    call = case['call']
    f = _table(case)
    reader = ct.ArrayReader(case['frames'])
    out = ct.refine_global(f, reader, call['diameter'], param_mode=call['param_mode'], per_frame=True)
    assert out.groupby('frame')['cost'].nunique().tolist() == [1, 1] and out['cost'].nunique() == 2
    for t in (0, 1):
        one = ct.refine_global(f[f['frame'] == t], reader, call['diameter'], param_mode=call['param_mode'])
        cols = ['background', 'signal', 'y', 'x', 'size', 'cost']
        assert out[out['frame'] == t][cols].values.tobytes() == one[cols].values.tobytes()
