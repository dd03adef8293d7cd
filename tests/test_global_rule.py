"""The rule of the global fit (``ctr_refine_global_device``, include/ctrefine.h) without a device: the
NumPy yardstick (``tests/_global.py``) against fixtures made by the reference's own global-mode
``refine_leastsq`` (``tests/golden/make_golden_global.py``), and the host side of
``clustertracking_amd/refine_global.py``."""
import ctypes
import importlib

import numpy as np
import pandas as pd
import pytest

import _global
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib

rg = importlib.import_module('clustertracking_amd.refine_global')    # (the function shadows the submodule)

CASES = _global.load_cases()
NAMES = sorted(CASES)
KEPT = [n for n in NAMES if int(CASES[n]['solution'])]


@pytest.fixture(scope='module')
def problems():
    return {name: _global.problem_of(CASES[name]) for name in NAMES}


@pytest.fixture(scope='module')
def solutions(problems):
    """the yardstick's (vector, cost, rounds) of every case that keeps a solution, computed once"""
    out = {}
    for name in KEPT:
        case, call = CASES[name], CASES[name]['call']
        out[name] = problems[name].refine(case['low'], case['high'], call.get('max_iter', 10), call.get('max_shift', 1.))
    return out


def test_the_fixture_holds_the_cases_the_reference_kept():
    assert {'gauss2d_size', 'size_background', 'size_signal_cluster', 'ring2d', 'two_frames', 'off_start', 'edge_clipped',
            'global_on_bound', 'pos_on_bound', 'fail_rms', 'training'} <= set(NAMES)
    assert len(KEPT) >= 6
    assert CASES['fail_rms']['fails'] == 1 and sum(int(CASES[n]['fails']) for n in NAMES) == 1
    # among the kept: a cluster of two or more features, two globals, two rounds
    assert any(np.diff(CASES[n]['feat_offset']).max() >= 2 for n in KEPT)
    assert any(_global.case_modes(CASES[n]).count(_global.GLOBAL) == 2 for n in KEPT)
    assert any(int(CASES[n]['B_rounds']) == 2 for n in KEPT)
    for n in NAMES:
        c = CASES[n]
        assert c['frames'].dtype == np.uint8 and max(c['frames'].shape[1:]) <= 64
        assert 4 <= len(c['params']) <= 10 and 9 <= c['call']['diameter'] <= 11
    c = CASES['two_frames']
    assert c['frames'].shape[0] == 2 and c['frames'][0].max() != c['frames'][1].max()
    c, p = CASES['global_on_bound'], _global.problem_of(CASES['global_on_bound'])
    assert abs(c['B_params'][0, 4] - c['high'][p.global_vars[0]]) < 1e-6
    c, p = CASES['pos_on_bound'], _global.problem_of(CASES['pos_on_bound'])
    B = p.pack(c['B_params'], np.mean)
    pos = np.concatenate([p.vidx[:, 2], p.vidx[:, 3]])
    assert (np.minimum(B[pos] - c['low'][pos], c['high'][pos] - B[pos]) < 1e-6).any()
    assert _global.problem_of(CASES['training']).nvar == 1
    rad = CASES['edge_clipped']['call']['diameter'] // 2
    assert (CASES['edge_clipped']['params'][:, 2:4].min() < rad)


@pytest.mark.parametrize('name', NAMES)
def test_objective_and_gradient_at_the_start(problems, name):
    case, prob = CASES[name], problems[name]
    x0 = case['start']
    np.testing.assert_allclose(prob.F(x0), float(case['F_start']), rtol=1e-12)
    np.testing.assert_allclose(prob.grad(x0), case['grad_start'], rtol=1e-12, atol=1e-12 * np.abs(case['grad_start']).max())


@pytest.mark.parametrize('name', NAMES)
def test_gradient_equals_finite_differences(problems, name):
    prob = problems[name]
    x0 = CASES[name]['start'] * 1.01
    g = prob.grad(x0)
    for v in range(len(x0)):
        h = 1e-6 * max(1., abs(x0[v]))
        e = np.zeros_like(x0)
        e[v] = h
        fd = (prob.F(x0 + e) - prob.F(x0 - e)) / (2 * h)
        assert abs(fd - g[v]) <= 2e-6 * max(abs(g).max(), 1e-12), (name, v, fd, g[v])


@pytest.mark.parametrize('name', NAMES)
def test_start_and_bounds_equal_the_reference_packed_ones(problems, name):
    """the yardstick's packing and the host's (refine_global.pack_problems), both exactly"""
    case, call, prob = CASES[name], CASES[name]['call'], problems[name]
    nd = case['frames'].ndim - 1
    dia = (call['diameter'],) * nd
    ff = rg.global_param_mode(call['fit_function'], nd, True, call['param_mode'])
    assert ff.modes == prob.modes
    bounds = {k: tuple(v) for k, v in call['bounds'].items()}
    off = np.array([0, len(case['frame_index'])])
    start, low, high, ls, ll, lh, lm = rg.pack_problems(ff, case['params'], case['feat_offset'], off, bounds,
                                                        tuple(int(d) // 2 for d in dia))
    assert lm == max(rg.n_locals(ff, n) for n in np.diff(case['feat_offset']))
    for host, ref in ((_global.host_vector(prob, start[0], ls), case['start']),
                      (_global.host_vector(prob, low[0], ll), case['low']),
                      (_global.host_vector(prob, high[0], lh), case['high'])):
        assert np.array_equal(host, ref)
    assert np.array_equal(prob.start(), case['start'])
    lo_f, hi_f = ff.feature_bounds(ff.validate_bounds(bounds, radius=tuple(int(d) // 2 for d in dia)), case['params'])
    lo, hi = prob.bounds(lo_f, hi_f)
    assert np.array_equal(lo, case['low']) and np.array_equal(hi, case['high'])


@pytest.mark.parametrize('name', KEPT)
def test_solution_equals_the_converged_reference(problems, solutions, name):
    case, prob = CASES[name], problems[name]
    x, cost, rounds = solutions[name]
    assert rounds == int(case['B_rounds'])
    if case['fails']:
        assert cost > case['call']['max_rms_dev']
        return
    np.testing.assert_allclose(cost, float(case['B_cost']), rtol=10 * float(case['scatter_cost']))
    err = _global.column_error(prob, prob.rows_of(x), case['B_params'], float(case['frames'].max()))
    assert (err <= 10 * case['scatter_columns']).all(), (err, case['scatter_columns'])


def test_public_names():
    assert callable(ct.refine_global) and callable(ct.refine_global_arrays)
    assert 'refine_global' in ct.__all__ and 'refine_global_arrays' in ct.__all__
    assert rg.GlobalResult._fields == ('params', 'cost', 'status', 'n_rounds', 'n_iter', 'globals', 'global_names')


def _table():
    f = pd.DataFrame(dict(y=[20., 40.], x=[20., 40.], signal=100., size=3.))
    return f, np.zeros((64, 64), np.uint8)


@pytest.mark.parametrize('kw,word', [
    (dict(constraints=[dict(type='eq')]), 'constraints'),
    (dict(compute_error=True), 'compute_error'),
    (dict(noise_size=1.), 'noise_size'),
    (dict(threshold=1.), 'noise_size'),
    (dict(fit_function=dict(params=[], func=None)), 'dict'),
    (dict(param_mode=dict(size='global', y='global')), 'global position'),
    (dict(param_mode=dict(size='global', pos='global')), 'global position'),
    (dict(param_mode=dict(size='var')), 'refine_leastsq'),
    (dict(param_mode=None), 'refine_leastsq'),
    (dict(param_mode=dict(size='global', signal='particle')), 'particle'),
])
def test_unsupported_is_loud(kw, word):
    f, im = _table()
    kw = dict(dict(param_mode=dict(size='global')), **kw)
    with pytest.raises(NotImplementedError) as e:
        ct.refine_global(f, im, 13, **kw)
    assert word in str(e.value)


def test_a_cluster_beyond_the_limit_is_named():
    """16 features in one cluster: 1 + 3 * 16 locals, a global and the residual are 51 columns"""
    y, x = np.meshgrid(np.arange(4) * 4. + 20., np.arange(4) * 4. + 20., indexing='ij')
    f = pd.DataFrame(dict(y=y.ravel(), x=x.ravel(), signal=100., size=3.))
    with pytest.raises(NotImplementedError) as e:
        ct.refine_global(f, np.zeros((64, 64), np.uint8), 9, param_mode=dict(size='global'))
    assert 'cluster 0 has 16 features' in str(e.value) and '51 columns' in str(e.value)
    params = np.zeros((16, 5))
    with pytest.raises(NotImplementedError) as e:
        ct.refine_global_arrays(np.zeros((1, 64, 64), np.uint8), params, [0, 16], [0], [0, 1], 9,
                                param_mode=dict(size='global'))
    assert 'cluster 0 has 16 features' in str(e.value)


def test_general_global_mode_stays_refused_by_refine_leastsq():
    f, im = _table()
    with pytest.raises(NotImplementedError) as e:
        ct.refine_leastsq(f, im, 13, param_mode=dict(size='global'))
    assert 'train_leastsq' in str(e.value) and 'refine_global' in str(e.value)


def _descriptor(param_mode=None):
    ff = rg.global_param_mode('gauss', 2, True, param_mode or dict(size='global'))
    d = rg.descriptor(ff, (32, 40), np.uint8, 1, (6, 6))
    d.n_problems = 0        # no pointer is followed
    return d


def test_descriptor_then_handle():
    """as tests/test_stage_calls.py::test_descriptor_then_handle expects of a stage"""
    lib = _lib.load()
    call = 'ctr_refine_global_device'
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    assert lib.ctr_refine_global_device(None, None, None) == _abi.ERR_INVALID
    assert msg().startswith(call + ': ') and msg() != call + ': null handle'
    assert lib.ctr_refine_global_device(None, ctypes.byref(_descriptor()), None) == _abi.ERR_INVALID
    assert msg() == call + ': null handle'
    assert _lib.SIGNATURES[call] == _lib._stage(_abi.RefineGlobal) and callable(_lib.Engine.refine_global_device)
    assert {call, 'ctr_refine_global_plan'} <= set(_lib.EXPORTS)


def test_descriptor_modes():
    lib = _lib.load()
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    call = lambda d: lib.ctr_refine_global_device(None, ctypes.byref(d), None)
    for mode in (_abi.MODE_VAR, _abi.MODE_CLUSTER, _abi.MODE_CONST, _abi.MODE_GLOBAL):     # every mode is taken
        d = _descriptor()
        d.modes[1] = mode
        assert call(d) == _abi.ERR_INVALID and msg().endswith('null handle')
    d = _descriptor()
    d.modes[2] = _abi.MODE_GLOBAL      # a position
    assert call(d) == _abi.ERR_UNSUPPORTED and 'global position' in msg()
    d = _descriptor()
    d.modes[4] = _abi.MODE_CONST       # no global column
    assert call(d) == _abi.ERR_INVALID and 'no global parameter' in msg()
    d = _descriptor()
    d.modes[0] = _abi.MODE_VAR         # the background never varies per feature
    assert call(d) == _abi.ERR_INVALID and 'background' in msg()
    d = _descriptor()
    d.modes[3] = 7
    assert call(d) == _abi.ERR_INVALID and 'unknown param mode' in msg()
    d = _descriptor()
    d.max_features = _abi.TRAIN_MAX_FEATURES + 1
    assert call(d) == _abi.ERR_UNSUPPORTED and '64 features' in msg()
    d = _descriptor()
    d.check_every = 0                  # there is no blind queue
    assert call(d) == _abi.ERR_INVALID and 'check_every' in msg()
    d = _descriptor()
    d.max_iter = 0
    assert call(d) == _abi.ERR_INVALID and 'max_iter' in msg()
    assert _abi.ABI_VERSION == 8 and lib.ctr_abi_version() == 8


def test_the_struct_is_the_header_s():
    """the ctypes struct against the header's field list, name by name"""
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), '..', 'include', 'ctrefine.h')).read()
    body = re.search(r'typedef struct ctr_refine_global \{(.*?)\} ctr_refine_global;', header, re.S).group(1)
    names = [re.search(r'(\w+)(\[[^\]]*\])?;', line).group(1) for line in body.splitlines() if ';' in line]
    assert names == [n for n, _ in _abi.RefineGlobal._fields_]      # (one declaration per line in the header)
    assert ctypes.sizeof(_abi.RefineGlobal) % 8 == 0


def _plan(max_locals, n_globals=1, clusters=0, problems=0, features=0):
    d = _descriptor(dict(size='global', background='global') if n_globals == 2 else None)
    d.max_locals, d.n_clusters, d.n_problems, d.n_features = max_locals, clusters, problems, features
    return _lib.refine_global_plan(d)


def test_plan():
    """scratch bytes and launches at L = 0, at the limit and one beyond"""
    align = lambda b: (b + 255) // 256 * 256
    for lm, g in ((0, 1), (13, 1), (46, 1), (45, 2)):
        nv = lm + g + 1
        tp = nv * (nv + 1) // 2
        row = (2 * tp + 5 * lm + (g + 1) * lm + 1) // 2 * 2
        plan = _plan(lm, g)
        assert plan == _lib.RefineGlobalPlan(0, 4, (nv + 15) // 16, row)      # no problem: nothing to launch
        c, p, n = 7, 2, 11
        plan = _plan(lm, g, c, p, n)
        want = 2 * align(8 * 1) + align(8 * c * row) + align(8 * c * 48) + align(8 * c * 56) + align(8 * p * 104) \
            + align(8 * 3 * n) + align(4 * c) + align(4 * (p + 1))
        assert plan.scratch_bytes == want and plan.launches_per_iteration == 4 and plan.row_doubles == row
    assert _plan(46).tiles == 3 and _plan(13).tiles == 1 and _plan(14).tiles == 1 and _plan(15).tiles == 2
    with pytest.raises(NotImplementedError) as e:
        _plan(47)
    assert '48 columns' in str(e.value)
    with pytest.raises(NotImplementedError):
        _plan(46, 2)
