"""The rule of the training stage (``ctr_train_device``, include/ctrefine.h) without a device: the
NumPy yardstick (``tests/_train.py``) against fixtures made by the reference's own global-mode
``refine_leastsq`` (``tests/golden/make_golden_train.py``), and the host side of
``clustertracking_amd/train.py``."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import _train
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib, train

CASES = _train.load_cases()
NAMES = sorted(CASES)


@pytest.fixture(scope='module')
def problems():
    return {name: _train.problem_of(CASES[name]) for name in NAMES}


def test_the_fixture_holds_the_cases_the_reference_kept():
    assert {'gauss2d_iso', 'ring2d', 'two_frames', 'close_pair', 'edge_clipped', 'on_bound', 'fail_rms'} <= set(NAMES)
    assert CASES['fail_rms']['fails'] == 1 and sum(int(CASES[n]['fails']) for n in NAMES) == 1
    assert all(CASES[n]['solution'] == 1 for n in ('gauss2d_iso', 'ring2d', 'two_frames', 'close_pair', 'edge_clipped',
                                                   'on_bound', 'fail_rms'))
    # every case the rule needs is there, with a pinned solution or as a start-only entry (objective, gradient,
    # packed start and bounds at the start): per-axis sizes, 3D, the disc's hole and clamp, inv_series
    assert {'gauss2d_aniso', 'gauss3d_aniso', 'disc2d', 'inv2_2d'} <= set(NAMES)
    assert CASES['gauss3d_aniso']['frames'].ndim == 4 and len(CASES['gauss3d_aniso']['start']) == 3
    assert len(CASES['gauss2d_aniso']['start']) == 2 and len(CASES['inv2_2d']['start']) == 4
    c = CASES['two_frames']
    assert c['frames'].shape[0] == 2 and c['frames'][0].max() != c['frames'][1].max()
    assert np.diff(CASES['close_pair']['feat_offset']).max() == 2
    c = CASES['on_bound']
    assert c['B_globals'][0] < c['high'][0] * (1 + 1e-12) and abs(c['B_globals'][0] - c['high'][0]) < 1e-2


@pytest.mark.parametrize('name', NAMES)
def test_objective_and_gradient_at_the_start(problems, name):
    case, prob = CASES[name], problems[name]
    x0 = case['start']
    np.testing.assert_allclose(prob.F(x0), float(case['F_start']), rtol=1e-12)
    if 'grad_start' in case:
        np.testing.assert_allclose(prob.grad(x0), case['grad_start'], rtol=1e-12, atol=1e-12 * np.abs(case['grad_start']).max())


@pytest.mark.parametrize('name', NAMES)
def test_gradient_equals_finite_differences(problems, name):
    prob, x0 = problems[name], CASES[name]['start'] * 1.05
    g = prob.grad(x0)
    for v in range(len(x0)):
        h = 1e-6 * max(1., abs(x0[v]))
        e = np.zeros_like(x0)
        e[v] = h
        fd = (prob.F(x0 + e) - prob.F(x0 - e)) / (2 * h)
        assert abs(fd - g[v]) <= 1e-6 * max(abs(g).max(), 1e-12), (name, v, fd, g[v])


@pytest.mark.parametrize('name', NAMES)
def test_solution_equals_the_converged_reference(problems, name):
    case, prob = CASES[name], problems[name]
    if not case['solution']:     # a start-only entry: the reference's two runs do not pin a solution
        return
    x = prob.solve(case['low'], case['high'])
    cost = prob.cost(x)
    if case['fails']:
        assert cost > case['call']['max_rms_dev']
        return
    np.testing.assert_allclose(x, case['B_globals'], rtol=10 * float(case['scatter_globals']))
    np.testing.assert_allclose(cost, float(case['B_cost']), rtol=10 * float(case['scatter_cost']))


@pytest.mark.parametrize('name', NAMES)
def test_start_and_bounds_equal_the_reference_packed_ones(name):
    case, call = CASES[name], CASES[name]['call']
    nd = case['frames'].ndim - 1
    dia = call['diameter'] if hasattr(call['diameter'], '__iter__') else (call['diameter'],) * nd
    ff = train.training_param_mode(call['fit_function'], nd, all(d == dia[0] for d in dia))
    bounds = {k: tuple(v) for k, v in call['bounds'].items()}
    assert train.training_bounds({k: v for k, v in bounds.items() if not k.endswith('_rel_diff')}, ff.size_columns) == bounds
    off = np.array([0, len(case['frame_index'])])
    start, low, high = train.pack_problems(ff, case['params'], case['feat_offset'], off, bounds,
                                           tuple(int(d) // 2 for d in dia))
    assert np.array_equal(start[0], case['start'])
    assert np.array_equal(low[0], case['low']) and np.array_equal(high[0], case['high'])


@pytest.mark.parametrize('fit,extra', [('gauss', []), ('ring', ['thickness']), ('disc', ['disc_size']),
                                       ('inv_series_2', ['signal_mult', 'param_a', 'param_b'])])
@pytest.mark.parametrize('ndim,iso', [(2, True), (2, False), (3, True), (3, False)])
def test_mode_table(fit, extra, ndim, iso):
    ff = train.training_param_mode(fit, ndim, iso)
    n_const = 2 + ndim
    assert ff.params == _train.param_names(fit, ndim, iso) and ff.params[len(ff.params) - len(extra):] == extra
    assert ff.modes == [_abi.MODE_CONST] * n_const + [_abi.MODE_GLOBAL] * (len(ff.params) - n_const)
    assert ff.modes == _train.default_modes(fit, ndim, iso)
    if extra:      # param_mode may move more parameters to 'const'
        ff = train.training_param_mode(fit, ndim, iso, {extra[0]: 'const'})
        assert ff.modes[ff.params.index(extra[0])] == _abi.MODE_CONST and _abi.MODE_GLOBAL in ff.modes


def test_size_rel_diff_is_added_where_none_is_given():
    assert train.training_bounds(None, ['size']) == {'size_rel_diff': (0.9, 9)}
    assert train.training_bounds({'size_y_rel_diff': (0.5, 1)}, ['size_y', 'size_x']) == \
        {'size_y_rel_diff': (0.5, 1), 'size_x_rel_diff': (0.9, 9)}
    given = {'thickness': (0.1, 0.9)}
    assert train.training_bounds(given, ['size'])['thickness'] == (0.1, 0.9) and 'size_rel_diff' not in given


def test_public_names():
    assert callable(ct.train_leastsq) and callable(ct.train_arrays)
    assert 'train_leastsq' in ct.__all__ and 'train_arrays' in ct.__all__


def _table():
    f = pd.DataFrame(dict(y=[20., 40.], x=[20., 40.], signal=100., size=3.))
    return f, np.zeros((64, 64), np.uint8)


@pytest.mark.parametrize('kw,word', [
    (dict(param_mode=dict(signal='var')), 'only constant and global'),
    (dict(param_mode=dict(size='cluster')), 'only constant and global'),
    (dict(param_mode=dict(y='var')), 'only constant and global'),
    (dict(param_mode=dict(signal='global')), 'global'),
    (dict(constraints=[dict(type='eq')]), 'constraints'),
    (dict(compute_error=True), 'compute_error'),
    (dict(noise_size=1.), 'noise_size'),
    (dict(threshold=1.), 'noise_size'),
    (dict(fit_function=dict(params=[], func=None)), 'dict'),
])
def test_unsupported_is_loud(kw, word):
    f, im = _table()
    kw = dict(dict(fit_function='gauss'), **kw)
    with pytest.raises(NotImplementedError) as e:
        ct.train_leastsq(f, im, 13, None, refine_com=False, **kw)
    assert word in str(e.value)


def _descriptor():
    ff = train.training_param_mode('gauss', 2, True)
    d = train.descriptor(ff, (32, 40), np.uint8, 1, (6, 6))
    d.n_problems = 0        # no pointer is followed
    return d


def test_descriptor_then_handle():
    """as tests/test_stage_calls.py::test_descriptor_then_handle expects of a stage"""
    lib = _lib.load()
    call = 'ctr_train_device'
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    assert lib.ctr_train_device(None, None, None) == _abi.ERR_INVALID
    assert msg().startswith(call + ': ') and msg() != call + ': null handle'
    assert lib.ctr_train_device(None, ctypes.byref(_descriptor()), None) == _abi.ERR_INVALID
    assert msg() == call + ': null handle'


def test_descriptor_modes():
    lib = _lib.load()
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    for mode in (_abi.MODE_VAR, _abi.MODE_CLUSTER):
        d = _descriptor()
        d.modes[1] = mode
        assert lib.ctr_train_device(None, ctypes.byref(d), None) == _abi.ERR_UNSUPPORTED
        assert 'only constant and global' in msg()
    d = _descriptor()
    d.modes[2] = _abi.MODE_GLOBAL      # a position
    assert lib.ctr_train_device(None, ctypes.byref(d), None) == _abi.ERR_UNSUPPORTED
    d = _descriptor()
    d.modes[4] = _abi.MODE_CONST       # nothing left to train
    assert lib.ctr_train_device(None, ctypes.byref(d), None) == _abi.ERR_INVALID
    d = _descriptor()
    d.max_features = _abi.TRAIN_MAX_FEATURES + 1
    assert lib.ctr_train_device(None, ctypes.byref(d), None) == _abi.ERR_UNSUPPORTED and '64 features' in msg()
    assert _abi.ABI_VERSION == 8 and lib.ctr_abi_version() == 8


def test_general_global_mode_stays_refused():
    f, im = _table()
    with pytest.raises(NotImplementedError) as e:
        ct.refine_leastsq(f, im, 13, param_mode=dict(size='global'))
    assert 'train_leastsq' in str(e.value)
