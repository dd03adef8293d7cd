"""The rule of ``ct.fit_error`` without a device: the NumPy restatement (tests/_fit_error.py) against
itself and against the reference's objective (tests/golden/fit_error/, made by
tests/golden/make_golden_fit_error.py), the argument refusals, the plan call, the header and
``distance_std``.

Bounds, each measured once on the cases of this file:
  * the analytic Hessian against central differences of the restatement's own analytic gradient, step
    ``STEP`` relative to max(1, |v|): the worst difference was 3.8e-8 of the largest entry (the
    difference's truncation and cancellation, not the formulas: the gradient itself agrees with
    differences of F to 3e-9); with a margin of ten, HESS_SELF;
  * F and the gradient against the reference: 1e-12, as test_train_rule.py (seen: 1.3e-15, 1.1e-14);
  * the Hessian and the std against the fixtures' Hessian from differences, which is the limiting side:
    5.4e-10 and 6.2e-10 where the reference's Jacobian was differenced (gauss, ring), 8.4e-7 and 4.2e-7
    where only its objective could be (disc, inv_series); with a margin of ten, HESS_REF and STD_REF.
"""
import ctypes
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _cases
import _fit_error as rule
import _residual
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib

fe = importlib.import_module('clustertracking_amd.fit_error')

STEP = 1e-5
HESS_SELF = 10 * 3.8e-8
HESS_REF = {'jacobian': 10 * 5.4e-10, 'objective': 10 * 8.4e-7}
STD_REF = {'jacobian': 10 * 6.2e-10, 'objective': 10 * 4.2e-7}
GEOMETRIES = [((32, 32), 9), ((32, 32), (7, 9)), ((12, 24, 24), 7), ((12, 24, 24), (5, 7, 7))]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fit_error', 'fit_error_cases.npz')


def golden_cases():
    z = np.load(GOLDEN)
    for name in json.loads(str(z['names'])):
        yield name, {key.split('/', 1)[1]: z[key] for key in z.files if key.startswith(name + '/')}


def cluster_of(case):
    call = json.loads(str(case['call']))
    frame, params = case['frame'], case['params']
    ndim = frame.ndim
    isotropic = _residual.model_of(call['fit_function'], ndim, call['diameter'])[3]
    modes = rule.modes_of(call['fit_function'], ndim, isotropic, call.get('param_mode'))
    return rule.Cluster(frame, params, params[:, 2:2 + ndim], call['diameter'], call['fit_function'], modes)


# ---- 1. the restatement against itself ------------------------------------------------------------------------
@pytest.mark.parametrize('shape,diameter', GEOMETRIES, ids=['2d-iso', '2d-aniso', '3d-iso', '3d-aniso'])
@pytest.mark.parametrize('fit,extra', rule.PROFILES, ids=[p[0] for p in rule.PROFILES])
def test_hessian_is_the_derivative_of_the_gradient(fit, extra, shape, diameter):
    worst = 0.
    for mode in rule.MODE_MIXES + rule.PROFILE_MIXES[fit]:
        rng = np.random.default_rng(5)
        ndim = len(shape)
        isotropic = _residual.model_of(fit, ndim, diameter)[3]
        true = rule.truth(rng, fit, extra, shape, diameter, 2)
        frame = rule.draw(rng, shape, fit, true)
        params = rule.fitted(rng, true, ndim)
        c = rule.Cluster(frame, params, params[:, 2:2 + ndim], diameter, fit, rule.modes_of(fit, ndim, isotropic, mode))
        v = c.vect()
        analytic = c.hessian(v)
        assert np.abs(analytic - analytic.T).max() <= 1e-15 * np.abs(analytic).max()
        numeric = np.zeros_like(analytic)
        for k in range(c.nv):
            e = np.zeros(c.nv)
            e[k] = STEP * max(1., abs(v[k]))
            numeric[:, k] = (c.gradient(v + e) - c.gradient(v - e)) / (2. * e[k])
        worst = max(worst, np.abs(analytic - numeric).max() / np.abs(analytic).max())
    print('%s %s: worst difference %.2e of the largest entry' % (fit, shape, worst))
    assert worst <= HESS_SELF


# ---- 2. and 3. the restatement against the reference; the fixtures are positive definite ---------------------------
@pytest.mark.parametrize('name,case', list(golden_cases()), ids=[n for n, _ in golden_cases()])
def test_restatement_against_the_reference(name, case):
    c = cluster_of(case)
    v = c.vect()
    np.testing.assert_array_equal(v, case['vect'])            # the layout of vect_from_params
    value, grad, _, _, _ = c.evaluate(v)
    assert abs(value - case['F']) <= 1e-12 * case['F']
    if 'grad' in case:
        assert np.abs(grad - case['grad']).max() <= 1e-12 * np.abs(case['grad']).max()
    status, std, cov = rule.cluster_result(c)
    assert status == rule.OK                                    # a condition of the fixture, not a tolerance
    source = str(case['hessian_from'])
    d_hess = np.abs(c.hessian(v) - case['hessian']).max() / np.abs(case['hessian']).max()
    ref_std = np.sqrt(2. * np.diag(np.linalg.inv(case['hessian'])))          # refine.py:400-406
    d_std = np.max(np.abs(std - ref_std) / ref_std)
    print('%s (%s differenced): Hessian %.2e of the largest entry, std %.2e' % (name, source, d_hess, d_std))
    assert d_hess <= HESS_REF[source] and d_std <= STD_REF[source]
    np.testing.assert_allclose(np.sqrt(np.diag(cov)), std, rtol=0, atol=0)


def test_the_fixtures_cover_what_the_issue_names():
    calls = {name: json.loads(str(case['call'])) for name, case in golden_cases()}
    fits = [c['fit_function'] for c in calls.values()]
    assert {'gauss', 'ring', 'disc', 'inv_series_2'} == set(fits) and len(calls) == 7
    assert calls['ring2d_pair_var']['param_mode'] == {'thickness': 'var'}
    assert calls['ring2d_pair_cluster']['param_mode'] == {'thickness': 'cluster'}
    assert calls['inv2_2d_pair']['param_mode']['signal_mult'] == 'const'
    corner = dict(golden_cases())['gauss2d_corner']
    assert cluster_of(corner).n_pix < 40 < cluster_of(dict(golden_cases())['gauss2d_pair']).n_pix      # clipped on two sides
    assert os.path.getsize(GOLDEN) < 2 ** 20


def test_dimer_of_the_end_to_end_test_has_a_bond_better_than_its_positions():
    frame, true, diameter = rule.ring_dimer()
    c = rule.Cluster(frame, true, true[:, 2:4], diameter, 'ring', rule.modes_of('ring', 2, True, None))
    status, std, cov = rule.cluster_result(c)
    assert status == rule.OK
    where = [c.variable(0, 2), c.variable(0, 3), c.variable(1, 2), c.variable(1, 3)]
    bond = rule.distance_std_np(cov[np.ix_(where, where)], true[0, 2:4] - true[1, 2:4])
    assert 0 < bond < 0.8 * np.sqrt(np.sum(std[where] ** 2))
    # ... and not only because the distance reads one direction: the errors along the bond are correlated
    assert cov[where[1], where[3]] != 0 and bond < np.sqrt(std[where[1]] ** 2 + std[where[3]] ** 2)


def test_statuses_of_the_restatement():
    rng = np.random.default_rng(3)
    frames, params, offs, cluster, diameter, _ = rule.table(rng, 'gauss', [], 2, True)
    out = rule.fit_error_np(frames, params, offs, cluster, diameter)
    assert (out.status == rule.OK).sum() >= len(params) - 2 and out.cov_offset[-1] == len(out.cov)
    assert out.n_vars[0] == {1: 4, 2: 7, 3: 10, 4: 13}[int((cluster[:offs[1]] == cluster[0]).sum())]
    ok = out.status == rule.OK
    assert np.isnan(out.params_std[:, 4]).all() and (out.params_std[ok][:, :4] > 0).all()
    bad = params.copy()
    bad[0, 1] = np.nan
    assert rule.fit_error_np(frames, bad, offs, cluster, diameter).status[0] == rule.NONFINITE


# ---- 4. refusals, the plan, the header, distance_std -----------------------------------------------------------
def test_arguments_are_refused_before_any_device_work():
    frames = np.zeros((2, 32, 32), dtype=np.uint8)
    params = np.tile([1., 50., 10., 10., 2.], (3, 1))
    offs, cluster = [0, 2, 3], [0, 0, 0]
    call = lambda **k: ct.fit_error_arrays(**dict(dict(frames=frames, params=params, frame_offset=offs, cluster=cluster, diameter=9), **k))
    with pytest.raises(NotImplementedError, match="param_mode 'global' couples all features"):
        call(param_mode=dict(size='global'))
    with pytest.raises(NotImplementedError, match='custom \\(dict\\) fit functions'):
        call(fit_function=dict(name='mine'))
    with pytest.raises(ValueError, match='Unknown fit function'):
        call(fit_function='lorentz')
    with pytest.raises(ValueError, match='params must be \\[N, 5\\]'):
        call(params=params[:, :4])
    with pytest.raises(ValueError, match='params must be \\[N, 6\\]'):
        call(fit_function='ring')
    with pytest.raises(ValueError, match='frame_offset must not decrease'):
        call(frame_offset=[0, 4, 3])
    with pytest.raises(ValueError, match='one entry per frame and one more'):
        call(frame_offset=[0, 3])
    with pytest.raises(ValueError, match='cluster must be one-dimensional with 3 entries'):
        call(cluster=[0, 0])
    with pytest.raises(ValueError, match='cluster must hold integers'):
        call(cluster=[0., 0., 1.])
    with pytest.raises(ValueError, match='mask_pos must be \\[3, 2\\]'):
        call(mask_pos=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='residual_factor must be a finite positive number'):
        call(residual_factor=0.)
    with pytest.raises(ValueError, match='n_clusters'):
        call(n_clusters=4)
    with pytest.raises(ValueError, match='diameter must hold integers >= 2'):
        call(diameter=1)
    with pytest.raises(NotImplementedError, match="param_mode 'global'"):
        fe.descriptor((32, 32), np.uint8, 1, 1, 1, 9, param_mode=dict(size='global'))


def test_the_plan_answers_without_a_device():
    up = lambda b: (b + 255) // 256 * 256
    p = _lib.fit_error_plan(fe.descriptor((32, 32), np.uint8, 3, 40, 17, 9, 'ring', dict(thickness='var')))
    assert p.max_vars == (16, 48, _abi.MAX_VARS) and p.chunk == (256, 32, 8) and p.grid == 17
    tri = lambda n: n * (n + 1) // 2
    assert p.lds_bytes == tuple(8 * (tri(v) + 64 * 14 + c * (v | 1) + 12) for v, c in zip(p.max_vars, p.chunk))
    assert p.lds_bytes[2] + 1024 <= 160 * 1024 // 2            # two workgroups of the largest class share a CU, the static LDS included
    assert p.scratch_bytes == up(4) + 2 * up(8 * 3)
    empty = _lib.fit_error_plan(fe.descriptor((12, 24, 24), np.float64, 0, 0, 0, (5, 7, 7), 'inv_series_2'))
    assert empty.grid == 0 and empty.scratch_bytes == 0
    big = _lib.fit_error_plan(fe.descriptor((32, 32), np.uint16, 10, 2 ** 20, 2 ** 19, 9))
    assert big.grid == 65536                                    # capped: the kernel strides
    d = fe.descriptor((32, 32), np.uint8, 1, 1, 1, 9)
    d.modes[1] = _abi.MODE_GLOBAL
    with pytest.raises(NotImplementedError, match="ctr_fit_error_plan: param_mode 'global'"):
        _lib.fit_error_plan(d)
    d.modes[1], d.modes[0] = _abi.MODE_VAR, _abi.MODE_VAR
    with pytest.raises(ValueError, match='ctr_fit_error_plan: the background'):
        _lib.fit_error_plan(d)
    d = fe.descriptor((32, 32), np.uint8, 1, 1, 1, 9)
    d.ndim = 4
    with pytest.raises(ValueError, match='ctr_fit_error_plan: ndim'):
        _lib.fit_error_plan(d)
    lib = _lib.load()
    assert lib.ctr_fit_error_device(None, None, None) == _abi.ERR_INVALID
    assert (lib.ctr_last_error(None) or b'').decode() == 'ctr_fit_error_device: null descriptor'
    assert lib.ctr_fit_error_device(None, ctypes.byref(fe.descriptor((32, 32), np.uint8, 0, 0, 0, 9)), None) == _abi.ERR_INVALID
    assert (lib.ctr_last_error(None) or b'').decode() == 'ctr_fit_error_device: null handle'


def test_header_signature_constants_and_docs():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8     # an addition, not a new ABI
    words = lambda text: ' '.join(text.replace(' * ', ' ').replace('\n *', '\n').split())
    rule_text = words(fe.__doc__.split('  Clusters.  ', 1)[1].split('There is no CPU fallback', 1)[0])
    assert rule_text in words(header)                           # the rule, in the same words
    for clause in ('Clusters.', 'Variables.', 'Pixels.', 'Residual and Hessian.', 'Result.', 'Statuses', 'Order of the sums.'):
        assert clause in fe.__doc__ and clause in header, clause
    assert 'come from the stage after the fit, ctr_fit_error_device' in header       # the sentence at ctr_batch.params_std
    assert 'the masks sit on the fitted positions' in fe.__doc__ and 'TOO_LARGE' in fe.__doc__
    bare = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', bare))
    assert [p.strip() for p in protos['ctr_fit_error_device'].split(',')] == ['ctr_handle* h', 'const ctr_fit_error* e', 'void* hip_stream']
    assert len(protos['ctr_fit_error_plan'].split(',')) == 6 == len(_lib.SIGNATURES['ctr_fit_error_plan'][1])
    assert _lib.SIGNATURES['ctr_fit_error_device'] == _lib._stage(_abi.FitError) and callable(_lib.Engine.fit_error_device)
    body = re.search(r'typedef struct ctr_fit_error \{(.*?)\} ctr_fit_error;', bare, flags=re.S).group(1)
    assert re.findall(r'\b(\w+)(?:\[\w+\])?\s*;', body) == [f[0] for f in _abi.FitError._fields_]
    codes = re.search(r'enum \{ (CTR_FITERR_OK.*?) \};', bare, flags=re.S).group(1)
    assert [c.split('=')[0].strip() for c in codes.split(',')] == [
        'CTR_FITERR_OK', 'CTR_FITERR_NOT_POSITIVE_DEFINITE', 'CTR_FITERR_NONFINITE', 'CTR_FITERR_EMPTY', 'CTR_FITERR_TOO_LARGE',
        'CTR_FITERR_BAD_TABLE']
    assert (fe.OK, fe.NOT_POSITIVE_DEFINITE, fe.NONFINITE, fe.EMPTY, fe.TOO_LARGE, fe.BAD_TABLE) == tuple(range(6))
    assert (rule.OK, rule.NOT_POSITIVE_DEFINITE, rule.NONFINITE, rule.EMPTY, rule.TOO_LARGE) == tuple(range(5))
    assert {'fit_error_arrays', 'fit_error'} <= set(ct.__all__) and ct.fit_error is fe.fit_error
    assert ct.fit_error.distance_std is fe.distance_std and ct.fit_error_arrays is fe.fit_error_arrays


def test_struct_layout_matches_the_compiler(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_fit_error));\n'
    expect = [ctypes.sizeof(_abi.FitError)]
    for f, _ in _abi.FitError._fields_:
        src += 'printf("%%zu\\n", offsetof(ctr_fit_error, %s));\n' % f
        expect.append(getattr(_abi.FitError, f).offset)
    src += 'return 0;}\n'
    (tmp_path / 'layout.c').write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == expect


def test_distance_std_on_a_hand_made_covariance():
    # two rows of one cluster 5 px apart along x; the only variables are their x: var 3 of row 0, var 3 of row 1
    params = np.array([[0., 1., 10., 10., 2.], [0., 1., 10., 15., 2.]])
    a, b, c = 0.04, 0.09, -0.03
    res = fe.FitError(None, np.zeros(2, dtype=np.int32), None, None, np.array([a, c, c, b]), np.array([0, 4]),
                      np.array([0, 1]), np.array([3, 3], dtype=np.int32))
    assert ct.fit_error.distance_std(res, params, 0, 1) == pytest.approx(np.sqrt(a + b - 2 * c), rel=1e-15)
    assert ct.fit_error.distance_std(res, params, 1, 0) == pytest.approx(np.sqrt(a + b - 2 * c), rel=1e-15)
    assert ct.fit_error.distance_std(res, params, 0, 1, mpp=0.5) == pytest.approx(0.5 * np.sqrt(a + b - 2 * c), rel=1e-15)
    assert np.sqrt(a + b - 2 * c) > np.sqrt(a + b)              # (this hand-made pair is anti-correlated in x: the bond is worse)
    # the y of both rows is constant: along y the distance has no error of its own
    tilted = params.copy()
    tilted[1, 2] = 13.
    want = np.sqrt(a + b - 2 * c) * 5. / np.hypot(3., 5.)
    assert ct.fit_error.distance_std(res, tilted, 0, 1) == pytest.approx(want, rel=1e-15)
    # a failed cluster, rows of different clusters, no covariance
    failed = res._replace(status=np.array([1, 1], dtype=np.int32))
    assert np.isnan(ct.fit_error.distance_std(failed, params, 0, 1))
    apart = res._replace(cov=np.array([a, b]), cov_offset=np.array([0, 1, 2]))
    assert np.isnan(ct.fit_error.distance_std(apart, params, 0, 1))
    with pytest.raises(ValueError, match='want_cov=True'):
        ct.fit_error.distance_std(res._replace(cov=None), params, 0, 1)
