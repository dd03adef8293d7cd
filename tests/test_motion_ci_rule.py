"""clustertracking_amd.motion_ci.diffusion_tensor_ci without a GPU: the index generator, hand-computed
cases of the NumPy restatement (tests/_motion_ci.py), the closed form of the acceleration against the
literal jackknife, the launch decision of ctr_diffusion_ci_plan against its restatement around every
threshold, the layout of the descriptor, and the argument errors of the wrapper, which are raised
before a device is needed.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.special import ndtri

import _cases
import _motion_ci as C
from clustertracking_amd import _abi, _lib, motion, motion_ci


# ---- the index generator ---------------------------------------------------------------------------
def test_indices_equal_the_restatement_in_python_integers():
    for B, n, seed in [(5, 3, 7), (20, 17, 0), (3, 1000, 2 ** 64 - 1), (70, 65, 123456789), (1, 2 * 10 ** 6, 5)]:
        if n > 10 ** 6:
            got = motion_ci.bootstrap_indices(B, n, seed)[:, :50]
            want = np.array([[C.bootstrap_index(seed, b, k, n) for k in range(50)] for b in range(B)])
        else:
            got, want = motion_ci.bootstrap_indices(B, n, seed), C.bootstrap_indices_int(B, n, seed)
            assert (C.bootstrap_indices(B, n, seed) == want).all()          # the fast form of the test helpers
        assert got.dtype == np.int64 and got.shape == want.shape and (got == want).all(), (B, n, seed)
        assert got.min() >= 0 and got.max() < n


def test_indices_depend_on_seed_b_k_n_only():
    a = motion_ci.bootstrap_indices(40, 33, 9)
    assert (motion_ci.bootstrap_indices(7, 33, 9) == a[:7]).all()             # b and k, not the number of resamples
    assert (motion_ci.bootstrap_indices(40, 33, 9) == a).all()
    assert (motion_ci.bootstrap_indices(40, 33, 10) != a).any() and (motion_ci.bootstrap_indices(40, 34, 9)[:, :33] != a).any()
    assert (motion_ci.bootstrap_indices(12, 1, 3) == 0).all()
    assert motion_ci.bootstrap_indices(4, 0, 3).shape == (4, 0) and motion_ci.bootstrap_indices(0, 4, 3).shape == (0, 4)
    # every row is drawn about equally often
    counts = np.bincount(motion_ci.bootstrap_indices(2000, 50, 1).ravel(), minlength=50)
    assert np.abs(counts - 2000).max() < 6 * np.sqrt(2000)
    for bad in (-1, 2 ** 64, 1.5):
        with pytest.raises(ValueError):
            motion_ci.bootstrap_indices(3, 3, bad)


# ---- hand-computable cases of the restatement --------------------------------------------------------
def test_one_row():
    """n = 1: every resample is the row itself; nothing lies below ostat: z0 = -inf, a = 0 / 0, rank 0"""
    x = np.array([[1., 2., 3.]])
    res = C.ci(x, 2, 4., n_samples=9, seed=3)
    want = np.outer(x[0], x[0])                                   # 0.5 fps / lag = 1
    assert (res['tensor'] == want).all() and (res['s'] == want).all() and res['counts'] == 1
    assert (res['z0'] == -np.inf).all() and np.isnan(res['a']).all() and (res['ranks'] == 0).all()
    assert (res['interval'] == want).all()
    C.assert_conditions(res, 9)


def test_percentile_with_one_resample():
    rng = np.random.RandomState(2)
    x = rng.normal(size=(11, 6))
    res = C.ci(x, 3, 30., alpha=0.1, n_samples=1, method='pi', seed=5)
    idx = C.bootstrap_indices_int(1, 11, 5)[0]
    s0 = sum(np.outer(x[k], x[k]) for k in idx) / 11 * 0.5 * 30. / 3
    assert (res['ranks'] == 0).all() and np.abs(res['interval'] - s0).max() <= 1e-15 * np.abs(s0).max()
    assert res['interval'].shape == (2, 6, 6)


def test_three_rows_by_hand():
    """x = (1, 1, 0), (2, -1, 0), (3, 2, 0); B = 5, seed 7 draws (1,0,2) (0,2,1) (1,0,2) (0,1,1) (1,2,1).
    Entry (0, 0): p = 1, 4, 9: s = 14/3 14/3 14/3 3 17/3, ostat 14/3, one below.
    Entry (0, 1): p = 1, -2, 6: s = 5/3 5/3 5/3 -1 2/3, ostat 5/3, two below.
    Entry (1, 1): p = 1, 1, 4: s = 2 2 2 1 2, ostat 2, one below.  Column 2: all 0, none below.
    'pi' with alphas 0.1, 0.5, 0.9: 4 alpha = 0.4, 2, 3.6: ranks 0, 2, 4."""
    assert C.bootstrap_indices_int(5, 3, 7).tolist() == [[1, 0, 2], [0, 2, 1], [1, 0, 2], [0, 1, 1], [1, 2, 1]]
    x = np.array([[1., 1., 0.], [2., -1., 0.], [3., 2., 0.]])
    res = C.ci(x, 1, 2., alpha=[0.1, 0.5, 0.9], n_samples=5, method='pi', seed=7)
    third = 1 / 3.
    assert np.allclose(res['s'][:, 0, 0], [14 * third, 14 * third, 14 * third, 3, 17 * third], rtol=1e-15, atol=0)
    assert np.allclose(res['s'][:, 0, 1], [5 * third, 5 * third, 5 * third, -1, 2 * third], rtol=1e-15, atol=0)
    assert res['s'][:, 1, 1].tolist() == [2, 2, 2, 1, 2] and (res['s'][:, 2] == 0).all()
    assert (res['ranks'] == np.array([0, 2, 4])[:, None, None]).all()
    assert np.allclose(res['interval'][:, 0, 0], [3, 14 * third, 17 * third], rtol=1e-15)
    assert np.allclose(res['interval'][:, 0, 1], [-1, 5 * third, 5 * third], rtol=1e-15)
    assert res['interval'][:, 1, 1].tolist() == [1, 2, 2] and (res['interval'][:, :, 2] == 0).all()
    z0 = res['z0']
    assert z0[0, 0] == ndtri(0.2) and z0[0, 1] == ndtri(0.4) and z0[1, 1] == ndtri(0.2)
    assert (z0[2] == -np.inf).all() and (z0 == z0.T).all()
    assert np.isnan(res['a'][2]).all() and np.isfinite(res['a'][:2, :2]).all()
    # BCa: in the zero column z0 = -inf makes avals NaN and the ranks 0
    bca = C.ci(x, 1, 2., alpha=[0.1, 0.5, 0.9], n_samples=5, method='bca', seed=7)
    assert (bca['ranks'][:, 2] == 0).all() and np.isnan(bca['avals'][:, 2]).all() and (bca['interval'][:, 2] == 0).all()


def test_scalar_alpha_and_empty_rows():
    assert C.alphas_of(0.05).tolist() == [0.025, 0.975]
    res = C.ci(np.zeros((0, 3)), 1, 1., n_samples=10)
    assert res['counts'] == 0 and np.isnan(res['interval']).all() and res['interval'].shape == (2, 3, 3)
    assert (res['ranks'] == 0).all() and np.isnan(res['tensor']).all()


def test_closed_form_of_the_acceleration():
    """a in p_k - mean(p) against the jackknife that deletes rows (234 rows as in the issue, and few)"""
    rng = np.random.RandomState(0)
    for n, D in [(234, 6), (234, 3), (5, 6), (65, 6)]:
        x = rng.normal(size=(n, D)) * rng.uniform(0.1, 3., D)
        lit, closed = C.jackknife_accel(x, 2, 25.), C.closed_form_accel(x)
        assert np.isfinite(lit).all() and (np.abs(lit - closed) <= 1e-9 * np.abs(lit)).all(), (n, D)
        res = C.ci(x, 2, 25., n_samples=50, seed=1)
        fast = C.ci(x, 2, 25., n_samples=50, seed=1, accel=C.closed_form_accel)
        assert (res['ranks'] == fast['ranks']).all()
    # two rows: d_0 = -d_1, a = 0 where the rows differ and 0 / 0 where they do not -- exactly, in both
    # forms, for rows whose arithmetic is exact
    x = np.array([[1., 2., 0.5], [3., -1., 0.5]])
    for acc in (C.jackknife_accel(x, 2, 4.), C.closed_form_accel(x)):
        assert (acc[:2, :2] == 0).all() and (acc[:2, 2] == 0).all() and np.isnan(acc[2, 2])
    assert np.isnan(C.closed_form_accel(np.ones((1, 3)))).all() and np.isnan(C.jackknife_accel(np.ones((1, 3)), 1, 1.)).all()


# ---- the interface -----------------------------------------------------------------------------------
def test_declared_and_exported():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define CTR_ABI_VERSION 8\b', header) and _abi.ABI_VERSION == 8
    declared = set(re.findall(r'\b(ctr_[a-z_]+)\s*\(', header))
    lib = _lib.load()
    for name in ('ctr_diffusion_ci_device', 'ctr_diffusion_ci_plan'):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    for name, value in (('MAX_SAMPLES', C.MAX_SAMPLES), ('MAX_ALPHA', C.MAX_ALPHA), ('LDS_BYTES', C.LDS_BYTES),
                        ('SCRATCH_BYTES', C.SCRATCH_BYTES)):
        assert re.search(r'#define CTR_DIFFUSION_CI_%s %d\b' % (name, value), header), name
        assert getattr(_abi, 'DIFFUSION_CI_' + name) == value
    assert re.search(r'enum \{ CTR_CI_BCA = 0, CTR_CI_PI = 1 \};', header) and (_abi.CI_BCA, _abi.CI_PI) == (0, 1)
    kern = open(os.path.join(_cases.ROOT, 'clustertracking_amd', 'csrc', 'motion_ci_kernels.h')).read()
    assert re.search(r'constexpr int CI_THREADS = %d;' % C.CI_THREADS, kern)
    assert callable(motion_ci.diffusion_tensor_ci) and callable(motion_ci.bootstrap_indices)
    import clustertracking_amd as cta
    assert cta.motion_ci is motion_ci and cta.diffusion_tensor_ci is motion_ci.diffusion_tensor_ci
    assert {'motion_ci', 'diffusion_tensor_ci', 'bootstrap_indices'} <= set(cta.__all__)
    assert 'not taken over' not in motion.__doc__


def test_struct_layout_matches_header(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_diffusion_ci));\n'
    for f in _abi.DiffusionCI._fields_:
        src += 'printf("%%zu\\n", offsetof(ctr_diffusion_ci, %s));\n' % f[0]
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out == [ctypes.sizeof(_abi.DiffusionCI)] + [getattr(_abi.DiffusionCI, f[0]).offset for f in _abi.DiffusionCI._fields_]


def _desc(ndim, n_perm, n_tracks, n_frames, n_lags, n_samples, pool, method=_abi.CI_BCA, alphas=(0.025, 0.975)):
    d = _abi.DiffusionCI()
    d.ndim, d.n_perm, d.n_tracks, d.n_frames, d.n_lags, d.fps = ndim, n_perm, n_tracks, n_frames, n_lags, 1.
    d.n_samples, d.seed, d.method, d.n_alpha, d.pool_tracks = n_samples, 0, method, len(alphas), int(pool)
    for q, a in enumerate(alphas[:C.MAX_ALPHA]):
        d.alphas[q], d.z_alpha[q] = a, ndtri(a)
    return d


def _plan(*args):
    try:
        return _lib.diffusion_ci_plan(_desc(*args))
    except ValueError:
        return 'invalid'
    except NotImplementedError:
        return 'unsupported'


def test_plan_against_its_restatement():
    """around the LDS / global switch, the chunking and the cap of n_samples; no device, no pointers"""
    n = 0
    for ndim, D in ((2, 3), (3, 6)):
        for n_perm in (1, 2, 6, 12):
            switch = C.LDS_BYTES // (8 * D * n_perm)              # frames of the largest LDS-resident track
            for F in (0, 1, 40, switch - 1, switch, switch + 1, 1250, 10 ** 6):
                for B in (0, 1, 1000, C.MAX_SAMPLES, C.MAX_SAMPLES + 1):
                    for T, L, pool in ((1, 1, 0), (3, 7, 0), (3, 7, 1), (200, 100, 0), (200, 100, 1), (0, 5, 0), (4, 0, 1)):
                        want = C.ci_plan(ndim, n_perm, T, F, L, B, pool)
                        assert _plan(ndim, n_perm, T, F, L, B, pool) == want, (ndim, n_perm, T, F, L, B, pool)
                        n += 1
            assert C.ci_plan(ndim, n_perm, 1, switch, 1, 100, 0)[0] and not C.ci_plan(ndim, n_perm, 1, switch + 1, 1, 100, 0)[0]
    assert n > 2000
    # with ndim 2 dimers the switch is a track of 1365 frames
    assert C.ci_plan(2, 2, 1, 1365, 1, 100, 0)[:2] == (True, 65520) and C.ci_plan(2, 2, 1, 1366, 1, 100, 0)[:2] == (False, 0)
    # pooled tracks count towards n_max
    assert C.ci_plan(2, 2, 3, 455, 1, 100, 1)[0] and not C.ci_plan(2, 2, 3, 456, 1, 100, 1)[0]
    # the number of pairs at which a call is cut into chunks
    for ndim, n_perm, F, B in ((3, 2, 20, C.MAX_SAMPLES), (3, 12, 1250, 10000), (2, 2, 300, 1)):
        fit = C.ci_plan(ndim, n_perm, 1, F, 10 ** 9, B, 0)[3]
        assert fit < 10 ** 9
        for L in (fit - 1, fit, fit + 1):
            want = C.ci_plan(ndim, n_perm, 1, F, L, B, 0)
            assert want[3] == min(L, fit) and want[2] <= C.SCRATCH_BYTES
            assert _plan(ndim, n_perm, 1, F, L, B, 0) == want
    # 200 tracks x 100 lags of a 3D tetramer over 1250 frames at B = 10 000: chunks of about a hundred pairs
    chunk = C.ci_plan(3, 12, 200, 1250, 100, 10000, 0)[3]
    assert 50 < chunk < 200
    # one pair larger than the scratch
    assert C.ci_plan(3, 12, 2000, 1250, 1, 10000, 1) == 'unsupported' == _plan(3, 12, 2000, 1250, 1, 10000, 1)
    assert _plan(3, 4096, 2 ** 20, 2 ** 20, 1, 10, 1) == 'invalid'


def test_plan_checks_the_descriptor():
    for kw in (dict(method=2), dict(alphas=()), dict(alphas=(0.5,) * 9), dict(alphas=(1.5,)), dict(alphas=(float('nan'),))):
        with pytest.raises(ValueError):
            _lib.diffusion_ci_plan(_desc(3, 2, 1, 10, 1, 10, 0, **kw))
    for args in ((4, 2, 1, 10, 1, 10, 0), (3, 0, 1, 10, 1, 10, 0), (3, 2, -1, 10, 1, 10, 0)):
        with pytest.raises(ValueError):
            _lib.diffusion_ci_plan(_desc(*args))
    d = _desc(3, 2, 1, 10, 1, 10, 0)
    d.fps = 0.
    with pytest.raises(ValueError):
        _lib.diffusion_ci_plan(d)


# ---- argument errors of the wrapper: before any device work -------------------------------------------
def test_argument_errors(monkeypatch):
    def no_engine(device=0):
        raise AssertionError("the engine was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    pos, ori = np.zeros((10, 3)), np.zeros((2, 10, 3, 3))
    with pytest.raises(NotImplementedError):
        motion_ci.diffusion_tensor_ci(pos, ori, method='abc')
    for kw in (dict(multi=True), dict(output='errorbar'), dict(epsilon=0.001), dict(statfunction=np.mean)):
        with pytest.raises(NotImplementedError):
            motion_ci.diffusion_tensor_ci(pos, ori, **kw)
    with pytest.raises(TypeError):
        motion_ci.diffusion_tensor_ci(pos, ori, resamples=10)
    for alpha in (0., 1., -0.1, 1.5, float('nan'), [], [0.5] * 9, [0.5, 1.0], [0.0, 0.5]):
        with pytest.raises(ValueError):
            motion_ci.diffusion_tensor_ci(pos, ori, alpha=alpha)
    for B in (0, -5, 2.5, C.MAX_SAMPLES + 1):
        with pytest.raises(ValueError):
            motion_ci.diffusion_tensor_ci(pos, ori, n_samples=B)
    for kw in (dict(method='xyz'), dict(seed=-1), dict(seed=2 ** 64), dict(ndim=4), dict(lagtime=0), dict(fps=0.)):
        with pytest.raises(ValueError):
            motion_ci.diffusion_tensor_ci(pos, ori, **kw)
    with pytest.raises(ValueError):
        motion_ci.diffusion_tensor_ci(pos, np.zeros((2, 9, 3, 3)))
    with pytest.raises(ValueError):
        motion_ci.diffusion_tensor_ci(np.zeros((10, 2)), ori)
    # good arguments reach the engine
    with pytest.raises(AssertionError):
        motion_ci.diffusion_tensor_ci(pos, ori, alpha=[0.1, 0.5, 0.9], n_samples=C.MAX_SAMPLES, method='pi', seed=2 ** 64 - 1)
