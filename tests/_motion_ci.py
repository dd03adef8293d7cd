"""The rule of clustertracking_amd.motion_ci.diffusion_tensor_ci restated in NumPy, literally (the CPU
yardstick of tests/test_motion_ci_rule.py and tests/test_gpu_motion_ci.py, and of
tools/motion_ci_time.py), and the launch decision of ctr_diffusion_ci_device restated from the host
code that takes it.

The rule is scikits.bootstrap.ci (methods 'bca' and 'pi') applied as the reference's
motion.diffusion_tensor_ci applies it (motion.py:201-216), restated from the package's published
source: the jackknife deletes rows, Phi and its inverse are scipy.special.ndtr / ndtri, the ranks
np.round and np.nan_to_num.  The package's np.random indices are replaced by the counter-based
generator of include/ctrefine.h, here in Python integers.  Nothing here touches the engine.
"""
import warnings

import numpy as np
from scipy.special import ndtr, ndtri

import _motion as M

# ---- the launch decision of ctr_diffusion_ci_device (clustertracking_amd/csrc/tu_motion_ci.hip) ----
CI_THREADS = 512                       # motion_ci_kernels.h
MAX_SAMPLES, MAX_ALPHA = 16384, 8      # include/ctrefine.h: CTR_DIFFUSION_CI_*
LDS_BYTES, SCRATCH_BYTES = 65536, 268435456


def ci_plan(ndim, n_perm, n_tracks, n_frames, n_lags, n_samples, pool):
    """(rows_in_lds, lds_bytes, scratch_bytes, pairs_per_chunk), or the name of the error
    (tu_motion_ci.hip: ctr_diffusion_ci_launch).  It follows n_max, the bound on the rows of a
    pair that the host knows, never the rows that exist."""
    if n_samples < 1:
        return 'invalid'
    if n_samples > MAX_SAMPLES:
        return 'unsupported'
    D = 3 if ndim == 2 else 6
    NE = D * (D + 1) // 2
    n_max = n_perm * n_frames * (n_tracks if pool else 1)
    if n_max > 2 ** 31 - 1:
        return 'invalid'
    n_pairs = n_lags if pool else n_tracks * n_lags
    pair_bytes = 8 * (n_max * D + NE * n_samples + 1)
    in_lds = 8 * D * n_max <= LDS_BYTES
    fit = SCRATCH_BYTES // pair_bytes
    if n_pairs > 0 and fit == 0:
        return 'unsupported'
    chunk = min(n_pairs, fit)
    return in_lds, (8 * D * n_max if in_lds else 0), chunk * pair_bytes, chunk


# ---- the index generator -------------------------------------------------------------------------
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(z):
    """the finaliser of splitmix64 (device_common.h), in Python integers"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def bootstrap_index(seed, b, k, n):
    r = mix64((mix64(seed) + ((b << 32) + k + 1) * GOLDEN) & MASK64)
    return (r * n) >> 64


def bootstrap_indices_int(n_samples, n, seed):
    """[B, n] int64, every entry in Python integers"""
    return np.array([[bootstrap_index(seed, b, k, n) for k in range(n)] for b in range(n_samples)],
                    dtype=np.int64).reshape(n_samples, n)


def _indices(b_lo, b_hi, n, seed):
    u = np.uint64
    b = np.arange(b_lo, b_hi, dtype=np.uint64)[:, None]
    k = np.arange(n, dtype=np.uint64)[None, :]
    z = u(mix64(seed)) + ((b << u(32)) + k + u(1)) * u(GOLDEN)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    r = z ^ (z >> u(31))
    hi, lo = r >> u(32), r & u(0xFFFFFFFF)
    return ((hi * u(n) + ((lo * u(n)) >> u(32))) >> u(32)).astype(np.int64)


def bootstrap_indices(n_samples, n, seed):
    """the same in wrapping uint64 arithmetic (the 128-bit product in 32-bit halves), for the sizes
    at which the loop above takes minutes; tests/test_motion_ci_rule.py holds the two against each
    other"""
    return _indices(0, n_samples, n, seed)


# ---- rows and statistic --------------------------------------------------------------------------
def rows(positions, bases, lag, ndim):
    """positions [F, 3], bases [P, F, 3, 3]: x [n, D] of one track and lag"""
    x = M.displacements(np.asarray(positions, dtype=np.float64), np.asarray(bases, dtype=np.float64), int(lag))
    return x[:, [0, 1, 5]] if ndim == 2 else x


def pooled_rows(positions, bases, lag, ndim):
    """positions [T, F, 3], bases [T, P, F, 3, 3]: the rows of all tracks in track order"""
    return np.concatenate([rows(positions[t], bases[t], lag, ndim) for t in range(len(positions))])


def stat(x, lag, fps):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return (x[:, :, None] * x[:, None, :]).mean(0) * 0.5 * fps / lag


def resampled(x, lag, fps, n_samples, seed):
    """s [B, D, D]"""
    n, D = x.shape
    s = np.empty((n_samples, D, D))
    batch = max(1, (1 << 18) // n)
    for b0 in range(0, n_samples, batch):
        xr = x[_indices(b0, min(b0 + batch, n_samples), n, seed)]          # [batch, n, D]
        s[b0:b0 + batch] = (xr[:, :, :, None] * xr[:, :, None, :]).mean(1) * 0.5 * fps / lag
    return s


def jackknife_accel(x, lag, fps):
    """a of scikits.bootstrap.ci: the jackknife deletes one row at a time"""
    n = len(x)
    with np.errstate(invalid='ignore', divide='ignore'):
        jstat = np.array([stat(np.delete(x, k, 0), lag, fps) for k in range(n)])
        jmean = np.mean(jstat, axis=0)
        return np.sum((jmean - jstat) ** 3, axis=0) / (6.0 * np.sum((jmean - jstat) ** 2, axis=0) ** 1.5)


def closed_form_accel(x):
    """the same in p_k - mean(p), p_k the product of row k: jm - j_k is a positive multiple of it"""
    p = x[:, :, None] * x[:, None, :]
    d = p - p.mean(0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.sum(d ** 3, axis=0) / (6.0 * np.sum(d ** 2, axis=0) ** 1.5)


def alphas_of(alpha):
    return np.array([alpha / 2, 1 - alpha / 2]) if np.ndim(alpha) == 0 else np.asarray(alpha, dtype=np.float64)


def ci(x, lag, fps, alpha=0.05, n_samples=10000, method='bca', seed=0, accel=jackknife_accel):
    """dict(interval [K, D, D], tensor, counts, z0, a, ranks [K, D, D] int64; s and avals for the
    conditions of the tests) of the rows x [n, D]"""
    n, D = x.shape
    alphas = alphas_of(alpha)
    K = len(alphas)
    if n == 0:
        nan = np.full((D, D), np.nan)
        return dict(interval=np.full((K, D, D), np.nan), tensor=nan, counts=0, z0=nan, a=nan,
                    ranks=np.zeros((K, D, D), dtype=np.int64), s=np.zeros((0, D, D)), avals=np.full((K, D, D), np.nan))
    ostat = stat(x, lag, fps)
    s = resampled(x, lag, fps, n_samples, seed)
    s_sorted = np.sort(s, axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        z0 = ndtri(np.sum(s < ostat, axis=0) / n_samples)
        a = accel(x, lag, fps) if accel is jackknife_accel else accel(x)
        if method == 'pi':
            avals = alphas[:, None, None] * np.ones((D, D))
        else:
            zs = z0 + ndtri(alphas).reshape(K, 1, 1)
            avals = ndtr(z0 + zs / (1 - a * zs))
        ranks = np.nan_to_num(np.round((n_samples - 1) * avals)).astype(np.int64)
    i, j = np.meshgrid(np.arange(D), np.arange(D), indexing='ij')
    interval = s_sorted[ranks, i, j]
    return dict(interval=interval, tensor=ostat, counts=n, z0=z0, a=a, ranks=ranks, s=s, avals=avals)


# ---- tolerances and the conditions under which exact ranks are defined -----------------------------
def value_tol(res):
    """[D, D]: 2 (n + 8) 2^-53 sqrt(S_ii S_jj), S_ii the largest resampled value of the diagonal
    entry i -- the summation bound of two float64 means of x_i x_j (Cauchy-Schwarz)"""
    S = np.einsum('bii->bi', res['s']).max(0)
    return 2 * (res['counts'] + 8) * 2.0 ** -53 * np.sqrt(S[:, None] * S[None, :])


def assert_conditions(res, n_samples):
    """no (B - 1) avals within 1e-6 of a half-integer; no resampled statistic within the value
    tolerance of ostat, except in the columns that are exactly zero and -- with one or two rows --
    the resamples that hold every row once: their sum is one addition at most, equal bytes in any
    order."""
    if res['counts'] == 0:
        return
    v = (n_samples - 1) * res['avals']
    v = v[np.isfinite(v)]
    assert (np.abs(v - np.floor(v) - 0.5) > 1e-6).all(), 'a rank at a half-integer'
    s, ostat = res['s'], res['tensor']
    near = np.abs(s - ostat) <= value_tol(res)
    zero = (s == 0).all(0) & (ostat == 0)
    if res['counts'] <= 2:
        near &= s != ostat
    assert not near[:, ~zero].any(), 'a resampled statistic at ostat'


def assert_matches(got, res, n_samples, what=''):
    """got: (interval, details) of the device for one pair"""
    interval, det = got
    assert int(det['counts']) == res['counts'], (what, det['counts'], res['counts'])
    assert np.asarray(det['ranks']).dtype == np.int64 and (det['ranks'] == res['ranks']).all(), (what, det['ranks'], res['ranks'])
    z0, want = np.asarray(det['z0']), res['z0']
    assert (np.isnan(z0) == np.isnan(want)).all() and (np.isinf(z0) == np.isinf(want)).all(), (what, z0, want)
    assert (z0[np.isinf(want)] == want[np.isinf(want)]).all(), what
    fin = np.isfinite(want)
    assert (np.abs(z0[fin] - want[fin]) <= 1e-12).all(), (what, np.abs(z0[fin] - want[fin]).max())
    a, want = np.asarray(det['a']), res['a']
    assert (np.isnan(a) == np.isnan(want)).all() and np.isfinite(a[~np.isnan(want)]).all(), (what, a, want)
    fin = np.isfinite(want)
    assert (np.abs(a[fin] - want[fin]) <= 1e-9 * np.abs(want[fin])).all(), (what, a, want)
    if res['counts'] == 0:
        assert np.isnan(det['tensor']).all() and np.isnan(interval).all(), what
        return
    tol = value_tol(res)
    assert (np.abs(det['tensor'] - res['tensor']) <= tol).all(), (what, np.abs(det['tensor'] - res['tensor']) / tol)
    assert interval.shape == res['interval'].shape, what
    assert (np.abs(interval - res['interval']) <= tol).all(), (what, np.abs(interval - res['interval']) / tol)
