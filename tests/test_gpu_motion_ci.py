"""clustertracking_amd.motion_ci.diffusion_tensor_ci on the device against the NumPy restatement
(tests/_motion_ci.py) at the shapes where the kernels can go wrong: row counts around a wavefront and
a frame tile, gaps at tile seams and permutation boundaries (the order of the compaction), the switch
between LDS-resident and global rows, resample counts around a wavefront, a workgroup and the cap,
columns that are identically zero, the options, and the byte identities the fixed orders promise.

Tolerances (tests/_motion_ci.py: assert_matches): counts, ranks, NaN and infinity patterns exact; z0
1e-12 absolute; a 1e-9 relative; tensor and interval entry (i, j) within 2 (n + 8) 2^-53
sqrt(S_ii S_jj).  Exact ranks are only defined away from ties: assert_conditions checks, from the
restatement alone, that no (B - 1) avals lies within 1e-6 of a half-integer and no resampled statistic
within the value tolerance of ostat.  With two rows the acceleration is 0 by symmetry (d_0 = -d_1), a
relative tolerance has nothing to hold on to in rounding noise, so those rows are small integers and
halves: every operation is exact and both sides give 0, or 0 / 0, exactly.
"""
import numpy as np
import pytest

import _motion as M
import _motion_ci as C
from clustertracking_amd import _abi, _lib, motion, motion_ci

pytestmark = pytest.mark.gpu

TILE = M.TILE


def _track(rng, T, F, P):
    """random positions and bases (any finite 3 x 3 will do for the arithmetic)"""
    return rng.normal(0., 1., (T, F, 3)).cumsum(1), rng.normal(0., 1., (T, P, F, 3, 3))


def _exact_track(rng, T, F, P):
    """small integers: every row, product and mean of up to two rows is exact in float64"""
    return (rng.randint(-3, 4, (T, F, 3)).cumsum(1).astype(np.float64),
            rng.randint(-2, 3, (T, P, F, 3, 3)).astype(np.float64))


def _compare(positions, bases, lags, fps, ndim, pool=False, **kw):
    """one call of the device for all tracks and lags, every pair against the restatement"""
    B = kw.setdefault('n_samples', 200)
    interval, det = motion_ci.diffusion_tensor_ci(positions, bases, lags, fps, ndim, pool_tracks=pool, return_details=True, **kw)
    T, K, D = len(positions), len(C.alphas_of(kw.get('alpha', 0.05))), 3 * (ndim - 1)
    lead = (len(lags),) if pool else (T, len(lags))
    assert interval.shape == lead + (K, D, D) and det['ranks'].shape == lead + (K, D, D)
    assert det['tensor'].shape == det['z0'].shape == det['a'].shape == lead + (D, D) and det['counts'].shape == lead
    assert det['counts'].dtype == np.int64 and det['ranks'].dtype == np.int64
    results = {}
    for at in np.ndindex(*lead):
        lag = int(lags[at[-1]])
        x = C.pooled_rows(positions, bases, lag, ndim) if pool else C.rows(positions[at[0]], bases[at[0]], lag, ndim)
        res = C.ci(x, lag, fps, kw.get('alpha', 0.05), B, kw.get('method', 'bca'), kw.get('seed', 0))
        C.assert_conditions(res, B)
        C.assert_matches((interval[at], {k: v[at] for k, v in det.items()}), res, B, what=at)
        results[at] = res
    return interval, det, results


# ---- rows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ndim', [2, 3])
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_row_counts(n, ndim, engine):
    """one permutation, no gaps: n = F - lag rows exactly; a lag beyond the video and a track of NaN
    have none"""
    rng = np.random.RandomState(100 * n + ndim)
    positions, bases = (_exact_track if n <= 2 else _track)(rng, 2, n + 2, 1)
    bases[1] = np.nan
    _, det, res = _compare(positions, bases, [2, n + 2, n + 5], 4., ndim, seed=n)
    assert det['counts'].tolist() == [[n, 0, 0], [0, 0, 0]]
    assert res[0, 0]['counts'] == n


@pytest.mark.parametrize('ndim,P,F', [(3, 1, 2 * TILE + 5), (2, 2, 2 * TILE + 5), (3, 2, TILE + 3), (3, 12, TILE + 9)])
def test_compaction_order(ndim, P, F, engine):
    """gaps at the seams of the frame tiles and at the first and last frame of single permutations:
    the rows keep the order permutation, frame, or the resamples would pick other rows"""
    rng = np.random.RandomState(7 * F + P)
    lags = [1, 3] if P < 12 else [3]
    positions, bases = _track(rng, 2, F, P)
    for b in (TILE - 3, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE):
        if b < F:
            positions[0, b, b % 3] = np.nan                        # frames b - lag and b of every permutation
    for p in range(P):
        gone = [b for b in (0, F - 4, TILE - 1 - p, TILE + p)[p % 4:p % 4 + 2] if b < F]
        bases[0, p, gone, p % 3, (p + 1) % 3] = np.nan             # of this permutation alone
    bases[1, :, rng.rand(F) < 0.7] = np.nan                         # a sparse track
    _, det, _ = _compare(positions[:1] if P == 12 else positions, bases[:1] if P == 12 else bases, lags, 25., ndim, seed=F)
    assert (det['counts'] > 0).all()
    if P < 12:
        assert det['counts'][1, 0] < det['counts'][0, 0] // 2
    tensor, counts = motion.diffusion_tensor(positions[:1], bases[:1], lags, 25., ndim, return_counts=True)
    assert (counts == det['counts'][:1]).all()
    M.assert_tensors(det['tensor'][:1], tensor)                     # ostat is ctr_diffusion_device's tensor


# ---- the switch between rows in LDS and rows in global memory --------------------------------------------
def _plan(ndim, P, T, F, n_lags, B, pool=False):
    d = _abi.DiffusionCI()
    d.ndim, d.n_perm, d.n_tracks, d.n_frames, d.n_lags, d.fps = ndim, P, T, F, n_lags, 1.
    d.n_samples, d.method, d.n_alpha, d.pool_tracks = B, _abi.CI_BCA, 1, int(pool)
    d.alphas[0] = 0.5
    return _lib.diffusion_ci_plan(d)


def _switch(ndim, P):
    """the most frames whose rows are LDS-resident, read from the plan"""
    lo, hi = 1, 1 << 20
    assert _plan(ndim, P, 1, lo, 1, 100)[0] and not _plan(ndim, P, 1, hi, 1, 100)[0]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _plan(ndim, P, 1, mid, 1, 100)[0] else (lo, mid)
    return lo


@pytest.mark.parametrize('ndim,P,step', [(2, 1, -1), (2, 1, 0), (2, 1, 1), (3, 1, 0), (3, 1, 1), (2, 2, 0), (2, 2, 1)])
def test_lds_global_switch(ndim, P, step, engine):
    """n_max = P F at the switch - 1, at it and + 1 (one permutation), and dimers in 2D on either side"""
    F = _switch(ndim, P) + step
    assert F < 1500 * (3 - P) and _plan(ndim, P, 1, F, 1, 100)[0] == (step <= 0)
    assert _plan(ndim, P, 1, F, 1, 100)[1] == (8 * 3 * (ndim - 1) * P * F if step <= 0 else 0)
    rng = np.random.RandomState(F)
    positions, bases = _track(rng, 1, F, P)
    positions[0, rng.choice(F, 5, replace=False), 0] = np.nan
    _compare(positions, bases, [1], 50., ndim, n_samples=130, seed=F)


def test_few_rows_of_a_long_track_keep_its_path(engine):
    """n << n_max: the launch follows n_max (global rows), whatever n is; the same rows in a short
    track go through LDS and give the same bytes"""
    F = _switch(3, 2) + 40
    rng = np.random.RandomState(3)
    positions, bases = _track(rng, 1, F, 2)
    bases[0, :, 70:] = np.nan
    assert not _plan(3, 2, 1, F, 2, 100)[0] and _plan(3, 2, 1, 70, 2, 100)[0]
    long_i, long_d, _ = _compare(positions, bases, [1, 2], 10., 3, seed=5)
    assert long_d['counts'].tolist() == [[138, 136]]
    short_i, short_d = motion_ci.diffusion_tensor_ci(positions[:, :70], bases[:, :, :70], [1, 2], 10., 3, n_samples=200, seed=5,
                                                  return_details=True)
    assert short_i.tobytes() == long_i.tobytes()
    for k in long_d:
        assert short_d[k].tobytes() == long_d[k].tobytes(), k


# ---- resamples ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 2, 63, 64, 65, C.CI_THREADS - 1, C.CI_THREADS, C.CI_THREADS + 1, 1000, C.MAX_SAMPLES])
def test_resample_counts(B, engine):
    rng = np.random.RandomState(11)
    positions, bases = _track(rng, 1, 31, 2)
    _, det, _ = _compare(positions, bases, [1], 8., 3, n_samples=B, seed=B)
    assert det['counts'].tolist() == [[60]]
    if B == 1:      # the only resample lies below ostat in some entries, above it in others: z0 = +inf / -inf, rank 0
        assert np.isinf(det['z0']).all() and (det['z0'] > 0).any() and (det['z0'] < 0).any() and (det['ranks'] == 0).all()


def test_default_resamples(engine):
    """the reference's defaults: 10 000 resamples, BCa, alpha 0.05; about 500 rows"""
    rng = np.random.RandomState(12)
    positions, bases = _track(rng, 1, 251, 2)
    interval, det = motion_ci.diffusion_tensor_ci(positions[0], bases[0], 1, 30., return_details=True)
    assert interval.shape == (2, 6, 6) and det['counts'] == 500 and isinstance(det['counts'], int)
    res = C.ci(C.rows(positions[0], bases[0], 1, 3), 1, 30.)
    C.assert_conditions(res, 10000)
    C.assert_matches((interval, det), res, 10000)
    assert (interval[0] < det['tensor']).all() and (det['tensor'] < interval[1]).all()


def test_above_the_cap_raises_before_any_launch(engine):
    rng = np.random.RandomState(13)
    positions, bases = _track(rng, 1, 20, 2)
    with pytest.raises(ValueError):
        motion_ci.diffusion_tensor_ci(positions, bases, n_samples=C.MAX_SAMPLES + 1)
    d = _abi.DiffusionCI()                                          # the entry point itself, without pointers
    d.ndim, d.n_perm, d.n_tracks, d.n_frames, d.n_lags, d.fps = 3, 2, 1, 20, 1, 1.
    d.n_samples, d.method, d.n_alpha = C.MAX_SAMPLES + 1, _abi.CI_BCA, 1
    d.alphas[0] = 0.5
    with pytest.raises(NotImplementedError):
        engine.diffusion_ci_device(d)


# ---- identically zero columns -----------------------------------------------------------------------------
def test_zero_columns(engine):
    """2D trimers evaluated with ndim 3: z translation and x, y rotation are exactly 0; their entries
    have nothing below ostat (z0 = -inf), a = 0 / 0, rank 0 and the interval 0"""
    rng = np.random.RandomState(14)
    pos = rng.uniform(20., 60., (2, 50, 1, 2)) + rng.uniform(-4., 4., (2, 50, 3, 2))
    pos[1, 7] = np.nan
    com, bases = M.orientation(pos, 3, 2, 0.4)
    interval, det, _ = _compare(com, bases, [1, 4], 15., 3, seed=2)
    zero = np.zeros((6, 6), dtype=bool)
    zero[[2, 3, 4]] = zero[:, [2, 3, 4]] = True
    assert (det['z0'][..., zero] == -np.inf).all() and np.isnan(det['a'][..., zero]).all()
    assert (det['ranks'][..., zero] == 0).all() and (interval[..., zero] == 0).all() and (det['tensor'][..., zero] == 0).all()
    assert np.isfinite(det['z0'][..., ~zero]).all() and np.isfinite(det['a'][..., ~zero]).all()


# ---- options ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(method='pi'), dict(alpha=[0.1, 0.5, 0.9]), dict(alpha=[0.3, 0.2, 0.6], method='pi'),
                                dict(alpha=1e-4), dict(alpha=0.999), dict(alpha=[0.5] * 8)],
                         ids=['pi', 'three', 'three-pi', 'near0', 'near1', 'eight'])
def test_options(kw, engine):
    rng = np.random.RandomState(15)
    positions, bases = _track(rng, 2, 45, 6)
    for ndim in (2, 3):
        interval, det, res = _compare(positions, bases, [2], 20., ndim, n_samples=401, seed=4, **kw)     # odd: alpha 0.5 is no tie
        if kw.get('method') == 'pi' and 'alpha' not in kw:
            assert (det['ranks'][:, :, 0] == 10).all() and (det['ranks'][:, :, 1] == 390).all()      # 400 alpha
        if kw.get('alpha') == 1e-4:
            assert (det['ranks'][:, :, 0] == 0).all() and (det['ranks'][:, :, 1] == 400).all()       # the ends


# ---- the byte identities of the fixed orders -----------------------------------------------------------------
def _same(a, b, what):
    assert a[0].tobytes() == b[0].tobytes(), what
    for k in a[1]:
        assert np.asarray(a[1][k]).tobytes() == np.asarray(b[1][k]).tobytes(), (what, k)


def test_byte_identity_alone_batch_sweep_chunks(engine):
    rng = np.random.RandomState(16)
    positions, bases = _track(rng, 3, 20, 2)
    bases[1, 0, 5] = np.nan
    lags = [1, 2, 5, 19, 25]
    kw = dict(fps=30., ndim=3, n_samples=C.MAX_SAMPLES, seed=77, return_details=True)
    first = motion_ci.diffusion_tensor_ci(positions, bases, lags, **kw)
    _same(first, motion_ci.diffusion_tensor_ci(positions, bases, lags, **kw), 'the same call twice')
    other = motion_ci.diffusion_tensor_ci(positions, bases, lags, **dict(kw, seed=78))
    assert other[1]['tensor'].tobytes() == first[1]['tensor'].tobytes()
    assert (other[0][:, :3] != first[0][:, :3]).any() and np.isnan(other[0][:, 4]).all()
    for t in range(3):
        for i, k in enumerate(lags):
            alone = motion_ci.diffusion_tensor_ci(positions[t], bases[t], k, **kw)          # [F, 3], [P, F, 3, 3], a scalar lag
            _same(alone, (first[0][t, i], {n: v[t, i] for n, v in first[1].items()}), (t, k))
        batch = motion_ci.diffusion_tensor_ci(positions[t:t + 1], bases[t:t + 1], lags, **kw)
        _same(batch, (first[0][t:t + 1], {n: v[t:t + 1] for n, v in first[1].items()}), t)
    # a sweep so long that it is cut into chunks: sized from the plan
    chunk = _plan(3, 2, 1, 20, 10 ** 6, C.MAX_SAMPLES)[3]
    assert 50 < chunk < 200
    sweep = [lags[i % 5] for i in range(2 * chunk + 3)]
    assert _plan(3, 2, 1, 20, len(sweep), C.MAX_SAMPLES)[3] == chunk < len(sweep)
    long = motion_ci.diffusion_tensor_ci(positions[2], bases[2], sweep, **kw)
    for i in range(len(sweep)):
        _same((long[0][i], {n: v[i] for n, v in long[1].items()}),
              (first[0][2, i % 5], {n: v[2, i % 5] for n, v in first[1].items()}), i)


# ---- pooled tracks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('ndim', [2, 3])
def test_pool_tracks(ndim, engine):
    """the rows of all tracks in track order, each with its own missing frames"""
    rng = np.random.RandomState(17)
    positions, bases = _track(rng, 3, 40, 6)
    positions[0, [3, 17]] = np.nan
    bases[1, 2, 10:30] = np.nan
    bases[2, :, ::2] = np.nan
    interval, det, res = _compare(positions, bases, [1, 2, 40], 12., ndim, pool=True, n_samples=300, seed=6)
    per_track = motion.diffusion_tensor(positions, bases, [1, 2, 40], 12., ndim, return_counts=True)[1]
    assert (det['counts'] == per_track.sum(0)).all() and det['counts'][2] == 0 and det['counts'][0] > 200
    one = motion_ci.diffusion_tensor_ci(positions, bases, 2, 12., ndim, pool_tracks=True, n_samples=300, seed=6)
    assert one.shape == interval.shape[1:] and one.tobytes() == interval[1].tobytes()


# ---- tensors -----------------------------------------------------------------------------------------------
def test_tensors_in_tensors_out(engine):
    import torch
    rng = np.random.RandomState(18)
    positions, bases = _track(rng, 2, 60, 2)
    kw = dict(fps=9., ndim=3, n_samples=300, seed=8, return_details=True)
    want = motion_ci.diffusion_tensor_ci(positions, bases, [1, 3], **kw)
    pos_d, bases_d = torch.from_numpy(positions).cuda(), torch.from_numpy(bases).cuda()
    got = motion_ci.diffusion_tensor_ci(pos_d, bases_d, [1, 3], **kw)
    assert got[0].is_cuda and got[0].dtype == torch.float64 and got[1]['ranks'].dtype == torch.int64
    assert all(v.is_cuda for v in got[1].values()) and got[1]['counts'].dtype == torch.int64
    _same((got[0].cpu().numpy(), {k: v.cpu().numpy() for k, v in got[1].items()}), want, 'tensors')
    assert pos_d.cpu().numpy().tobytes() == positions.tobytes() and bases_d.cpu().numpy().tobytes() == bases.tobytes()
    side = torch.cuda.Stream()                           # a stream of the caller's
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = motion_ci.diffusion_tensor_ci(pos_d, bases_d, [1, 3], **kw)
    side.synchronize()
    _same((on_side[0].cpu().numpy(), {k: v.cpu().numpy() for k, v in on_side[1].items()}), want, 'side stream')
    with pytest.raises(ValueError):
        motion_ci.diffusion_tensor_ci(pos_d.float(), bases_d)
