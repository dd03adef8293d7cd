"""clustertracking_amd.motion on the device: against the reference's fixtures
(tests/golden/motion/motion_cases.npz) and against the NumPy restatement (tests/_motion.py) at the shapes
where the kernels can go wrong -- the frame tile of the diffusion kernel and its edges, lags at and
beyond the tile and the video, the lag that reads the later frame from global memory, gaps at the
tile's seam -- and the byte identities the fixed reduction order promises.

Tolerances as in tests/test_motion_rule.py: com and bases atol 1e-12, a tensor within 1e-10 of its
largest entry, n_samples exact.
"""
import numpy as np
import pytest

import _motion as M
from clustertracking_amd import motion

pytestmark = pytest.mark.gpu

CASES = M.load_cases()
IDS = [c['name'] for c in CASES]
TILE = M.TILE


# ---- the reference's fixtures --------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_fixture_orientation(case, engine):
    com, bases = motion.orientation_df(M.table_frame(case), case['cluster_size'], case['mpp'], None, case['sizes'],
                                       case['angles'])
    M.assert_same(com, case['com'], 1e-12, 'com')          # the reference's shapes: (length, 3), (P, length, 3, 3)
    M.assert_same(bases, case['bases'], 1e-12, 'bases')


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_fixture_tensor(case, engine):
    for lag, want in zip(case['lags'], case['tensors']):
        got, n = motion.diffusion_tensor(case['com'], case['bases'], int(lag), case['fps'], case['ndim'], return_counts=True)
        assert got.shape == want.shape and isinstance(n, int)       # the reference's shape: (D, D)
        M.assert_tensors(got, want, 'lag %d' % lag)
    sweep = motion.diffusion_tensor(case['com'], case['bases'], case['lags'], case['fps'], case['ndim'])
    M.assert_tensors(sweep, case['tensors'], 'sweep')
    one = motion.diffusion_tensor(case['com'], case['bases'][0], 1, case['fps'], case['ndim'])      # [F, 3, 3]
    ref, _ = M.diffusion_tensor(case['com'][None], case['bases'][None, :1], [1], case['fps'], case['ndim'])
    M.assert_tensors(one, ref[0, 0], 'one permutation')


# ---- orientation against the restatement -----------------------------------------------------------
GEOMETRIES = [(2, 2), (2, 3), (3, 3), (3, 4), (3, 2)]


def _clusters(rng, T, F, cluster_size, ndim):
    """features a few pixels apart around a wandering centre; per track its own missing frames"""
    pos = rng.uniform(20., 60., (T, F, 1, ndim)) + rng.uniform(-4., 4., (T, F, cluster_size, ndim))
    for t in range(T):
        gone = rng.rand(F) < 0.1 * (t + 1)
        pos[t, gone] = np.nan
        if F > 2:
            pos[t, (5 * t + 1) % F, cluster_size - 1, 0] = np.nan     # one coordinate missing
    return pos


@pytest.mark.parametrize('T,F', [(1, 1), (1, 63), (3, 64), (3, 65), (1, 257), (3, 513)])
@pytest.mark.parametrize('ndim,cluster_size', GEOMETRIES)
def test_orientation_against_restatement(ndim, cluster_size, T, F, engine):
    rng = np.random.RandomState(1000 * F + 10 * ndim + cluster_size)
    pos = _clusters(rng, T, F, cluster_size, ndim)
    sizes = rng.uniform(0.8, 1.4, cluster_size)
    P = len(M.PERMUTATIONS[cluster_size])
    angles = rng.uniform(0., 2 * np.pi, (T, P, F)) if (ndim, cluster_size) == (3, 2) else None
    com, bases = motion.orientation_arrays(pos, cluster_size, ndim, 0.37, sizes, angles)
    want_com, want_bases = M.orientation(pos, cluster_size, ndim, 0.37, sizes, angles)
    assert com.shape == (T, F, 3) and bases.shape == (T, P, F, 3, 3)
    M.assert_same(com, want_com, 1e-12, 'com')
    M.assert_same(bases, want_bases, 1e-12, 'bases')
    com1, bases1 = motion.orientation_arrays(pos, cluster_size, ndim, 0.37, None, angles)       # equal weights
    want_com, want_bases = M.orientation(pos, cluster_size, ndim, 0.37, None, angles)
    M.assert_same(com1, want_com, 1e-12, 'com, sizes=None')
    M.assert_same(bases1, want_bases, 1e-12, 'bases, sizes=None')


def test_orientation_degenerate_geometry_is_nan(engine):
    """coincident features, a collinear 3D trimer, a 3D dimer along [1, 0, 0]: NaN bases, no error"""
    pos = np.array([[[[3., 4.], [3., 4.]], [[3., 4.], [5., 4.]]]])
    com, bases = motion.orientation_arrays(pos, 2, 2)
    assert np.isnan(bases[0, :, 0]).all() and np.isfinite(bases[0, :, 1]).all() and np.isfinite(com).all()
    pos = np.array([[[[0., 0., 0.], [0., 0., 1.], [0., 0., 2.]], [[0., 0., 0.], [0., 1., 1.], [0., 0., 2.]]]])
    com, bases = motion.orientation_arrays(pos, 3, 3)
    assert np.isnan(bases[0, :, 0]).all() and np.isfinite(bases[0, :, 1]).all() and np.isfinite(com).all()
    pos = np.array([[[[0., 0., 0.], [0., 0., 2.]], [[0., 0., 0.], [0., 1., 2.]]]])
    com, bases = motion.orientation_arrays(pos, 2, 3, angles=np.full((1, 2, 2), 0.3))
    assert np.isnan(bases[0, :, 0]).all() and np.isfinite(bases[0, :, 1]).all() and np.isfinite(com).all()
    com, bases = motion.orientation_arrays(np.zeros((0, 4, 2, 2)), 2, 2)
    assert com.shape == (0, 4, 3) and bases.shape == (0, 2, 4, 3, 3)


# ---- diffusion tensor against the restatement ------------------------------------------------------
FRAMES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
F_GLOBAL = TILE + M.MOT_HALO_MAX + 30         # the later frame of a long lag lies beyond the staged halo
LAG_GLOBAL = M.MOT_HALO_MAX + 82


def _lags_of(F):
    return sorted({k for k in (1, F - 1, F, TILE - 1, TILE, TILE + 1) if k >= 1})


def _track(rng, T, F, P, lags):
    """random positions and bases (any finite 3 x 3 will do for the arithmetic), per track its own
    gaps: NaN bases or positions at b = TILE - 1, TILE and TILE - lag, and scattered; the last of
    three tracks is NaN throughout"""
    positions = rng.normal(0., 1., (T, F, 3)).cumsum(1)
    bases = rng.normal(0., 1., (T, P, F, 3, 3))
    for t in range(T):
        seam = [TILE - 1, TILE] + [TILE - k for k in lags] + [2 * TILE - 1, 2 * TILE]
        for n, b in enumerate(b for b in seam if 0 <= b < F):
            if (n + t) % 3 == 0:
                positions[t, b, n % 3] = np.nan
            elif (n + t) % 3 == 1:
                bases[t, :, b, n % 3, (n + t) % 3] = np.nan
        if F > 8:
            scattered = rng.choice(F, max(1, F // 20), replace=False)
            bases[t, (t + 1) % P, scattered] = np.nan                   # one permutation only
    if T == 3:
        bases[2] = np.nan
    return positions, bases


def _check(positions, bases, lags, fps, ndim):
    tensor, counts = motion.diffusion_tensor(positions, bases, lags, fps, ndim, return_counts=True)
    want, want_n = M.diffusion_tensor(positions, bases, lags, fps, ndim)
    assert counts.dtype == np.int64 and (counts == want_n).all(), (counts, want_n)
    M.assert_tensors(tensor, want)
    return tensor, counts


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('F', FRAMES)
def test_tensor_against_restatement(F, T, engine):
    rng = np.random.RandomState(7 * F + T)
    lags = _lags_of(F)
    positions, bases = _track(rng, T, F, 2, lags)
    assert not any(M.mot_reads_global(F, k) for k in lags)
    for ndim in (2, 3):
        tensor, counts = _check(positions, bases, lags, 12.5, ndim)
        assert tensor.shape == (T, len(lags), 3 * (ndim - 1), 3 * (ndim - 1))
        for i, k in enumerate(lags):
            if k >= F:
                assert (counts[:, i] == 0).all() and np.isnan(tensor[:, i]).all()
        if T == 3:
            assert (counts[2] == 0).all() and np.isnan(tensor[2]).all()


def test_tensor_lag_from_global_memory(engine):
    """F beyond TILE + MOT_HALO_MAX: the rows of a long lag take their later frame from global
    memory, those of the short lags of the same call from LDS"""
    F = F_GLOBAL
    lags = [LAG_GLOBAL, 1, TILE, M.MOT_HALO_MAX, M.MOT_HALO_MAX + 1, F - 1]
    assert [M.mot_reads_global(F, k) for k in lags] == [True, False, False, False, True, True]
    rng = np.random.RandomState(5)
    positions, bases = _track(rng, 3, F, 6, lags)
    _check(positions, bases, lags, 30., 3)
    # the same rows through LDS alone: a video cut to TILE + MOT_HALO_MAX frames keeps lag 300's
    # rows of the first tile
    cut = TILE + M.MOT_HALO_MAX
    assert not M.mot_reads_global(cut, 300)
    _check(positions[:, :cut], bases[:, :, :cut], [300], 30., 3)


def test_tensor_unsorted_lags_with_a_duplicate(engine):
    rng = np.random.RandomState(9)
    lags = [7, 1, TILE, 7, 3, 400, 2]
    positions, bases = _track(rng, 3, 300, 12, lags)
    tensor, counts = _check(positions, bases, lags, 25., 3)
    assert tensor[:, 0].tobytes() == tensor[:, 3].tobytes() and (counts[:, 0] == counts[:, 3]).all()
    assert (counts[:, 5] == 0).all()


# ---- the byte identities of the fixed reduction order ----------------------------------------------
def test_bit_identity(engine):
    rng = np.random.RandomState(21)
    F, lags = F_GLOBAL, [1, 2, 5, TILE - 1, TILE + 1, LAG_GLOBAL, 40]
    positions, bases = _track(rng, 3, F, 6, lags)
    positions[2], bases[2] = positions[0][::-1], bases[1][:, ::-1]         # a third track with rows
    first, n_first = motion.diffusion_tensor(positions, bases, lags, 30., 3, return_counts=True)
    again, n_again = motion.diffusion_tensor(positions, bases, lags, 30., 3, return_counts=True)
    assert np.isfinite(first).all() and (n_first > 0).all()
    assert first.tobytes() == again.tobytes() and n_first.tobytes() == n_again.tobytes()        # two runs
    for i, k in enumerate(lags):                                           # lag k alone = lag k of the sweep
        alone, n_alone = motion.diffusion_tensor(positions, bases, [k], 30., 3, return_counts=True)
        assert alone[:, 0].tobytes() == first[:, i].tobytes() and (n_alone[:, 0] == n_first[:, i]).all(), k
    for t in range(3):                                                     # track t alone = track t of the batch
        alone = motion.diffusion_tensor(positions[t:t + 1], bases[t:t + 1], lags, 30., 3)
        assert alone[0].tobytes() == first[t].tobytes(), t
        single = motion.diffusion_tensor(positions[t], bases[t], lags, 30., 3)      # [F, 3], [P, F, 3, 3]
        assert single.tobytes() == first[t].tobytes(), t
    pos = _clusters(rng, 3, 300, 4, 3)
    a = motion.orientation_arrays(pos, 4, 3, 0.3, [1., 1.2, 0.9, 1.1])
    b = motion.orientation_arrays(pos, 4, 3, 0.3, [1., 1.2, 0.9, 1.1])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    alone = motion.orientation_arrays(pos[1:2], 4, 3, 0.3, [1., 1.2, 0.9, 1.1])
    assert alone[0].tobytes() == a[0][1:2].tobytes() and alone[1].tobytes() == a[1][1:2].tobytes()


# ---- the other paths ---------------------------------------------------------------------------------
def test_device_tensors_chain_without_host_copy(engine):
    import torch
    rng = np.random.RandomState(33)
    pos = _clusters(rng, 3, 2 * TILE + 1, 3, 3)
    sizes, lags = [1., 1.3, 0.8], [1, 4, TILE]
    com_h, bases_h = motion.orientation_arrays(pos, 3, 3, 0.25, sizes)
    want, want_n = motion.diffusion_tensor(com_h, bases_h, lags, 20., 3, return_counts=True)
    pos_d = torch.from_numpy(pos).cuda()
    com_d, bases_d = motion.orientation_arrays(pos_d, 3, 3, 0.25, sizes)
    assert com_d.is_cuda and bases_d.is_cuda and com_d.dtype == torch.float64
    got, got_n = motion.diffusion_tensor(com_d, bases_d, lags, 20., 3, return_counts=True)
    assert got.is_cuda and got_n.is_cuda and got_n.dtype == torch.int64
    assert com_d.cpu().numpy().tobytes() == com_h.tobytes() and bases_d.cpu().numpy().tobytes() == bases_h.tobytes()
    assert got.cpu().numpy().tobytes() == want.tobytes() and (got_n.cpu().numpy() == want_n).all()
    side = torch.cuda.Stream()                           # a stream of the caller's
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        com_s, bases_s = motion.orientation_arrays(pos_d, 3, 3, 0.25, sizes)
        got_s = motion.diffusion_tensor(com_s, bases_s, lags, 20., 3)
    side.synchronize()
    assert got_s.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        motion.orientation_arrays(pos_d.float(), 3, 3)


def test_pool_tracks_is_the_count_weighted_mean(engine):
    rng = np.random.RandomState(44)
    lags = [1, 3, 50, 400]
    positions, bases = _track(rng, 3, 300, 6, lags)
    for ndim in (2, 3):
        per, n = motion.diffusion_tensor(positions, bases, lags, 8., ndim, return_counts=True)
        pooled, n_pooled = motion.diffusion_tensor(positions, bases, lags, 8., ndim, pool_tracks=True, return_counts=True)
        assert (n_pooled == n.sum(0)).all() and pooled.shape == per.shape[1:]
        for i in range(len(lags)):
            if n[:, i].sum() == 0:
                assert np.isnan(pooled[i]).all()
                continue
            rows = n[:, i] > 0
            want = (per[rows, i] * n[rows, i, None, None]).sum(0) / n[rows, i].sum()
            assert np.abs(pooled[i] - want).max() <= 1e-12 * np.abs(want).max()
        # ... which is the tensor of the pooled rows
        x = [M.displacements(positions[t], bases[t], 3) for t in range(3)]
        x = np.concatenate(x)
        if ndim == 2:
            x = x[:, [0, 1, 5]]
        M.assert_tensors(pooled[1], (x[:, :, None] * x[:, None, :]).mean(0) * 0.5 / (3 / 8.))
    one = motion.diffusion_tensor(positions, bases, 3, 8., 3, pool_tracks=True)
    assert one.shape == (6, 6)
