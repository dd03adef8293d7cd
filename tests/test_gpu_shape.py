"""clustertracking_amd.shape on the device against the NumPy restatement (tests/_shape.py) at the shapes
where the kernels can go wrong: every geometry (the 2D tetramer included) around the workgroup of the
coordinates kernel; the frame tile of the dynamics kernel and its edges, lags at and around the staged
halo, the lag that reads the later frame from global memory, lags at and beyond the video, gaps at the
tile's seam; values exactly on a histogram edge, at the reach and at pi, the smallest and the largest
tables; and the byte identities the fixed reduction order promises.

Tolerances: bonds and rg are NumPy's doubles bit for bit; angles atol 1e-12 (tests/test_gpu_motion.py
gives com and bases the same: ample for a few ulp of atan2 at pi); counts exact; a mean or a moment
within 1e-10 of the largest magnitude of its (track, coordinate) row, the project's tensor tolerance;
min and max of bonds exact.
"""
import numpy as np
import pytest

import _shape as S
import clustertracking_amd as ct
from clustertracking_amd import shape

pytestmark = pytest.mark.gpu

TILE = S.TILE
GEOMETRIES = [(2, 2), (2, 3), (2, 4), (3, 2), (3, 3), (3, 4)]       # (ndim, cluster_size)


def _same_coords(got, want, n):
    """bonds and rg equal bit for bit with NaNs in the same cells, angles within 1e-12"""
    nb = n * (n - 1) // 2
    assert got.shape == want.shape and got.dtype == np.float64
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[..., :nb], want[..., :nb])
    np.testing.assert_array_equal(got[..., -1], want[..., -1])
    ang_g, ang_w = got[..., nb:-1], want[..., nb:-1]
    ok = np.isfinite(ang_w)
    if ok.any():
        assert np.abs(ang_g[ok] - ang_w[ok]).max() <= 1e-12


# ---- coordinates ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,F', [(1, 1), (1, 63), (3, 64), (3, 65), (1, 257), (3, 513)])
@pytest.mark.parametrize('ndim,n', GEOMETRIES)
def test_coordinates_against_restatement(ndim, n, T, F, engine):
    rng = np.random.RandomState(1000 * F + 10 * ndim + n)
    pos = S.clusters(rng, T, F, n, ndim)
    mpp = 0.37 if ndim == 2 else (0.5, 0.37, 0.37)
    res = shape.shape_arrays(pos, n, ndim, mpp)
    assert res.names == S.names(n) and res.coords.shape == (T, F, S.n_coords(n))
    want = S.coords(pos, n, ndim, mpp)
    assert np.isnan(want).any() or F == 1
    _same_coords(res.coords, want, n)
    one = shape.shape_arrays(pos, n, ndim)                   # mpp = 1
    _same_coords(one.coords, S.coords(pos, n, ndim), n)


def test_coordinates_degenerate_and_by_hand(engine):
    """the hand-computed clusters of tests/test_shape_rule.py, coincident and collinear features: the
    restatement's values, no error"""
    tri = np.array([[[[0., 0.], [3., 0.], [0., 4.]], [[0., 0.], [0., 1.], [0., 2.]], [[2.5, 2.5]] * 3,
                     [[1., 1.], [1., 1.], [-3., -3.]]]])
    got = shape.shape_arrays(tri, 3, 2).coords
    _same_coords(got, S.coords(tri, 3, 2), 3)
    assert got[0, 0, :3].tolist() == [3., 4., 5.] and abs(got[0, 0, 3] - np.pi / 2) <= 1e-15
    assert got[0, 1, 3:6].tolist() == [0., np.pi, 0.]       # collinear: 0, pi, 0
    assert (got[0, 2] == 0.).all() and got[0, 3, 3:6].tolist() == [0., 0., 0.]
    tet = np.array([[[[1., 1., 1.], [1., -1., -1.], [-1., 1., -1.], [-1., -1., 1.]], [[0.5, 0.5, 0.5]] * 4]])
    got = shape.shape_arrays(tet, 4, 3).coords
    _same_coords(got, S.coords(tet, 4, 3), 4)
    assert (got[0, 0, :6] == np.sqrt(8.)).all() and got[0, 0, 18] == np.sqrt(3.) and (got[0, 1] == 0.).all()
    square = np.array([[[[0., 0.], [0., 1.], [1., 1.], [1., 0.]]]])
    got = shape.shape_arrays(square, 4, 2).coords
    _same_coords(got, S.coords(square, 4, 2), 4)
    dimer = np.array([[[[0., 0., 0.], [1., 1., 1.]], [[np.inf, 0., 0.], [1., 1., 1.]]]])
    got = shape.shape_arrays(dimer, 2, 3, (2., 3., 6.)).coords
    assert got[0, 0].tolist() == [7., 3.5] and np.isnan(got[0, 1]).all()
    empty = shape.shape_arrays(np.zeros((0, 4, 2, 2)), 2, 2)
    assert empty.coords.shape == (0, 4, 2)


# ---- dynamics ------------------------------------------------------------------------------------------
def _seamed(rng, T, F, n, ndim, lags, dead_track=False):
    """clusters with, per track, gaps at the seams of the tiles: frames TILE - 1, TILE, TILE - lag, 2 TILE
    - 1, 2 TILE; with dead_track the last of three tracks is NaN throughout"""
    pos = S.clusters(rng, T, F, n, ndim)
    for t in range(T):
        seam = [TILE - 1, TILE] + [TILE - k for k in lags] + [2 * TILE - 1, 2 * TILE]
        for i, b in enumerate(b for b in seam if 0 <= b < F):
            if (i + t) % 2 == 0:
                pos[t, b] = np.nan
    if dead_track and T == 3:
        pos[2] = np.nan
    return pos


def _check_dynamics(pos, n, ndim, lags, mpp, fps):
    res = shape.shape_dynamics_arrays(pos, n, ndim, lags, mpp, fps)
    T, C, L = pos.shape[0], S.n_coords(n), len(lags)
    nb = n * (n - 1) // 2
    want = S.dynamics(S.coords(pos, n, ndim, mpp), lags, fps)
    assert res.names == S.names(n) and res.lags.tolist() == list(lags)
    assert res.n.dtype == np.int64 and res.n.shape == (T, C, L) and res.pooled_n.shape == (C, L)
    np.testing.assert_array_equal(res.n, want['n'])
    np.testing.assert_array_equal(res.pooled_n, want['pooled_n'])
    np.testing.assert_array_equal(res.n_frames, want['n_frames'])
    for name in ('mean_d', 'mean_d2', 'mean_d4', 'flex'):
        S.assert_rows(getattr(res, name), want[name], name)
        S.assert_rows(getattr(res, 'pooled_' + name)[None], want['pooled_' + name][None], 'pooled_' + name)
        assert np.isnan(getattr(res, name)[want['n'] == 0]).all()
    for name in ('mean', 'var', 'min', 'max'):
        S.assert_rows(getattr(res, name)[..., None], want[name][..., None], name)
    for name in ('min', 'max'):                             # bonds and rg are the restatement's doubles
        np.testing.assert_array_equal(getattr(res, name)[:, :nb], want[name][:, :nb])
        np.testing.assert_array_equal(getattr(res, name)[:, -1], want[name][:, -1])
    return res, want


@pytest.mark.parametrize('T', [1, 3])
@pytest.mark.parametrize('F', [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_dynamics_against_restatement(F, T, engine):
    n, ndim = 3, 2
    C = S.n_coords(n)
    halo = S.shp_halo(F, C)
    lags = sorted({k for k in (1, F - 1, F, TILE - 1, TILE, TILE + 1, halo - 1, halo, halo + 1) if k >= 1})
    assert not any(S.shp_reads_global(F, C, k) for k in lags)          # F <= TILE + halo: every later frame is staged
    rng = np.random.RandomState(7 * F + T)
    pos = _seamed(rng, T, F, n, ndim, lags, dead_track=True)
    res, want = _check_dynamics(pos, n, ndim, lags, 0.37, 12.5)
    for i, k in enumerate(lags):
        if k >= F:
            assert (res.n[:, :, i] == 0).all() and np.isnan(res.flex[:, :, i]).all() and np.isnan(res.pooled_mean_d2[:, i]).all()
    if T == 3:
        assert (res.n[2] == 0).all() and (res.n_frames[2] == 0).all() and np.isnan(res.var[2]).all()
    if F > 2:
        assert res.n.max() > 0


@pytest.mark.parametrize('ndim,n', [(2, 2), (3, 3), (2, 4), (3, 4)])
def test_dynamics_lag_from_global_memory(ndim, n, engine):
    """F beyond TILE + the largest halo of the geometry: the rows of a long lag take their later frame from
    global memory, those of the short lags of the same call from LDS; lags around the halo"""
    C = S.n_coords(n)
    top = S.shp_halo_max(C)
    F = TILE + top + 30
    assert S.shp_halo(F, C) == top
    lags = [top + 20, 1, top - 1, top, top + 1, TILE, F - 1, F]
    reads = [S.shp_reads_global(F, C, k) for k in lags]
    assert reads[:5] == [True, False, False, False, True] and reads[5] == (TILE > top) and reads[6:] == [True, False]
    rng = np.random.RandomState(5 + n)
    T = 3 if n < 4 else 2
    pos = _seamed(rng, T, F, n, ndim, lags)
    res, want = _check_dynamics(pos, n, ndim, lags, 0.25, 30.)
    assert (res.n[:, :, 0] > 0).all() and (res.n[:, :, -1] == 0).all()
    # the rows of lag top + 1 through LDS alone: a video cut to TILE + top frames keeps those of the first tile
    cut = TILE + top
    assert not S.shp_reads_global(cut, C, top + 1)
    _check_dynamics(pos[:, :cut], n, ndim, [top + 1], 0.25, 30.)


def test_dynamics_unsorted_lags_scalar_lag_and_empty(engine):
    rng = np.random.RandomState(9)
    lags = [7, 1, TILE, 7, 3, 400, 2]
    pos = _seamed(rng, 3, 300, 2, 3, lags)
    res, _ = _check_dynamics(pos, 2, 3, lags, (0.5, 0.2, 0.2), 25.)
    assert res.mean_d2[:, :, 0].tobytes() == res.mean_d2[:, :, 3].tobytes() and (res.n[:, :, 5] == 0).all()
    one = shape.shape_dynamics_arrays(pos, 2, 3, 3, (0.5, 0.2, 0.2), 25.)      # a scalar lag: a sweep of one
    assert one.n.shape == (3, 2, 1) and one.flex[:, :, 0].tobytes() == res.flex[:, :, 4].tobytes()
    none = shape.shape_dynamics_arrays(np.zeros((0, 10, 2, 2)), 2, 2, [1, 2])
    assert none.n.shape == (0, 2, 2) and (none.pooled_n == 0).all() and np.isnan(none.pooled_flex).all()
    flat = shape.shape_dynamics_arrays(np.zeros((2, 0, 3, 2)), 3, 2, [1])
    assert (flat.n == 0).all() and (flat.n_frames == 0).all() and np.isnan(flat.mean).all() and np.isnan(flat.mean_d).all()


def _bytes_equal(a, b, fields, what):
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (what, name)


PER_TRACK = ('n', 'mean_d', 'mean_d2', 'mean_d4', 'flex', 'n_frames', 'mean', 'var', 'min', 'max')
PER_LAG = ('n', 'mean_d', 'mean_d2', 'mean_d4', 'flex', 'pooled_n', 'pooled_mean_d', 'pooled_mean_d2', 'pooled_mean_d4',
           'pooled_flex')


def test_bit_identity(engine):
    """a (track, coordinate, lag) gives the same bytes on two calls, alone and inside a sweep of lags,
    alone and inside a batch of three tracks, and on a side stream"""
    import torch
    n, ndim = 3, 3
    C = S.n_coords(n)
    F = TILE + S.shp_halo_max(C) + 30
    lags = [1, 2, 5, TILE - 1, TILE + 1, S.shp_halo_max(C) + 20, 40]
    assert S.shp_reads_global(F, C, lags[5])
    rng = np.random.RandomState(21)
    pos = _seamed(rng, 3, F, n, ndim, lags)
    first = shape.shape_dynamics_arrays(pos, n, ndim, lags, 0.3, 30.)
    again = shape.shape_dynamics_arrays(pos, n, ndim, lags, 0.3, 30.)
    assert (first.n > 0).all() and np.isfinite(first.mean_d4).all()
    _bytes_equal(first, again, first._fields[2:], 'two calls')
    for i, k in enumerate(lags):                                           # lag k alone = lag k of the sweep
        alone = shape.shape_dynamics_arrays(pos, n, ndim, [k], 0.3, 30.)
        for name in PER_LAG:
            assert getattr(alone, name)[..., 0].tobytes() == getattr(first, name)[..., i].tobytes(), (k, name)
    for t in range(3):                                                     # track t alone = track t of the batch
        alone = shape.shape_dynamics_arrays(pos[t:t + 1], n, ndim, lags, 0.3, 30.)
        for name in PER_TRACK:
            assert getattr(alone, name)[0].tobytes() == getattr(first, name)[t].tobytes(), (t, name)
        for name in PER_LAG[:5]:                                           # pooled over one track: that track
            assert getattr(alone, 'pooled_' + name).tobytes() == getattr(alone, name)[0].tobytes(), (t, name)
    pos_d = torch.from_numpy(pos).cuda()
    side = torch.cuda.Stream()                                             # a stream of the caller's
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = shape.shape_dynamics_arrays(pos_d, n, ndim, lags, 0.3, 30.)
        coords_s = shape.shape_arrays(pos_d, n, ndim, 0.3).coords
    side.synchronize()
    for name in first._fields[2:]:
        assert getattr(got, name).cpu().numpy().tobytes() == getattr(first, name).tobytes(), name
    a, b = shape.shape_arrays(pos, n, ndim, 0.3).coords, shape.shape_arrays(pos[1:2], n, ndim, 0.3).coords
    assert coords_s.cpu().numpy().tobytes() == a.tobytes() and b.tobytes() == a[1:2].tobytes()


# ---- histogram -----------------------------------------------------------------------------------------
def _check_histogram(pos, q, n, ndim, mpp, bond_max, bond_dr, angle_bins, per_track):
    res = shape.shape_histogram_arrays(pos, n, ndim, bond_max, bond_dr, angle_bins, mpp, per_track)
    want = S.histogram(q, n, bond_max, bond_dr, angle_bins, per_track)
    names = S.names(n)
    nb = n * (n - 1) // 2
    assert res.names_bond == names[:nb] + ('rg',) and res.names_angle == names[nb:-1]
    for name in ('bond_edges', 'angle_edges', 'count_bond', 'above', 'count_angle', 'n'):
        got = getattr(res, name)
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, name
        np.testing.assert_array_equal(got, want[name], err_msg=name)
    assert (res.count_bond.sum(-1) + res.above == res.n[..., None]).all()              # the sum identity, on every row
    assert (res.count_angle.sum(-1) == res.n[..., None]).all()
    for name in ('density_bond', 'density_angle'):          # one product and one division, each rounded once
        np.testing.assert_allclose(getattr(res, name), want[name], rtol=1e-14, atol=0., equal_nan=True, err_msg=name)
    return res


def test_histogram_values_on_an_edge_at_the_reach_and_at_pi(engine):
    """3-4-5 triangles scaled by 1 / 4: the bonds 0.75 and 1.0 sit exactly on an edge of width 0.25 and fall
    in the upper bin, the bond 1.25 is exactly bond_max and counts in `above`; a collinear trimer has an
    angle of exactly pi, which the closed last bin takes; NaN frames are nowhere"""
    tri = np.array([[0., 0.], [3., 0.], [0., 4.]]) / 4.
    line = np.array([[0., 0.], [0., 0.75], [0., 1.5]])
    pos = np.stack([np.stack([tri] * 5 + [line] * 3 + [np.full((3, 2), np.nan)] * 2)] * 2)      # [2, 10, 3, 2]
    pos[1, :5] += 7.
    q = S.coords(pos, 3, 2)
    assert q[0, 0, :3].tolist() == [0.75, 1., 1.25] and q[0, 5, :6].tolist() == [0.75, 1.5, 0.75, 0., np.pi, 0.]
    assert S.min_angle_edge_distance(q, 3, 3) > 0.05
    res = _check_histogram(pos, q, 3, 2, 1., 1.25, 0.25, 3, False)
    assert res.n.tolist() == [16] and len(res.bond_edges) == 6 and res.bond_edges[3] == 0.75 and res.bond_edges[5] == 1.25
    assert res.count_bond[0].tolist() == [0, 0, 0, 16, 0] and res.above[0] == 0            # bond_01 = 0.75: bin 3, not 2
    assert res.count_bond[1].tolist() == [0, 0, 0, 0, 10] and res.above[1] == 6            # 1.0: bin 4; 1.5: above
    assert res.count_bond[2].tolist() == [0, 0, 0, 6, 0] and res.above[2] == 10            # 1.25 == bond_max: above
    assert res.count_angle[1].tolist() == [10, 0, 6] and res.count_angle[0].tolist() == [6, 10, 0]   # pi: the last bin
    per = _check_histogram(pos, q, 3, 2, 1., 1.25, 0.25, 3, True)
    assert per.n.tolist() == [8, 8] and (per.count_bond.sum(0) == res.count_bond).all()
    none = shape.shape_histogram_arrays(np.full((2, 3, 2, 2), np.nan), 2, 2, 1., 0.5, 4)
    assert none.n.tolist() == [0] and (none.count_bond == 0).all() and np.isnan(none.density_bond).all()
    assert none.count_angle.shape == (0, 4)


@pytest.mark.parametrize('name', sorted(S.HIST_CASES))
def test_histogram_against_restatement(name, engine):
    case = S.HIST_CASES[name]
    n, ndim = case['cluster_size'], case['ndim']
    pos, q, seed = S.clusters_off_edges(case['seed'], case['T'], case['F'], n, ndim, case['mpp'], case['angle_bins'])
    # the restatement's own distance to an edge first: a count cannot hide behind the angles' tolerance
    assert seed == case['seed'] and S.min_angle_edge_distance(q, n, case['angle_bins']) > 1e-9
    got = shape.shape_arrays(pos, n, ndim, case['mpp']).coords
    _same_coords(got, q, n)
    res = _check_histogram(pos, q, n, ndim, case['mpp'], case['bond_max'], case['bond_dr'], case['angle_bins'], case['per_track'])
    assert res.n.sum() > 0 and res.count_bond.shape[-1] == len(res.bond_edges) - 1


# ---- tensors and tables --------------------------------------------------------------------------------
def test_tensors_in_give_tensors_out_with_the_same_bytes(engine):
    import torch
    rng = np.random.RandomState(33)
    n, ndim, lags = 4, 2, [1, 4, TILE]
    pos = _seamed(rng, 3, 2 * TILE + 1, n, ndim, lags)
    pos_d = torch.from_numpy(pos).cuda()
    a, b = shape.shape_arrays(pos, n, ndim, 0.25), shape.shape_arrays(pos_d, n, ndim, 0.25)
    assert b.coords.is_cuda and b.coords.device == pos_d.device and b.coords.dtype == torch.float64 and b.names == a.names
    assert b.coords.cpu().numpy().tobytes() == a.coords.tobytes()
    a, b = shape.shape_dynamics_arrays(pos, n, ndim, lags, 0.25, 20.), shape.shape_dynamics_arrays(pos_d, n, ndim, lags, 0.25, 20.)
    for name in a._fields:
        if name != 'names':
            x = getattr(b, name)
            assert x.is_cuda and x.device == pos_d.device and x.cpu().numpy().tobytes() == getattr(a, name).tobytes(), name
    assert b.n.dtype == torch.int64 and b.n_frames.dtype == torch.int64 and b.lags.dtype == torch.int64
    a = shape.shape_histogram_arrays(pos, n, ndim, 3.75, 0.0625, 36, 0.25, True)
    b = shape.shape_histogram_arrays(pos_d, n, ndim, 3.75, 0.0625, 36, 0.25, True)
    for name in a._fields[2:]:
        x = getattr(b, name)
        assert x.is_cuda and x.device == pos_d.device and x.cpu().numpy().tobytes() == getattr(a, name).tobytes(), name
    assert b.count_bond.dtype == torch.int64 and b.count_bond.shape == (3, 7, 60) and b.count_angle.shape == (3, 12, 36)
    with pytest.raises(ValueError):
        shape.shape_arrays(pos_d.float(), n, ndim)


def _linked_table(rng, n, n_clusters, n_frames, first_frame):
    """a linked, labelled table of n_clusters clusters of n features over n_frames frames, a few features
    dropped; particle ids n * cluster + slot, cluster labels unique per frame"""
    import pandas as pd
    rows = []
    for fr in range(n_frames):
        for c in range(n_clusters):
            centre = np.array([40. + 30. * c, 50.]) + rng.normal(0., 1., 2)
            for s in range(n):
                if rng.rand() < 0.12 and 0 < fr < n_frames - 1:
                    continue                                # a dropped feature: the frame is incomplete
                y, x = centre + rng.uniform(-3., 3., 2)
                rows.append((fr + first_frame, n * c + s, 10 * fr + c, y, x))
    f = pd.DataFrame(rows, columns=['frame', 'particle', 'cluster', 'y', 'x'])
    return f.astype({'frame': np.int64, 'particle': np.int64, 'cluster': np.int64})


@pytest.mark.parametrize('n', [2, 3])
def test_shape_df_and_flexibility(n, engine):
    rng = np.random.RandomState(50 + n)
    f = _linked_table(rng, n, 3, 14, 5)
    block, track_ids, first = ct.track_positions(f, n)
    assert first == 5 and block.shape[0] == 3 and np.isnan(block).any()
    q = S.coords(block, n, 2, 0.4)
    df = shape.shape_df(f, n, mpp=0.4)
    whole = np.isfinite(block).all((2, 3))
    assert list(df.columns) == list(S.names(n)) and df.index.names == ['cluster_track', 'frame']
    assert len(df) == whole.sum() < whole.size and np.isfinite(df.values).all()
    for (t, fr), row in df.iterrows():
        _same_coords(row.values, q[t, fr - first], n)
    lags = [1, 2, 5]
    flex = shape.flexibility(f, n, lags, mpp=0.4, fps=8.)
    want = S.dynamics(q, lags, 8.)
    assert flex.index.names == ['cluster_track', 'lag'] and flex.columns.names == ['coordinate', 'stat']
    assert flex.shape == (3 * len(lags), len(S.names(n)) * 5)
    for stat in shape.STATS:
        got = np.stack([[flex.loc[(t, k), (c, stat)] for k in lags] for t in track_ids for c in S.names(n)])
        S.assert_rows(got.reshape(3, len(S.names(n)), len(lags)), want[stat].astype(np.float64), stat)
    assert ct.shape_df is shape.shape_df and ct.flexibility is shape.flexibility
