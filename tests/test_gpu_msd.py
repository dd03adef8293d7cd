"""Mean squared displacement on the device against the yardstick ``tests/_msd.py``.
The exact tables (steps that are multiples of 1/4, mpp a power of two: every sum is exact in any
order) must equal it bit for bit; they stand on every edge of the launch: a span around the LDS tile
``_abi.MSD_TILE`` with a gap across it, ids around the ensemble's chunk ``_abi.MSD_CHUNK``, track
lengths around the wavefront and the workgroup, lags around the video's length.  The rounded tables
stay within the derived bounds ``_msd.bound`` and ``_msd.bound_msd``."""
import numpy as np
import pandas as pd
import pytest

import _msd as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi

pytestmark = pytest.mark.gpu

TILE, CHUNK = _abi.MSD_TILE, _abi.MSD_CHUNK


def _spans():
    """four tracks with a span of TILE - 1, TILE, TILE + 1 and 2 TILE + 1 frames, each with a gap:
    across the workgroup's stride for the two that are dense in LDS; for the two that are read from
    the sorted rows up to the tile's edge (only the last frame lies beyond it) and across it; the
    longest also has a repeated id (so that row i + k is not the partner of row i behind it) and the
    table an unlinked row"""
    tracks = [yard.span_with_gap(0, TILE - 1, (254, 259)), yard.span_with_gap(1, TILE, (254, 259)),
              yard.span_with_gap(2, TILE + 1, (TILE - 4, TILE)), yard.span_with_gap(3, 2 * TILE + 1, (TILE - 2, TILE + 3))]
    return yard.exact_tracks(1, tracks, extra=[(150, 3), (151, -1), (TILE + 40, 3)])


def _lengths():
    """tracks of 1, 2, 63, 64, 65, 255, 256 and 257 rows without a gap, starting at different frames"""
    return yard.exact_tracks(2, [list(range(3 * p, 3 * p + rows)) for p, rows in enumerate((1, 2, 63, 64, 65, 255, 256, 257))])


def _small(ndim):
    """T = 6: a gap, a track of one row, an id without rows (3), a repeated id, negative ids"""
    tracks = [[0, 1, 4, 5], [2], [0, 1, 2, 3, 4], [], [1, 2, 3, 4, 5], [4, 5]]
    return yard.exact_tracks(3 + ndim, tracks, n_frames=6, ndim=ndim, extra=[(1, 2), (2, -1), (3, -5), (4, 0), (4, -1)])


def _chunks(n):
    return yard.exact_tracks(n, [[0, 1, 2]] * n)


# name: (table, mpp, lags)
EXACT = {
    'spans': (_spans, 0.5, (24,)),
    'lengths': (_lengths, (0.25, 2.), (70,)),
    'small_2d': (lambda: _small(2), 0.5, (1, 5, 9)),                # L = 1, T - 1 and T + 3
    'small_3d': (lambda: _small(3), (0.5, 1., 4.), (1, 5, 9)),
    'chunk_minus': (lambda: _chunks(CHUNK - 1), 2., (3,)),
    'chunk': (lambda: _chunks(CHUNK), 2., (3,)),
    'chunk_plus': (lambda: _chunks(CHUNK + 1), 2., (3,)),
    'two_chunks_plus': (lambda: _chunks(2 * CHUNK + 1), 2., (3,)),
    'no_rows': (lambda: (np.zeros((0, 2)), np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64)), 1., (2,)),
    'no_frames': (lambda: (np.zeros((0, 3)), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64)), 1., (2,)),
}
ROUNDED = {
    'jitter_2d': (lambda: yard.jittered_video(0, ndim=2), 0.16, (7,)),
    'jitter_3d': (lambda: yard.jittered_video(1, ndim=3), (0.21, 0.16, 0.16), (7,)),
    'jitter_2d_5': (lambda: yard.jittered_video(2, n_frames=5, n_particles=4, absent=(0, 2)), 1., (3,)),
}
_cache = {}


def _table(name):
    """(pos, off, par, mpp, {L: (per-particle, pooled) of the yardstick}): computed once, never changed"""
    if name not in _cache:
        make, mpp, lags = (EXACT.get(name) or ROUNDED[name])
        pos, off, par = make()
        _cache[name] = (pos, off, par, mpp, {L: (yard.msd(pos, off, par, L, mpp), yard.emsd(pos, off, par, L, mpp)) for L in lags})
    return _cache[name]


@pytest.mark.parametrize('name', sorted(EXACT))
def test_exact_tables_equal_the_yardstick_bit_for_bit(engine, name):
    pos, off, par, mpp, wants = _table(name)
    for L, (per, pooled) in wants.items():
        got = ct.msd_arrays(pos, off, par, L, mpp, fps=4.)
        assert isinstance(got.msd, np.ndarray) and got.n.dtype == np.int32 and got.status == _abi.MSD_OK
        np.testing.assert_array_equal(got.lagt, np.arange(1, L + 1) / 4.)
        yard.assert_equal_bits(got, per, (name, L))
        ens = ct.emsd_arrays(pos, off, par, L, mpp, fps=4.)
        assert isinstance(ens.msd, np.ndarray) and ens.n.dtype == np.int64 and ens.status == _abi.MSD_OK
        np.testing.assert_array_equal(ens.lagt, got.lagt)
        yard.assert_equal_bits(ens, pooled, (name, L, 'ensemble'))


def _shared_lags():
    """(pos, off, par, P, L, long_id, the yardstick's pooled result at mpp 0.5): computed once, never changed"""
    if 'shared_lags' not in _cache:
        P, L, long_id = 9 * CHUNK + 1, 460, 4 * CHUNK + 7
        tracks = [[0, 1]] * P
        tracks[long_id] = yard.span_with_gap(2, 450, (200, 203))
        pos, off, par = yard.exact_tracks(9, tracks)
        _cache['shared_lags'] = (pos, off, par, P, L, long_id, yard.emsd(pos, off, par, L, 0.5))
    return _cache['shared_lags']


def test_lags_of_a_chunk_shared_between_workgroups(engine):
    """Ten chunks of ids: the launch then gives the lags of a chunk to some 200 workgroups, and with
    460 lags each of them sums up to three lags, one after the other.  One track of 450 frames with
    a gap among tracks of two rows: the chunk with the long track reduces at every lag up to 449, the
    others write zeros from lag 2 on."""
    pos, off, par, P, L, long_id, want = _shared_lags()
    assert want.n[0] == P - 1 + 445 and want.n[448] == 1 and (want.n[449:] == 0).all() and (want.n[:449] > 0).all()
    ens = ct.emsd_arrays(pos, off, par, L, 0.5)
    yard.assert_equal_bits(ens, want, 'ensemble')
    ids = [0, long_id, P - 1]
    yard.assert_equal_bits(ct.msd_arrays(pos, off, par, L, 0.5, particles=ids), yard.msd(pos, off, par, L, 0.5, particles=ids), 'ids')


def test_the_edge_tables_hold_their_edges(engine):
    pos, off, par, _, wants = _table('spans')
    tracks = yard.tracks_of(off, par)
    assert [max(t) - min(t) + 1 for t in (tracks[p] for p in range(4))] == [TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
    assert [max(t) - min(t) + 1 - len(t) for t in (tracks[p] for p in range(4))] == [5, 5, 4, 5]        # the gaps
    assert (par == 3).sum() == len(tracks[3]) + 2 and (par < 0).sum() == 1
    per = wants[24][0]
    assert (per.n[:, 0] == [len(tracks[p]) - 2 for p in range(4)]).all() and (per.n[:, 5] > per.n[:, 0] - 12).all()
    pos, off, par, _, wants = _table('lengths')
    assert np.bincount(par).tolist() == [1, 2, 63, 64, 65, 255, 256, 257]
    assert wants[70][0].n[:, 0].tolist() == [0, 1, 62, 63, 64, 254, 255, 256] and np.isnan(wants[70][0].msd[1, 1:]).all()
    for ndim in (2, 3):
        pos, off, par, _, wants = _table('small_%dd' % ndim)
        assert len(off) - 1 == 6 and pos.shape[1] == ndim and (par < 0).sum() == 3
        assert (wants[9][0].n[:, 5:] == 0).all() and wants[5][0].n[0].tolist() == [2, 0, 1, 2, 1]
        assert wants[5][0].n[3].tolist() == [0] * 5 and wants[5][0].n[1].tolist() == [0] * 5
    for name, P in (('chunk_minus', CHUNK - 1), ('chunk', CHUNK), ('chunk_plus', CHUNK + 1), ('two_chunks_plus', 2 * CHUNK + 1)):
        assert _table(name)[4][3][1].n.tolist() == [2 * P, P, 0]


@pytest.mark.parametrize('name', ['small_2d', 'small_3d', 'lengths'])
def test_selected_particles(engine, name):
    """the first id, the last and an id without rows; alone and in a batch the same bytes"""
    pos, off, par, mpp, wants = _table(name)
    L = max(wants)
    P = int(par.max()) + 1
    ids = [0, P - 1, P + 1]
    want = yard.msd(pos, off, par, L, mpp, particles=ids, n_particles=P + 2)
    got = ct.msd_arrays(pos, off, par, L, mpp, particles=ids, n_particles=P + 2)
    assert got.msd.shape == (3, L)
    yard.assert_equal_bits(got, want, name)
    assert np.isnan(got.msd[2]).all() and (got.n[2] == 0).all()
    full = ct.msd_arrays(pos, off, par, L, mpp, n_particles=P + 2)
    assert full.msd.shape == (P + 2, L)
    for name in ('msd', 'mean_d', 'mean_d2', 'n'):
        assert getattr(full, name)[ids].tobytes() == getattr(got, name).tobytes()
    assert ct.msd_arrays(pos, off, par, L, mpp, particles=[]).msd.shape == (0, L)


@pytest.mark.parametrize('name', sorted(ROUNDED))
def test_rounded_tables_stay_within_the_derived_bounds(engine, name):
    pos, off, par, mpp, wants = _table(name)
    assert len(off) - 1 <= 6 and par.max() < 5
    for L, (per, pooled) in wants.items():
        yard.assert_within_bounds(ct.msd_arrays(pos, off, par, L, mpp), per, (name, L))
        yard.assert_within_bounds(ct.emsd_arrays(pos, off, par, L, mpp), pooled, (name, L, 'ensemble'))


def test_refused_tables(engine):
    import torch
    pos, off, par, mpp, wants = _table('small_2d')
    L = 5
    before = ct.msd_arrays(pos, off, par, L, mpp), ct.emsd_arrays(pos, off, par, L, mpp)
    falling = np.array(off)
    falling[2], falling[3] = falling[3] + 1, falling[2]
    beyond = np.array(off)
    beyond[-1] += 1
    P = int(par.max()) + 1
    for fn in (ct.msd_arrays, ct.emsd_arrays):
        for bad in (falling, beyond):
            with pytest.raises(ValueError, match='frame_offset'):
                fn(pos, bad, par, L, mpp)
        with pytest.raises(ValueError, match='n_particles'):
            fn(pos, off, par, L, mpp, n_particles=P - 1)
    t_pos, t_par = torch.from_numpy(np.array(pos)).cuda(), torch.from_numpy(np.array(par)).cuda()
    for t_off, n_particles in ((torch.from_numpy(falling).cuda(), P), (torch.from_numpy(np.array(off)).cuda(), P - 1)):
        got = ct.msd_arrays(t_pos, t_off, t_par, L, mpp, n_particles=n_particles)
        ens = ct.emsd_arrays(t_pos, t_off, t_par, L, mpp, n_particles=n_particles)
        for res, shape in ((got, (n_particles, L)), (ens, (L,))):
            assert int(res.status) == _abi.MSD_BAD_TABLE != 0 and tuple(res.msd.shape) == shape
            assert torch.isnan(res.msd).all() and torch.isnan(res.mean_d).all() and torch.isnan(res.mean_d2).all()
            assert not res.n.any()
    # the same calls after the refused ones: the bytes they gave before
    after = ct.msd_arrays(pos, off, par, L, mpp), ct.emsd_arrays(pos, off, par, L, mpp)
    for a, b in zip(before, after):
        assert b.status == _abi.MSD_OK
        for name in ('msd', 'mean_d', 'mean_d2', 'n'):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes()


def test_tensors_in_tensors_out(engine):
    import torch
    pos, off, par, mpp, wants = _table('jitter_3d')
    L = 7
    host, host_ens = ct.msd_arrays(pos, off, par, L, mpp, fps=2.), ct.emsd_arrays(pos, off, par, L, mpp, fps=2.)
    t_pos, t_off, t_par = (torch.from_numpy(np.array(a)).cuda() for a in (pos, off, par))
    P = int(par.max()) + 1
    for n_particles in (P, None):
        for _ in range(2):                      # two calls: identical bytes
            got = ct.msd_arrays(t_pos, t_off, t_par, L, mpp, fps=2., n_particles=n_particles)
            ens = ct.emsd_arrays(t_pos, t_off, t_par, L, mpp, fps=2., n_particles=n_particles)
            for res, ref in ((got, host), (ens, host_ens)):
                assert all(torch.is_tensor(x) and x.device == t_pos.device for x in res) and int(res.status) == _abi.MSD_OK
                for name in ('lagt', 'msd', 'mean_d', 'mean_d2', 'n'):
                    assert getattr(res, name).cpu().numpy().tobytes() == getattr(ref, name).tobytes(), name
            assert got.n.dtype == torch.int32 and ens.n.dtype == torch.int64
    sel = ct.msd_arrays(t_pos, t_off, t_par, L, mpp, particles=torch.tensor([1, 4], device=t_pos.device), n_particles=P)
    assert sel.msd.cpu().numpy().tobytes() == host.msd[[1, 4]].tobytes()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = ct.emsd_arrays(t_pos, t_off, t_par, L, mpp, n_particles=P)
    s.synchronize()
    assert other.msd.cpu().numpy().tobytes() == host_ens.msd.tobytes()
    with pytest.raises(ValueError, match='float64'):
        ct.msd_arrays(t_pos.float(), t_off, t_par, n_particles=P)


@pytest.mark.parametrize('name', ['jitter_2d', 'jitter_3d', 'small_3d'])
def test_ensemble_is_the_pooled_value_of_the_particles(engine, name):
    """emsd_arrays against the n-weighted mean of msd_arrays' own output.  With X the largest term and
    u = 2^-53: a particle's mean times n_p gives its sum back within (n_p - 1) n_p X u (its summation)
    + 2 n_p X u (division, product), at most (n_p + 1) n_p X u; those added exactly (fsum) and divided
    by n: (n + 1) X u + 2 X u; the ensemble's own sum and division: n X u: (2 n + 4) X u in all."""
    import math
    pos, off, par, mpp, wants = _table(name)
    L = max(wants)
    per, ens = ct.msd_arrays(pos, off, par, L, mpp), ct.emsd_arrays(pos, off, par, L, mpp)
    want = wants[L][0]
    n = per.n.astype(np.int64).sum(0)
    assert (ens.n == n).all()
    X = want.max_d.max(0)                      # per lag and coordinate, over the particles
    for name, scale in (('mean_d', X), ('mean_d2', X ** 2)):
        values = getattr(per, name)
        for k in range(L):
            for a in range(pos.shape[1]):
                if n[k] == 0:
                    assert np.isnan(getattr(ens, name)[k, a])
                    continue
                pooled = math.fsum(values[p, k, a] * per.n[p, k] for p in range(len(values)) if per.n[p, k]) / n[k]
                err = abs(getattr(ens, name)[k, a] - pooled)
                assert err <= (2 * n[k] + 4) * scale[k, a] * yard.U, (name, k, a, err)


def test_table_forms(engine):
    """non-dense particle ids and a first frame other than 0"""
    pos, off, par, mpp, wants = _table('jitter_2d')
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    f = pd.DataFrame({'y': pos[:, 0], 'x': pos[:, 1], 'frame': frame + 3, 'particle': (10 * par + 7).astype(np.int32)})
    # in a table every id is a particle: the unlinked row (-3) is a particle of one row, the first column
    ids, dense = np.unique(f['particle'].values, return_inverse=True)
    arrays = ct.msd_arrays(pos, off, dense, 4, mpp, fps=24.)
    im = ct.imsd(f, mpp, 24., max_lagtime=4)
    assert im.columns.tolist() == [-3, 7, 17, 27, 37, 47] == ids.tolist() and im.columns.name == 'particle'
    assert im.index.name == 'lagt' and im.index.tolist() == arrays.lagt.tolist()
    assert im.values.tobytes() == np.ascontiguousarray(arrays.msd.T).tobytes() and im[-3].isna().all() and im[7].notna().all()
    assert arrays.msd[1:].tobytes() == ct.msd_arrays(pos, off, par, 4, mpp).msd.tobytes()
    ens = ct.emsd_arrays(pos, off, dense, 4, mpp, fps=24.)
    em = ct.emsd(f, mpp, 24., max_lagtime=4)
    assert isinstance(em, pd.Series) and em.name == 'msd' and em.index.name == 'lagt'
    assert em.values.tobytes() == ens.msd.tobytes() and em.index.tolist() == ens.lagt.tolist()
    # rows in another order: the same table
    det = ct.emsd(f.iloc[np.random.RandomState(0).permutation(len(f))], mpp, 24., max_lagtime=4, detail=True)
    assert list(det.columns) == ['<y>', '<x>', '<y^2>', '<x^2>', 'msd', 'N', 'lagt'] and det.index.tolist() == [1, 2, 3, 4]
    assert det[['<y>', '<x>']].values.tobytes() == ens.mean_d.tobytes() and det['N'].tolist() == ens.n.tolist()
    assert det['msd'].values.tobytes() == ens.msd.tobytes() and det[['<y^2>', '<x^2>']].values.tobytes() == ens.mean_d2.tobytes()
    assert det['lagt'].tolist() == ens.lagt.tolist()


def test_scratch_grows_and_comes_back(engine):
    """a small call, a larger one (more particles, more rows, longer L), the small one again: the first bytes"""
    pos, off, par, mpp, wants = _table('small_3d')
    big = _table('two_chunks_plus')
    first = ct.msd_arrays(pos, off, par, 5, mpp), ct.emsd_arrays(pos, off, par, 5, mpp)
    grown = ct.msd_arrays(big[0], big[1], big[2], 40, big[3]), ct.emsd_arrays(big[0], big[1], big[2], 40, big[3])
    last = ct.msd_arrays(pos, off, par, 5, mpp), ct.emsd_arrays(pos, off, par, 5, mpp)
    for a, b in zip(first, last):
        for name in ('msd', 'mean_d', 'mean_d2', 'n'):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes()
    yard.assert_equal_bits(first[0], wants[5][0])
    yard.assert_equal_bits(first[1], wants[5][1])
    per, pooled = big[4][3]                     # the yardstick at L = 3: lags 1 and 2 have pairs, no other
    for name in ('msd', 'mean_d', 'mean_d2', 'n'):
        g, w = getattr(grown[0], name), getattr(per, name)
        assert g.shape[:2] == (2 * CHUNK + 1, 40) and (g[:, :2] == w[:, :2]).all()
        assert (g[:, 2:] == 0).all() if name == 'n' else np.isnan(g[:, 2:]).all()
        g, w = getattr(grown[1], name), getattr(pooled, name)
        assert g.shape[0] == 40 and (g[:2] == w[:2]).all()
        assert (g[2:] == 0).all() if name == 'n' else np.isnan(g[2:]).all()


def test_chain_from_frames_to_an_msd_without_drift(engine):
    """six Gaussians at integer centres, all shifted by (0, +1) per frame, no noise: located at the
    centres, so the MSD of the linked table is |v|^2 k^2 = k^2 exactly and 0 after the drift is subtracted"""
    import torch
    centres = np.array([(10, 8), (12, 30), (25, 18), (40, 9), (45, 40), (55, 24)])
    frames = np.zeros((8, 64, 64), dtype=np.uint8)
    for t in range(8):
        for y, x in centres:
            ct.artificial.draw_gaussian(frames[t], (y, x + t), 1.5, 200)
    r = ct.find_link_arrays(torch.from_numpy(frames).cuda(), search_range=4, separation=5, diameter=5, minmass=100,
                            _on_device=True)
    P = int(r.n_tracks)
    assert P == 6
    k = np.arange(1, 10.)
    want = np.where(k <= 7, k ** 2, np.nan)
    per = ct.msd_arrays(r.pos, r.frame_offset, r.particle, 9, n_particles=P)
    ens = ct.emsd_arrays(r.pos, r.frame_offset, r.particle, 9, n_particles=P)
    assert all(torch.is_tensor(x) for x in per) and int(per.status) == 0
    np.testing.assert_array_equal(per.msd.cpu().numpy(), np.tile(want, (6, 1)))
    np.testing.assert_array_equal(ens.msd.cpu().numpy(), want)
    np.testing.assert_array_equal(ens.n.cpu().numpy(), 6 * np.maximum(8 - k, 0))
    drift = ct.compute_drift_arrays(r.pos, r.frame_offset, r.particle, n_particles=P)
    fixed = ct.subtract_drift_arrays(r.pos, r.frame_offset, drift.drift)
    per = ct.msd_arrays(fixed, r.frame_offset, r.particle, 9, mpp=0.5, fps=10., n_particles=P)
    np.testing.assert_array_equal(per.msd.cpu().numpy(), np.tile(np.where(k <= 7, 0., np.nan), (6, 1)))
    np.testing.assert_array_equal(per.lagt.cpu().numpy(), k / 10.)
    assert (ct.emsd_arrays(fixed, r.frame_offset, r.particle, 9, n_particles=P).msd.cpu().numpy()[:7] == 0.).all()
