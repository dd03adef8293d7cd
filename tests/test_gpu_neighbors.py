"""Nearest neighbours and proximity on the device against the yardstick
``tests/_neighbors.py``.  ``dist2``, ``index``, ``count`` and ``particle_min2`` are the yardstick's bytes:
the same operations in the same order, and every element has one owner.  ``dist`` and ``particle_min``
lie within 1 ulp of ``np.sqrt`` of those squares (the largest difference seen is printed; on the MI355X
it was 0).  The tables are the smallest that reach every edge of the launch: the tile of 256 rows on the
owner side and on the candidate side, frames without a work item, every capacity of the list (1, 4, 16)
and the first ``k`` past one, ties on both sides of a tile edge, a candidate at exactly ``max_dist``."""
import numpy as np
import pandas as pd
import pytest

import _neighbors as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi

pytestmark = pytest.mark.gpu

TABLES = {2: yard.tile_edges(2), 3: yard.tile_edges(3)}
_want = {}


def want(ndim, lag, k):
    """the yardstick on the table of the tile edges: computed once per (ndim, lag) at k = 16 -- the first k
    of the 16 best are the k best -- and never changed"""
    if (ndim, lag) not in _want:
        _want[ndim, lag] = yard.neighbors(*TABLES[ndim], k=_abi.NBR_MAX_K, lag=lag)
    r = _want[ndim, lag]
    return yard.Result(r.dist[:, :k], r.dist2[:, :k], r.index[:, :k], r.count, None, None)


def compare(got, ref, what):
    """the exact outputs bit for bit, the square roots within 1 ulp; returns the largest ulp seen"""
    assert got.index.dtype == np.int64 and got.count.dtype == np.int64, what
    assert got.index.shape == ref.index.shape and got.count.shape == ref.count.shape, (what, got.index.shape, ref.index.shape)
    assert (got.index == ref.index).all(), (what, 'index', np.argwhere(got.index != ref.index)[:5])
    assert (got.count == ref.count).all(), (what, 'count', np.argwhere(got.count != ref.count)[:5])
    yard.assert_equal_bits(got.dist2, ref.dist2, (what, 'dist2'))
    worst = yard.ulps(got.dist, np.sqrt(ref.dist2))
    if ref.particle_min2 is None:
        assert got.particle_min is None and got.particle_min2 is None, what
    else:
        yard.assert_equal_bits(got.particle_min2, ref.particle_min2, (what, 'particle_min2'))
        worst = max(worst, yard.ulps(got.particle_min, np.sqrt(ref.particle_min2)))
    print(what, 'largest |sqrt - np.sqrt| in ulp:', worst)
    assert worst <= 1, (what, worst)
    return worst


def check(what, pos, off, **kw):
    got = ct.neighbors_arrays(pos, off, **kw)
    assert isinstance(got.dist, np.ndarray) and got.status == _abi.NBR_OK
    ref = yard.neighbors(pos, off, **kw)
    compare(got, ref, what)
    return got, ref


def blob(res):
    return b''.join(np.ascontiguousarray(x.cpu().numpy() if hasattr(x, 'cpu') else x).tobytes() for x in res[:-1] if x is not None)


# ---- the table of the tile edges: every capacity, every lag ----
def test_the_table_holds_its_edges():
    for ndim in (2, 3):
        assert np.diff(TABLES[ndim][1]).tolist() == [0, 1, 2, 255, 256, 257, 513] and TABLES[ndim][0].shape[1] == ndim
        assert sum(-(-n // yard.TILE) for n in np.diff(TABLES[ndim][1])) == 9           # work items
    r = want(2, 0, 16)
    assert (r.index[0] == -1).all() and r.count[0] == 0                                # the one-row frame
    assert r.index[1].tolist() == [2] + [-1] * 15 and r.count[1:3].tolist() == [1, 1]  # the two-row frame
    assert (r.index[3:] >= 0).all() and (np.diff(r.dist2[3:], axis=1) >= 0).all()
    ahead = want(2, 1, 1)
    assert ahead.index[0, 0] in (1, 2) and (ahead.index[-513:] == -1).all() and (ahead.count[-513:] == 0).all()
    assert (want(2, 7, 4).index == -1).all() and not want(3, 7, 4).count.any()


@pytest.mark.parametrize('lag', [0, 1, 2, 7])
@pytest.mark.parametrize('k', [1, 2, 4, 5, 16])
@pytest.mark.parametrize('ndim', [2, 3])
def test_tile_edges(engine, ndim, k, lag):
    pos, off = TABLES[ndim]
    got = ct.neighbors_arrays(pos, off, k=k, lag=lag)
    assert got.status == _abi.NBR_OK and got.dist.shape == (len(pos), k)
    compare(got, want(ndim, lag, k), ('tile_edges', ndim, k, lag))


def test_a_frame_with_fewer_rows_than_k(engine):
    pos, off = yard.uniform_frames(1, (3, 1, 0, 5), (9., 9.))
    for k in (3, 5, 16):
        got, ref = check(('few rows', k), pos, off, k=k)
        assert (got.index[:3, :2] >= 0).all() and (got.index[:3, 2:] == -1).all() and np.isnan(got.dist[:3, 2:]).all()
        assert (got.index[3] == -1).all() and got.count.tolist() == [2, 2, 2, 0, 4, 4, 4, 4, 4]
    check(('few rows', 'lag 1'), pos, off, k=4, lag=1)


def _holes():
    """rows that do not exist in the middle of a tile, of the owners and of the candidates"""
    pos, off = yard.uniform_frames(2, (300, 280), (40., 40., 40.), 3)
    pos[100] = np.nan
    pos[130, 1] = np.inf
    pos[131, 0] = -np.inf
    pos[270, 2] = np.nan
    pos[300 + 17] = np.nan
    pos[300 + 260, 0] = np.inf
    return pos, off


def test_rows_that_do_not_exist(engine):
    pos, off = _holes()
    gone = [100, 130, 131, 270, 317, 560]
    for lag in (0, 1):
        got, ref = check(('holes', lag), pos, off, k=4, lag=lag)
        assert (got.index[gone] == -1).all() and not got.count[gone].any() and np.isnan(got.dist2[gone]).all()
        assert not np.isin(got.index, gone).any()                           # nobody's neighbour
    assert (got.count[:300][np.isfinite(pos[:300]).all(1)] == 278).all()


def test_coincident_rows(engine):
    pos, off = yard.uniform_frames(4, (300,), (30., 30.))
    pos[5] = pos[6] = pos[7]
    pos[256] = pos[255]                                # across the tile edge
    pos[299] = pos[0]
    got, ref = check('coincident', pos, off, k=3)
    assert got.index[5, :2].tolist() == [6, 7] and got.index[7, :2].tolist() == [5, 6] and (got.dist2[5:8, :2] == 0.).all()
    assert got.index[255, 0] == 256 and got.index[256, 0] == 255 and got.index[0, 0] == 299 and got.dist[299, 0] == 0.
    same, _ = check('all rows equal', np.full((260, 2), 3.5), np.array([0, 260]), k=4)
    assert same.index[0].tolist() == [1, 2, 3, 4] and same.index[259].tolist() == [0, 1, 2, 3] and (same.dist == 0.).all()


def test_lattice_ties_across_the_tile_edge(engine):
    """20 x 20 unit lattice, row-major, one frame of 400 rows: row 250 has its four nearest at 230, 249,
    251 (first tile) and 270 (second tile), all at d2 = 1; ties go to the smaller row"""
    pos, off = yard.lattice(20, 20)
    for k in (2, 4, 16):
        got, ref = check(('lattice', k), pos, off, k=k)
        assert got.index[250, :min(k, 4)].tolist() == [230, 249, 251, 270][:k]
        assert got.index[236, :min(k, 4)].tolist() == [216, 235, 237, 256][:k]      # 256: the first row of the second tile
    assert got.dist2[250].tolist() == [1.] * 4 + [2.] * 4 + [4.] * 4 + [5.] * 4
    assert got.index[250, 4:8].tolist() == [229, 231, 269, 271]
    near, _ = check('lattice within 1.5', pos, off, k=4, max_dist=1.5)
    assert near.count[250] == 8 and near.count[0] == 3 and near.index[0].tolist() == [1, 20, 21, -1]


def test_a_candidate_at_exactly_max_dist(engine):
    pos, off = yard.lattice(20, 20)
    two, _ = check('lattice within 2', pos, off, k=16, max_dist=2.)
    assert two.count[250] == 8 and (two.index[250, 8:] == -1).all()           # the four at d2 = 4 = limit2 are out
    over, _ = check('lattice just over 2', pos, off, k=16, max_dist=float(np.nextafter(2., 3.)))
    assert over.count[250] == 12 and over.dist2[250, 8:12].tolist() == [4.] * 4
    five, _ = check('lattice within 5', pos, off, k=1, max_dist=5.)            # (3, 4) and (0, 5) apart: d2 = 25
    assert five.count[250] == 68                                               # 80 lattice points with d2 <= 25, 12 of them at 25
    tri = np.array([[0., 0.], [3., 4.], [6., 8.]])
    at = ct.neighbors_arrays(tri, np.array([0, 3]), k=2, max_dist=5.)
    assert at.count.tolist() == [0, 0, 0] and (at.index == -1).all() and np.isnan(at.dist).all()


def test_groups_same_and_other(engine):
    pos, off = TABLES[2]
    group = np.random.RandomState(6).randint(-3, 12, len(pos)).astype(np.int64)
    assert (group < 0).any()
    got = {p: check(('groups', p), pos, off, k=4, group=group, pairs=p, max_dist=9.)[0] for p in ('all', 'same', 'other')}
    assert (got['all'].count == got['same'].count + got['other'].count).all()
    assert got['same'].count.sum() > 0 and got['other'].count.sum() > 0
    assert not got['same'].count[group < 0].any()                              # group -1 is nobody's group
    found = got['same'].index >= 0
    assert (group[got['same'].index[found]] == np.broadcast_to(group[:, None], found.shape)[found]).all()
    ahead = {p: check(('groups ahead', p), pos, off, k=5, group=group, pairs=p, lag=1)[0] for p in ('all', 'same', 'other')}
    assert (ahead['all'].count == ahead['same'].count + ahead['other'].count).all()


@pytest.mark.parametrize('ndim', [2, 3])
def test_count_matches_pair_correlation(engine, ndim):
    """g(r) and the neighbours walk the same pairs (csrc/pair_walk.h): the pairs that g(r) bins in a frame
    are the candidates that the neighbours count in it, exactly, for every `pairs`, at the default grid cap
    and under a cap of two workgroups.  tests/test_neighbors_rule.py holds the two restatements to the same."""
    pos, off, group = yard.shared_rule(ndim)
    mpp = (0.5, 1., 2.)[:ndim]
    totals = {}
    for pairs in ('all', 'same', 'other'):
        def both():
            g = ct.pair_correlation_arrays(pos, off, yard.SHARED_CUTOFF, yard.SHARED_DR, mpp=mpp, edge='none', group=group, pairs=pairs)
            assert g.status == _abi.PCF_OK and g.count.shape == (len(off) - 1, 16) and g.r_edges[16] == yard.SHARED_CUTOFF
            n = ct.neighbors_arrays(pos, off, k=1, mpp=mpp, max_dist=float(g.r_edges[16]), group=group, pairs=pairs, lag=0)
            assert n.status == _abi.NBR_OK
            return g.count.sum(1), yard.counts_per_frame(n.count, off)
        binned, counted = both()
        print(ndim, pairs, 'pairs per frame', binned.tolist())
        assert binned.dtype == counted.dtype == np.int64 and (binned == counted).all(), (ndim, pairs, binned, counted)
        with engine.stage_max_grid(2):
            low_binned, low_counted = both()
        assert (low_binned == binned).all() and (low_counted == binned).all(), (ndim, pairs, low_binned, low_counted)
        totals[pairs] = binned
    assert (totals['all'] == totals['same'] + totals['other']).all()
    assert totals['all'][:2].tolist() == [0, 0] and (totals['same'][3:] > 0).all() and (totals['other'][3:] > 0).all()


def test_mpp_per_axis(engine):
    pos, off = TABLES[3]
    got, ref = check('mpp 3D', pos, off, k=4, mpp=(2., 1., 0.5), max_dist=11.)
    plain = ct.neighbors_arrays(pos, off, k=4)
    assert (got.index != plain.index).any()
    check('mpp 2D', *TABLES[2], k=5, mpp=(0.25, 0.5))
    check('mpp number', *TABLES[2], k=1, mpp=0.3)


def test_rows_outside_every_frame(engine):
    pos, _ = yard.uniform_frames(8, (7,), (5., 5.))
    got, ref = check('outside', pos, np.array([2, 5]), k=2)
    assert (got.index[[0, 1, 5, 6]] == -1).all() and not got.count[[0, 1, 5, 6]].any() and np.isnan(got.dist[[0, 1, 5, 6]]).all()
    assert got.count[2:5].tolist() == [2, 2, 2] and ((got.index[2:5] >= 2) & (got.index[2:5] < 5)).all()
    got, ref = check('outside, two frames', pos, np.array([1, 3, 6]), k=2, lag=1, particle=np.arange(7) % 3, n_particles=3)
    assert (got.index[[0, 3, 4, 5, 6]] == -1).all() and ((got.index[1:3, :2] >= 3) & (got.index[1:3, :2] < 6)).all()


def _particles(n):
    particle = np.random.RandomState(9).randint(-2, 40, n).astype(np.int64)
    particle[particle == 7] = 8                    # absent
    particle[particle == 33] = 32
    particle[0] = 33                               # the one-row frame: always alone
    return particle


def test_per_particle(engine):
    pos, off = TABLES[2]
    particle = _particles(len(pos))
    got, ref = check('particles', pos, off, k=2, particle=particle, n_particles=35)      # ids 35 .. 39 and < 0 are out of range
    assert got.particle_min.shape == (35,) and np.isnan(got.particle_min[[7, 33]]).all()
    assert np.isfinite(np.delete(got.particle_min, [7, 33])).all()
    whole, _ = check('particles, P from the ids', pos, off, k=1, particle=particle)
    assert whole.particle_min.shape == (40,) and whole.particle_min2[:35].tobytes() == got.particle_min2.tobytes()
    check('particles ahead', pos, off, k=1, lag=1, particle=particle, n_particles=35, max_dist=4.)
    none, _ = check('no particle in range', pos, off, k=1, particle=np.full(len(pos), 5, dtype=np.int64), n_particles=3)
    assert np.isnan(none.particle_min).all()
    # the scratch grows with P and comes back
    wide, _ = check('many ids', pos, off, k=1, particle=particle * 1000 + 2000, n_particles=50000)
    assert np.isfinite(wide.particle_min).sum() == 40            # the 42 ids -2 .. 39 without 7 (absent) and 33 (alone)
    again = ct.neighbors_arrays(pos, off, k=2, particle=particle, n_particles=35)
    assert blob(again) == blob(got)


BAD_OFFSETS = ([0, 5, 3, 1284], [0, 3, 3, 1285], [-1, 3, 4, 4])


def test_a_refused_table(engine):
    import torch
    pos, off = TABLES[2]
    particle = _particles(len(pos))
    t_pos, t_par = torch.from_numpy(pos).cuda(), torch.from_numpy(particle).cuda()
    assert len(pos) == 1284
    for bad in BAD_OFFSETS:
        b_off = np.array(bad, dtype=np.int64)
        res = ct.neighbors_arrays(t_pos, torch.from_numpy(b_off).cuda(), k=5, particle=t_par, n_particles=35)
        assert int(res.status) == _abi.NBR_BAD_TABLE
        host = [x.cpu().numpy() for x in res[:-1]]
        ref = yard.refused(len(pos), 5, 35)
        for g, w in zip(host[:2] + host[4:], (ref.dist, ref.dist2, ref.particle_min, ref.particle_min2)):
            assert g.shape == w.shape and np.isnan(g).all()
        assert host[2].shape == (1284, 5) and (host[2] == -1).all() and host[3].shape == (1284,) and not host[3].any()
        with pytest.raises(ValueError, match='frame_offset'):
            ct.neighbors_arrays(pos, b_off, k=5, particle=particle, n_particles=35)
    good = ct.neighbors_arrays(t_pos, torch.from_numpy(off).cuda(), k=5)        # the handle is as good as before
    assert int(good.status) == _abi.NBR_OK
    compare(ct.static.Neighbors(*(x if x is None else x.cpu().numpy() for x in good)), want(2, 0, 5), 'after the refusals')


def test_no_rows_and_no_frames(engine):
    for ndim in (2, 3):
        none = ct.neighbors_arrays(np.zeros((0, ndim)), np.zeros(1, dtype=np.int64), k=3)
        assert none.dist.shape == none.dist2.shape == none.index.shape == (0, 3) and none.count.shape == (0,) and none.status == 0
        assert none.particle_min is None
    empty = ct.neighbors_arrays(np.zeros((0, 2)), np.zeros(3, dtype=np.int64), k=1, particle=np.zeros(0, dtype=np.int64), n_particles=4)
    assert empty.dist.shape == (0, 1) and empty.particle_min.shape == (4,) and np.isnan(empty.particle_min).all()
    assert np.isnan(empty.particle_min2).all()
    nothing = ct.neighbors_arrays(np.zeros((0, 2)), np.zeros(1, dtype=np.int64), particle=np.zeros(0, dtype=np.int64))
    assert nothing.particle_min.shape == (0,)
    pos, _ = yard.uniform_frames(8, (300,), (5., 5.))
    for off in ([0], [300], [7, 7]):                   # rows, but no frame that holds one
        got, ref = check(('no frame', off), pos, np.array(off, dtype=np.int64), k=2)
        assert (got.index == -1).all() and not got.count.any() and np.isnan(got.dist).all() and np.isnan(got.dist2).all()


def test_tensors_in_tensors_out(engine):
    import torch
    pos, off = TABLES[3]
    group = np.random.RandomState(6).randint(-3, 12, len(pos)).astype(np.int64)
    particle = _particles(len(pos))
    kw = dict(k=5, mpp=(1., 0.5, 2.), max_dist=30., pairs='other', lag=1)
    ref = yard.neighbors(pos, off, group=group, particle=particle, n_particles=35, **kw)
    t_pos, t_off = torch.from_numpy(pos).cuda(), torch.from_numpy(off).cuda()
    t_kw = dict(kw, group=torch.from_numpy(group).cuda(), particle=torch.from_numpy(particle).cuda(), n_particles=35)
    first = None
    for _ in range(2):                           # two calls: the same bytes
        got = ct.neighbors_arrays(t_pos, t_off, **t_kw)
        assert all(torch.is_tensor(x) and x.device == t_pos.device for x in got)
        assert got.status.dtype == torch.int32 and got.status.shape == (1,) and int(got.status) == _abi.NBR_OK
        assert got.index.dtype == got.count.dtype == torch.int64 and got.dist.dtype == got.particle_min.dtype == torch.float64
        compare(ct.static.Neighbors(*(x.cpu().numpy() for x in got)), ref, 'tensors')
        first = first or blob(got)
        assert blob(got) == first
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = ct.neighbors_arrays(t_pos, t_off, **t_kw)
    s.synchronize()
    assert blob(other) == first
    again = ct.neighbors_arrays(pos, off, group=group, particle=particle, n_particles=35, **kw)       # the same bytes from ndarrays
    assert isinstance(again.dist, np.ndarray) and again.status == _abi.NBR_OK and blob(again) == first
    counted = ct.neighbors_arrays(t_pos, t_off, k=1, particle=t_kw['particle'])       # P from the tensor: the one host read
    assert counted.particle_min.shape == (40,)
    with pytest.raises(ValueError, match='float64'):
        ct.neighbors_arrays(t_pos.float(), t_off)
    with pytest.raises(ValueError, match='int64'):
        ct.neighbors_arrays(t_pos, t_off, group=t_kw['group'].int(), pairs='same')
    with pytest.raises(ValueError, match='int64'):
        ct.neighbors_arrays(t_pos, t_off, particle=t_kw['particle'].int())


@pytest.mark.parametrize('ndim,k,lag', [(2, 1, 0), (2, 16, 0), (3, 4, 0), (3, 5, 1), (2, 2, 2)])
def test_under_a_lowered_grid_cap(engine, ndim, k, lag):
    """one workgroup, then three, walk the 9 work items, the 1284 rows of the defaults and the 35 keys: the
    bytes of the default run"""
    pos, off = TABLES[ndim]
    particle = _particles(len(pos))
    call = lambda: ct.neighbors_arrays(pos, off, k=k, lag=lag, particle=particle, n_particles=35)
    base = call()
    compare(ct.static.Neighbors(*base[:4], None, None, 0), want(ndim, lag, k), ('default cap', ndim, k, lag))
    for cap in (1, 3):
        with engine.stage_max_grid(cap):
            got = call()
        assert got.status == _abi.NBR_OK and blob(got) == blob(base), (ndim, k, lag, cap)
    outside = lambda: ct.neighbors_arrays(pos, np.array([300, 700, 1000]), k=k, lag=lag)
    base = outside()
    for cap in (1, 3):
        with engine.stage_max_grid(cap):
            assert blob(outside()) == blob(base)
    assert engine.set_stage_max_grid(0) == 65536


# ---- the table forms ----
def _linked():
    """three frames, 4 .. 6, of a dimer, a second dimer and a single that is alone in frame 6; the rows
    shuffled; `particle` ids that are not dense, `cluster` as a second integer column"""
    rows = []
    for t in range(3):
        rows += [(4 + t, 10. + t, 10., 10, 0), (4 + t, 10. + t, 13., 20, 0),             # a dimer, bond 3
                 (4 + t, 30., 30. + t, 35, 1), (4 + t, 34., 33. + t, 40, 1)]             # another, bond 5
    rows += [(4, 50., 10., 77, 2), (5, 50., 11., 77, 2)]
    f = pd.DataFrame(rows, columns=['frame', 'y', 'x', 'particle', 'cluster'])
    f.loc[len(f)] = (9, 1., 1., 99, 3)             # alone in its frame, after a gap of two empty frames
    f = f.astype({'frame': np.int64, 'particle': np.int64, 'cluster': np.int32})
    return f.iloc[np.random.RandomState(3).permutation(len(f))]


def _by_hand(f, **kw):
    """the restatement on the rows sorted by frame, brought back into the row order of f"""
    frames = f['frame'].values
    order = np.argsort(frames, kind='stable')
    off = np.searchsorted(frames[order], np.arange(frames.min(), frames.max() + 2), side='left')
    group = kw.pop('group', None)
    res = yard.neighbors(f[['y', 'x']].values[order], off, group=None if group is None else f[group].values[order], **kw)
    dist, neighbor, count = np.empty_like(res.dist), np.empty_like(res.index), np.empty_like(res.count)
    for s, r in enumerate(order):                  # sorted row s is row r of f
        dist[r], count[r] = res.dist[s], res.count[s]
        neighbor[r] = [order[j] if j >= 0 else -1 for j in res.index[s]]
    return dist, neighbor, count


def test_neighbors_of_a_table(engine):
    f = _linked()
    assert not f['frame'].is_monotonic_increasing
    yx, frame = f[['y', 'x']].values, f['frame'].values
    for kw in (dict(k=2), dict(k=1, lag=1), dict(k=3, max_dist=6., mpp=0.5), dict(k=2, group='cluster', pairs='same'),
               dict(k=2, group='cluster', pairs='other', max_dist=45.)):
        want_dist, want_neighbor, want_count = _by_hand(f, **dict(kw))
        call = dict(kw)
        if 'group' in call:
            call['group_column'] = call.pop('group')
        dist, neighbor, count = ct.neighbors(f, **call)
        assert (neighbor == want_neighbor).all() and (count == want_count).all() and neighbor.dtype == np.int64, kw
        assert yard.ulps(dist, want_dist) <= 1 and dist.shape == (len(f), kw['k'])
        # what the columns mean, from the table alone
        for r in range(len(f)):
            for m, n in enumerate(neighbor[r]):
                if n < 0:
                    assert np.isnan(dist[r, m])
                    continue
                assert frame[n] == frame[r] + kw.get('lag', 0) and (n != r or kw.get('lag', 0))
                d = (yx[n] - yx[r]) * kw.get('mpp', 1.)
                assert abs(dist[r, m] - np.sqrt(d[0] * d[0] + d[1] * d[1])) <= 2. ** -52 * dist[r, m]
    dist, neighbor, count = ct.neighbors(f, k=1, group_column='cluster', pairs='same')
    bond = pd.Series(dist[:, 0], index=f['cluster'].values).groupby(level=0).min()
    assert bond.loc[0] == 3. and bond.loc[1] == 5. and np.isnan(bond.loc[2]) and np.isnan(bond.loc[3])


def test_proximity_of_a_linked_table(engine):
    f = _linked()
    prox = ct.proximity(f)
    assert prox.index.tolist() == [10, 20, 35, 40, 77, 99] and prox.index.name == 'particle' and prox.columns.tolist() == ['proximity']
    dist, _, _ = _by_hand(f, k=1)
    by_hand = pd.Series(dist[:, 0], index=f['particle'].values).groupby(level=0).min()
    assert yard.ulps(prox['proximity'].values, by_hand.loc[prox.index].values) <= 1
    assert prox.loc[10, 'proximity'] == 3. and prox.loc[35, 'proximity'] == 5. and np.isnan(prox.loc[99, 'proximity'])
    half = ct.proximity(f, mpp=0.5)
    assert half.loc[20, 'proximity'] == 1.5 and half.loc[40, 'proximity'] == 2.5
