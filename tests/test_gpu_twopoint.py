"""Two-point displacement correlations on the device against the yardstick
``tests/_twopoint.py``.  The integer outputs ``n``, ``n_moved``, ``beyond`` and the dot and L sums are the
yardstick's exactly: the same operations in the same order, and integer sums in any order.  The c sum lies
within ``n[k, b]`` units of the yardstick's: a last-place difference of ``sqrt`` or of the division behind it
can move a pair's integer by at most one (the largest difference seen is printed; on the MI355X it was 0).
The means are the bytes of clause 10 applied to the device's own integers.  The tables are the smallest that
reach every edge of the launch: the tile of 256 rows on the owner side and on the candidate side, the LDS
table of 2048 partners, the flush after 32 candidate tiles, and the exact limits of the rule."""
import numpy as np
import pytest

import _twopoint as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi

pytestmark = pytest.mark.gpu

_tables, _want = {}, {}


def table(name, *args):
    """the table of a case, built once"""
    key = (name,) + args
    if key not in _tables:
        _tables[key] = getattr(yard, name)(*args)
    return _tables[key]


def want(key, pos, off, particle, lags, **kw):
    """the yardstick of a case: computed once, shared and never changed"""
    if key not in _want:
        _want[key] = yard.twopoint(pos, off, particle, lags, **kw)
    return _want[key]


def host(res):
    return type(res)(*(x.cpu().numpy() if hasattr(x, 'cpu') else x for x in res))


def blob(res):
    return b''.join(np.ascontiguousarray(x.cpu().numpy() if hasattr(x, 'cpu') else x).tobytes() for x in res[:-2])


def compare(got, ref, ndim, what):
    """the integers exactly, the c sum within n, the means bit for bit from the device's integers; returns
    the largest difference of a c sum"""
    got = host(got)
    assert got.n.dtype == got.sums.dtype == got.n_moved.dtype == got.beyond.dtype == got.lags.dtype == np.int64, what
    assert got.n.shape == ref.n.shape and got.sums.shape == ref.n.shape + (3, 2), (what, got.n.shape, got.sums.shape)
    assert (got.r_edges == ref.r_edges).all() and (got.lags == ref.lags).all() and got.unit == ref.unit, what
    assert (got.n == ref.n).all(), (what, 'n', np.argwhere(got.n != ref.n)[:5])
    assert (got.n_moved == ref.n_moved).all() and (got.beyond == ref.beyond).all(), (what, got.n_moved, ref.n_moved, got.beyond, ref.beyond)
    mine = yard.integers(got.sums)
    worst = 0
    for k in range(len(ref.lags)):
        for b in range(ref.n.shape[1]):
            assert mine[k][b][:2] == ref.sums[k][b][:2], (what, k, b, mine[k][b], ref.sums[k][b])
            off_by = abs(mine[k][b][2] - ref.sums[k][b][2])
            assert off_by <= ref.n[k, b], (what, k, b, off_by, ref.n[k, b])
            worst = max(worst, off_by)
    print(what, 'largest |c sum - yardstick| in units of 2^-40:', worst)
    m = yard.means(got.n, got.sums, got.unit, ndim)
    for name in ('dot', 'longitudinal', 'transverse', 'cos'):
        yard.assert_equal_bits(getattr(got, name), getattr(m, name), (what, name))
    return worst


def check(what, pos, off, particle, lags, **kw):
    got = ct.twopoint_arrays(pos, off, particle, lags, **kw)
    assert isinstance(got.n, np.ndarray) and got.status == _abi.TP_OK
    ref = want(what, pos, off, particle, lags, **kw)
    compare(got, ref, pos.shape[1], what)
    return got, ref


# ---- the tile edges ----
def test_the_table_holds_its_edges():
    for ndim in (2, 3):
        pos, off, particle, group = table('tile_edges', ndim)
        assert np.diff(off).tolist() == [513, 257, 256, 255, 2, 1, 0, 513] and pos.shape[1] == ndim
        assert (particle < 0).sum() == 1 and particle.max() < 520 and np.isnan(pos).any(1).sum() == 2 and np.isinf(pos).any(1).sum() == 1
        assert len(set(particle[:off[1]])) < off[1]                                      # a repeated id
        ref = want(('tile', ndim), pos, off, particle, yard.TILE_LAGS, **yard.TILE_KW)
        assert (ref.beyond > 0).all() and (ref.n_moved > 0).all() and (ref.n.sum(1) > 0).all()
        assert ref.n_moved[0] < ref.n_moved[0] + ref.beyond[0] < off[6]
        q = pos[:off[1]]
        rows, u, u2, moved, far = yard.displacements(pos, particle, off, 0, 1, 2.25)
        twins = [(i, j) for i in np.nonzero(moved)[0] for j in np.nonzero(moved)[0] if i < j and (q[i] == q[j]).all()]
        assert twins and all((u[i] == u[j]).all() for i, j in twins)                   # coincident rows that have moved


@pytest.mark.parametrize('ndim', [2, 3])
def test_tile_edges(engine, ndim):
    pos, off, particle, group = table('tile_edges', ndim)
    got, ref = check(('tile', ndim), pos, off, particle, yard.TILE_LAGS, **yard.TILE_KW)
    assert got.n.shape == (3, 16) and got.sums.shape == (3, 16, 3, 2)
    one = ct.twopoint_arrays(pos, off, particle, 7, **yard.TILE_KW)                    # an int: one lag
    assert one.lags.tolist() == [7] and (one.n[0] == got.n[2]).all() and (one.sums[0] == got.sums[2]).all()


def test_mpp_per_axis(engine):
    pos, off, particle, group = table('tile_edges', 3)
    check('mpp 3D', pos, off, particle, [1, 2], cutoff=9., dr=0.75, max_disp=2., mpp=(2., 1., 0.5))
    pos, off, particle, group = table('tile_edges', 2)
    check('mpp number', pos, off, particle, [1], cutoff=3., dr=0.125, max_disp=0.4, mpp=0.3)


# ---- the matching edges ----
@pytest.mark.parametrize('variant', ['alone', 'repeated'])
def test_matching_edges(engine, variant):
    pos, off, particle = table('matching_edges', variant)
    assert np.diff(off).tolist() == [2049, 2048, 2049]
    got, ref = check(('matching', variant), pos, off, particle, [1, 2], cutoff=8., dr=0.5, max_disp=1.5)
    last = off[2] + 2048
    partner = yard.partners(particle, np.arange(off[1], off[2]), np.arange(off[2], off[3]))
    if variant == 'alone':
        assert partner[7] == last and yard.partners(particle, np.arange(off[1]), np.arange(off[2], off[3]))[5] == last
    else:
        assert partner[7] == last - 1 and partner[8] == off[2] + 3 and particle[last] == particle[last - 1]
    assert ref.n_moved[0] > 4000 and ref.beyond[0] > 0


# ---- the flush in the middle of a walk ----
def test_flush_carry_and_sign(engine):
    """What this table pins is the flush itself: many work items add into one cell, so the carry out of the low
    word and the sign extension of a negative sum both run.  The flush after 32 candidate tiles happens here (33
    tiles) and is shown to be harmless, not to be needed: these sums would fit the int64 of LDS without it, and a
    table on which they would not is far beyond a test."""
    pos, off, particle = table('flush_table')
    assert np.diff(off).tolist() == [8193, 8193] and -(-8193 // yard.TILE) == 33
    got, ref = check('flush', pos, off, particle, [1], cutoff=8., dr=0.5, max_disp=4.)
    assert (ref.n[0] > 0).all()                                                          # every bin is populated
    flat = [v for cell in ref.sums[0] for v in cell]
    assert min(flat) < 0 < max(flat)                                                     # the sign extension and the carry both run
    assert (got.sums[0, :, :, 0] == -1).any() and (got.sums[0, :, :, 0] == 0).any()


# ---- the exact limits ----
def test_exact_limits_on_a_lattice(engine):
    moves = np.tile([1., 0.], (144, 1))
    moves[0] = [3., 4.]                               # u2 == max2: it has moved
    moves[1] = [3., 5.]                               # beyond
    pos, off, particle = yard.lattice_frames(12, 12, [moves])
    got, ref = check('limits', pos, off, particle, [1], cutoff=5., dr=1., max_disp=5.)
    assert got.n_moved.tolist() == [143] and got.beyond.tolist() == [1] and got.unit == 2. ** -35
    ij = np.delete(pos[:144], 1, axis=0).astype(np.int64)
    d2 = ((ij[:, None, :] - ij[None, :, :]) ** 2).sum(-1)
    by_hand = [int(((d2 >= b * b) & (d2 < (b + 1) * (b + 1)) & (d2 > 0)).sum()) for b in range(5)]
    assert got.n[0].tolist() == by_hand and by_hand[0] == 0
    assert (d2 == 25).sum() > 0 and (d2 == 4).sum() > 0       # d2 == edge2[B] is no pair; d2 == edge2[2] falls in bin 2
    assert got.n[0].sum() == ((d2 > 0) & (d2 < 25)).sum()
    closer = ct.twopoint_arrays(pos, off, particle, 1, 5., 1., float(np.nextafter(5., 0.)))
    assert closer.n_moved.tolist() == [142] and closer.beyond.tolist() == [2]


def test_rigid_translation(engine):
    """every row moves by (0.25, -0.5) per frame: dot is exactly 0.3125 k^2 and the c sum exactly n 2^40"""
    pos, off, particle = yard.lattice_frames(20, 15, [(0.25, -0.5)] * 3)
    got, ref = check('rigid', pos, off, particle, [1, 2, 3], cutoff=6., dr=0.5, max_disp=4.)
    assert got.n_moved.tolist() == [900, 600, 300] and not got.beyond.any()
    mine = yard.integers(got.sums)
    for ki, k in enumerate((1, 2, 3)):
        has = got.n[ki] > 0
        assert has.sum() >= 8 and (got.dot[ki][has] == 0.3125 * k * k).all() and (got.cos[ki][has] == 1.).all()
        assert np.isnan(got.dot[ki][~has]).all()
        assert all(mine[ki][b][2] == int(got.n[ki, b]) << 40 for b in range(12))


# ---- groups ----
def test_same_plus_other_is_all(engine):
    pos, off, particle, group = table('tile_edges', 2)
    got = {}
    for pairs in ('all', 'same', 'other'):
        got[pairs], _ = check(('groups', pairs), pos, off, particle, yard.TILE_LAGS, group=group, pairs=pairs, **yard.TILE_KW)
    assert (got['all'].n == got['same'].n + got['other'].n).all() and got['same'].n.sum() > 0 and got['other'].n.sum() > 0
    a, s, o = (yard.integers(got[p].sums) for p in ('all', 'same', 'other'))
    for k in range(3):
        for b in range(16):
            assert a[k][b] == [x + y for x, y in zip(s[k][b], o[k][b])], (k, b)
    assert (got['all'].n % 2 == 0).all() and all(v % 2 == 0 for lag in a for cell in lag for v in cell)
    assert (got['same'].n_moved == got['all'].n_moved).all()


# ---- against g(r) ----
@pytest.mark.parametrize('ndim', [2, 3])
def test_counts_match_pair_correlation(engine, ndim):
    """every row has moved and none coincide: the pairs of lag k are the pairs that g(r) bins in the frames
    t < T - k (csrc/pair_walk.h walks both)"""
    pos, off, particle = yard.walkers((300, 300, 300, 300), (40., 20.)[ndim - 2], 0.3, 8, ndim)
    res = ct.twopoint_arrays(pos, off, particle, [1, 2, 3], 8., 0.5, 100.)
    g = ct.pair_correlation_arrays(pos, off, 8., 0.5, edge='none')
    assert res.n_moved.tolist() == [900, 600, 300] and not res.beyond.any() and g.count.shape == (4, 16)
    for ki, k in enumerate((1, 2, 3)):
        assert (res.n[ki] == g.count[:4 - k].sum(0)).all() and res.n[ki].sum() > 0, (ndim, k)


# ---- refused tables, no rows, no frames ----
def test_a_refused_table(engine):
    import torch
    pos, off, particle, group = table('tile_edges', 2)
    t_pos, t_off, t_par = (torch.from_numpy(x).cuda() for x in (pos, off, particle))
    bad_off = off.copy()
    bad_off[3] = bad_off[2] - 1
    cases = [(torch.from_numpy(bad_off).cuda(), t_par, 520, bad_off, particle),
             (torch.tensor([0, len(pos) + 1], device='cuda'), t_par, 520, np.array([0, len(pos) + 1]), particle),
             (torch.tensor([-1, 4], device='cuda'), t_par, 520, np.array([-1, 4]), particle),
             (t_off, t_par, int(particle.max()), off, particle)]                         # an id >= P
    for c_off, c_par, P, h_off, h_par in cases:
        res = ct.twopoint_arrays(t_pos, c_off, c_par, [1, 2], n_particles=P, **yard.TILE_KW)
        assert int(res.status) == _abi.TP_BAD_TABLE
        h = host(res)
        for x in (h.dot, h.longitudinal, h.transverse, h.cos):
            assert x.shape == (2, 16) and np.isnan(x).all()
        assert not h.n.any() and not h.sums.any() and not h.n_moved.any() and not h.beyond.any()
        with pytest.raises(ValueError, match='frame_offset'):
            ct.twopoint_arrays(pos, h_off, h_par, [1, 2], n_particles=P, **yard.TILE_KW)
    good = ct.twopoint_arrays(t_pos, t_off, t_par, yard.TILE_LAGS, n_particles=520, **yard.TILE_KW)      # the handle is as good as before
    assert int(good.status) == _abi.TP_OK
    compare(good, want(('tile', 2), pos, off, particle, yard.TILE_LAGS, **yard.TILE_KW), 2, 'after the refusals')


def test_no_rows_and_no_frames(engine):
    none = np.zeros(0, dtype=np.int64)
    for ndim in (2, 3):
        for off in ([0], [0, 0, 0]):
            res = ct.twopoint_arrays(np.zeros((0, ndim)), np.array(off), none, [1, 4], 2., 0.5, 1.)
            assert res.status == 0 and res.n.shape == (2, 4) and not res.n.any() and not res.sums.any()
            assert not res.n_moved.any() and not res.beyond.any() and np.isnan(res.dot).all() and np.isnan(res.cos).all()
    pos, off, particle = yard.walkers((300,), 5., 0.1, 1)
    for o in ([0], [300], [7, 7], [0, 300]):              # rows, but no frame that holds one, or no frame a lag on
        res = ct.twopoint_arrays(pos, np.array(o), particle, 1, 2., 0.5, 1.)
        assert not res.n.any() and not res.n_moved.any() and np.isnan(res.transverse).all()
    pos, off, particle = yard.walkers((20, 20, 20), 5., 0.1, 1)
    inner = ct.twopoint_arrays(pos, np.array([20, 40, 60]), particle, 1, 2., 0.5, 1.)        # rows outside the frames take no part
    alone = ct.twopoint_arrays(pos[20:], np.array([0, 20, 40]), particle[20:], 1, 2., 0.5, 1.)
    assert blob(inner) == blob(alone) and inner.n_moved.tolist() == [20]


# ---- tensors ----
def test_tensors_in_tensors_out(engine):
    import torch
    pos, off, particle, group = table('tile_edges', 3)
    kw = dict(cutoff=8., dr=0.5, max_disp=1.5, mpp=(1., 0.5, 2.), pairs='other')
    ref = want('tensors', pos, off, particle, [1, 2, 7], group=group, **kw)
    t_pos, t_off, t_par, t_group = (torch.from_numpy(x).cuda() for x in (pos, off, particle, group))
    first = None
    for _ in range(3):                               # three calls: the same bytes
        got = ct.twopoint_arrays(t_pos, t_off, t_par, [1, 2, 7], group=t_group, n_particles=520, **kw)
        assert all(torch.is_tensor(x) and x.device == t_pos.device for x in got[:10]) and isinstance(got.unit, float)
        assert got.status.dtype == torch.int32 and got.status.shape == (1,) and int(got.status) == _abi.TP_OK
        assert got.n.dtype == got.sums.dtype == got.lags.dtype == torch.int64 and got.dot.dtype == got.r_edges.dtype == torch.float64
        first = first or blob(got)
        assert blob(got) == first
    compare(got, ref, 3, 'tensors')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = ct.twopoint_arrays(t_pos, t_off, t_par, [1, 2, 7], group=t_group, n_particles=520, **kw)
    s.synchronize()
    assert blob(other) == first
    again = ct.twopoint_arrays(pos, off, particle, [1, 2, 7], group=group, n_particles=520, **kw)        # the same bytes from ndarrays
    assert isinstance(again.n, np.ndarray) and again.status == _abi.TP_OK and blob(again) == first
    counted = ct.twopoint_arrays(t_pos, t_off, t_par, 1, 8., 0.5, 1.5)                  # P from the tensor: the one host read
    assert int(counted.status) == _abi.TP_OK
    with pytest.raises(ValueError, match='float64'):
        ct.twopoint_arrays(t_pos.float(), t_off, t_par, 1, 8., 0.5, 1.5)
    with pytest.raises(ValueError, match='int64'):
        ct.twopoint_arrays(t_pos, t_off, t_par.int(), 1, 8., 0.5, 1.5)
    with pytest.raises(ValueError, match='int64'):
        ct.twopoint_arrays(t_pos, t_off, t_par, 1, 8., 0.5, 1.5, group=t_group.int(), pairs='same')


# ---- a lowered grid cap ----
@pytest.mark.parametrize('ndim', [2, 3])
def test_under_a_lowered_grid_cap(engine, ndim):
    """one workgroup, then three, walk the 3 x 8 items of the partners, the 3 x 9 of the pairs, the rows of the
    check and the words of the defaults: the bytes of the default run"""
    pos, off, particle, group = table('tile_edges', ndim)
    call = lambda: ct.twopoint_arrays(pos, off, particle, yard.TILE_LAGS, group=group, pairs='other', **yard.TILE_KW)
    base = call()
    for cap in (1, 3):
        with engine.stage_max_grid(cap):
            got = call()
        assert got.status == _abi.TP_OK and blob(got) == blob(base), (ndim, cap)
    assert engine.set_stage_max_grid(0) == 65536


# ---- the table form ----
def test_twopoint_of_a_table(engine):
    f = yard.linked_table()
    assert not f['frame'].is_monotonic_increasing
    one = ct.twopoint(f, 1, 4., 1., 2.)
    assert one.index.name == 'r' and one.index.tolist() == [0., 1., 2., 3.]
    assert one.columns.tolist() == ['n', 'dot', 'longitudinal', 'transverse', 'cos'] and one['n'].tolist() == [0, 0, 0, 12]
    assert one.loc[3., 'dot'] == (0.25 - 0.0625) / 2 and np.isnan(one.loc[0., 'cos'])
    frames = f['frame'].values
    order = np.argsort(frames, kind='stable')
    off = np.searchsorted(frames[order], np.arange(3, 8), side='left')
    ids, dense = np.unique(f['particle'].values[order], return_inverse=True)
    ref = yard.twopoint(f[['y', 'x']].values[order], off, dense, [1, 3], 4., 1., 2., mpp=0.5, group=f['cluster'].values[order], pairs='same')
    m = yard.means(ref.n, yard.words(ref.sums), ref.unit, 2)
    many = ct.twopoint(f, [1, 3], 4., 1., 2., mpp=0.5, group_column='cluster', pairs='same')
    assert many.index.names == ['lag', 'r'] and many.index.tolist() == [(k, r) for k in (1, 3) for r in (0., 1., 2., 3.)]
    assert many['n'].tolist() == ref.n.reshape(-1).tolist() and many['n'].sum() == 16
    for name in ('dot', 'longitudinal', 'transverse'):
        yard.assert_equal_bits(many[name].values, getattr(m, name).reshape(-1), name)
    assert ct.twopoint(f, 1, 4., 1., 2., group_column='cluster', pairs='other')['n'].sum() == 0
