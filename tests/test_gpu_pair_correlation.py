"""Pair correlation function g(r) on the device against the yardstick
``tests/_pair_correlation.py``.  ``count``, ``n_ref``, ``n_rows`` and ``r_edges`` are exact in every mode;
``weight``, ``g_frame`` and ``g`` are the yardstick's bytes for ``edge='none'`` and ``'interior'`` (no
trigonometry, every operation in a pinned order).  For ``'arc'``: ``weight`` within ``n_ref[t] * 1e-14``
-- asin and acos good to 2 ulp each make a quadrant angle good to about 5 ulp of pi / 2, four of them
divided by 2 pi under 1e-15 per row, times a margin of ten -- and ``g_frame`` and ``g`` within the
relative error which that implies for their denominators, plus the roundings of the two products,
the division and, for ``g``, of the T additions (2^-53 each).  The cases stand on the edges of the
launch: the tile of 256 rows on the reference side and on the neighbour side, frames without a work
item, one bin and ``_abi.PCF_MAX_BINS`` of them, pairs exactly on a bin edge."""
import numpy as np
import pandas as pd
import pytest

import _pair_correlation as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi

pytestmark = pytest.mark.gpu

U = 2. ** -53


def _walls_then_middle():
    """frame 0 has every row within 5 of a wall of the box [0, 30]^2 (no interior row at cutoff 10),
    frame 1 rows in the middle too, frame 2 one row"""
    rng = np.random.RandomState(8)
    ring = rng.uniform(0., 5., (40, 2))
    ring[::2] = 30. - ring[::2]
    return yard.table([ring, rng.uniform(0., 30., (300, 2)), [[15., 15.]]])


def _mixed():
    """NaN rows, an infinite one, coincident rows, rows outside the given boundary"""
    pos, off = yard.uniform_frames(4, (30, 0, 45), (20., 16.))
    pos[2] = np.nan
    pos[7, 1] = np.nan
    pos[9, 0] = np.inf
    pos[11] = pos[12] = pos[13]
    pos[40] = pos[3]                      # equal rows of different frames are no pair
    pos[50] = (25., 3.)                   # outside
    pos[51] = (-1., 3.)
    return pos, off


def _groups(n, seed=6, low=-3, high=12):
    return np.random.RandomState(seed).randint(low, high, n).astype(np.int64)


def _3d():
    return yard.uniform_frames(5, (120, 1, 300), (12., 20., 40.), 3)


_tile, _lat, _mix, _wm, _vol = yard.tile_edges(), yard.lattice(20, 20, 2), _mixed(), _walls_then_middle(), _3d()
_dim = yard.dimers(1, 300)
BOX = [[0., 0.], [20., 16.]]
# name: (pos, frame_offset, keywords)
CASES = {
    'tile_none': _tile + (dict(cutoff=10., dr=0.5, edge='none'),),
    'tile_interior': _tile + (dict(cutoff=10., dr=0.5, edge='interior'),),
    'tile_arc': _tile + (dict(cutoff=10., dr=0.5, edge='arc'),),
    'tile_arc_boundary_mpp': _tile + (dict(cutoff=3., dr=0.125, edge='arc', mpp=(0.25, 0.5), boundary=[[-2., 0.], [61., 45.5]]),),
    'tile_groups_same': _tile + (dict(cutoff=10., dr=0.5, edge='arc', group=_groups(len(_tile[0])), pairs='same'),),
    'tile_groups_other': _tile + (dict(cutoff=10., dr=0.5, edge='arc', group=_groups(len(_tile[0])), pairs='other'),),
    'tile_groups_all': _tile + (dict(cutoff=10., dr=0.5, edge='arc', group=_groups(len(_tile[0])), pairs='all'),),
    'no_frames': (np.zeros((0, 2)), np.zeros(1, dtype=np.int64), dict(cutoff=4., dr=0.5, edge='arc')),
    'one_frame_no_rows': (np.zeros((0, 3)), np.zeros(2, dtype=np.int64), dict(cutoff=4., dr=0.5, edge='none')),
    'one_bin': _tile + (dict(cutoff=3., dr=3., edge='arc'),),
    'bins_at_the_cap': _wm + (dict(cutoff=64., dr=2. ** -5, edge='arc'),),
    'cutoff_no_multiple_of_dr': _wm + (dict(cutoff=10.2, dr=0.5, edge='none'),),
    'lattice_none': _lat + (dict(cutoff=5., dr=1., edge='none'),),
    'lattice_interior': _lat + (dict(cutoff=5., dr=1., edge='interior'),),
    'lattice_arc': _lat + (dict(cutoff=5., dr=1., edge='arc'),),
    'mixed_none': _mix + (dict(cutoff=6., dr=0.5, edge='none', boundary=BOX),),
    'mixed_arc': _mix + (dict(cutoff=6., dr=0.5, edge='arc', boundary=BOX),),
    'mixed_interior_default_box': _mix + (dict(cutoff=2., dr=0.25, edge='interior'),),
    'volume_none': _vol + (dict(cutoff=6., dr=0.5, edge='none', mpp=(2., 1., 0.5)),),
    'volume_interior': _vol + (dict(cutoff=4., dr=0.5, edge='interior', mpp=(2., 1., 0.5)),),
    'no_interior_row': _wm + (dict(cutoff=10., dr=1., edge='interior', boundary=[[0., 0.], [30., 30.]]),),
    'all_rows_equal': (np.full((6, 2), 3.5), np.array([0, 4, 6]), dict(cutoff=2., dr=0.5, edge='arc')),
    'dimers_same': _dim[:2] + (dict(cutoff=10., dr=0.5, edge='arc', group=_dim[2], pairs='same'),),
    'dimers_other': _dim[:2] + (dict(cutoff=10., dr=0.5, edge='none', group=_dim[2], pairs='other'),),
}
_want = {}


def want(name):
    """the yardstick's result, computed once and never changed"""
    if name not in _want:
        pos, off, kw = CASES[name]
        _want[name] = yard.pair_correlation(pos, off, **kw)
    return _want[name]


def compare(got, ref, edge, what):
    for name in ('count', 'n_ref', 'n_rows'):
        assert getattr(got, name).dtype == np.int64 and getattr(got, name).shape == getattr(ref, name).shape, (what, name)
        assert (getattr(got, name) == getattr(ref, name)).all(), (what, name)
    assert got.r_edges.tobytes() == ref.r_edges.tobytes(), what
    if edge != 'arc':
        for name in ('weight', 'g_frame', 'g'):
            yard.assert_equal_bits(getattr(got, name), getattr(ref, name), (what, name))
        return 0.
    T = len(ref.n_ref)
    assert got.weight.shape == ref.weight.shape and not np.isnan(got.weight).any()
    err = np.abs(got.weight - ref.weight)
    worst = float((err / np.maximum(ref.n_ref[:, None], 1)).max()) if err.size else 0.
    print(what, 'largest |weight - yardstick| / n_ref = %.3g' % worst)
    assert (err <= ref.n_ref[:, None] * 1e-14).all(), (what, worst)
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.where(ref.weight > 0, ref.n_ref[:, None] * 1e-14 / ref.weight, 0.)
    for name, bound in (('g_frame', rel + 4 * U), ('g', (rel.max(0) if T else np.zeros(len(ref.g))) + (T + 4) * U)):
        g, w = getattr(got, name), getattr(ref, name)
        assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (what, name)
        ok = np.isnan(w) | (np.abs(g - w) <= bound * np.abs(w))
        assert ok.all(), (what, name, np.argwhere(~ok)[:5])
    return worst


@pytest.mark.parametrize('name', sorted(CASES))
def test_cases_against_the_yardstick(engine, name):
    pos, off, kw = CASES[name]
    got = ct.pair_correlation_arrays(pos, off, **kw)
    assert isinstance(got.g, np.ndarray) and got.status == _abi.PCF_OK
    compare(got, want(name), kw['edge'], name)


def test_the_cases_hold_their_edges():
    """what the cases are there for, asserted on the yardstick"""
    assert np.diff(_tile[1]).tolist() == [0, 1, 2, 255, 256, 257, 513]
    t = want('tile_none')
    assert t.n_rows.tolist() == [0, 1, 2, 255, 256, 257, 513] and np.isnan(t.g_frame[:2]).all() and not np.isnan(t.g_frame[2:]).any()
    ti = want('tile_interior')
    assert (ti.n_ref[3:] > 0).all() and (ti.n_ref[3:] < ti.n_rows[3:]).all()
    assert len(want('one_bin').g) == 1 and len(want('bins_at_the_cap').g) == _abi.PCF_MAX_BINS
    assert len(want('cutoff_no_multiple_of_dr').g) == 21
    assert want('no_frames').g_frame.shape == (0, 8) and np.isnan(want('no_frames').g).all()
    assert want('one_frame_no_rows').n_rows.tolist() == [0] and np.isnan(want('one_frame_no_rows').g).all()
    # the lattice: pairs on every edge 1 .. 4 in the upper bin, those at 5 = r_edges[B] in none
    lat = want('lattice_interior')
    assert lat.n_ref.tolist() == [100, 100] and lat.count[0].tolist() == [0, 800, 1600, 2000, 2400]
    mixed = want('mixed_none')
    assert mixed.n_rows.tolist() == [27, 0, 43] and mixed.count[0, 0] >= 6          # three coincident rows: six ordered pairs
    assert want('mixed_interior_default_box').n_ref.sum() > 0
    vol = want('volume_interior')
    assert vol.n_ref[0] > 0 and vol.n_ref[1] == 0 and not np.isnan(vol.g).any()
    inner = want('no_interior_row')
    assert inner.n_ref[0] == 0 and inner.n_rows[0] == 40 and np.isnan(inner.g_frame[0]).all() and np.isnan(inner.g_frame[2]).all()
    yard.assert_equal_bits(inner.g, inner.g_frame[1])                             # the pool skips the NaN frames
    eq = want('all_rows_equal')
    assert eq.count[:, 0].tolist() == [12, 2] and np.isnan(eq.g).all() and np.isnan(eq.g_frame).all()
    parts = [want('tile_groups_' + p).count for p in ('all', 'same', 'other')]
    assert (parts[0] == parts[1] + parts[2]).all() and parts[1].sum() > 0 and (_groups(len(_tile[0])) < 0).any()
    assert (parts[0] == want('tile_arc').count).all()
    same = want('dimers_same')
    assert same.count[0, 8] == 600 and same.count.sum() == 600 and want('dimers_other').count[0, :20].sum() == 0


def test_counts_of_same_and_other_add_up_on_the_device(engine):
    got = {}
    for p in ('all', 'same', 'other'):
        pos, off, kw = CASES['tile_groups_' + p]
        got[p] = ct.pair_correlation_arrays(pos, off, **kw).count
    assert (got['all'] == got['same'] + got['other']).all()
    pos, off, kw = CASES['dimers_same']
    same = ct.pair_correlation_arrays(pos, off, **kw)
    assert same.count[0, 8] == 600 and same.count.sum() == 600


def test_tensors_in_tensors_out_and_a_bad_table(engine):
    import torch
    pos, off, kw = CASES['tile_groups_same']
    ref = want('tile_groups_same')
    t_pos, t_off = torch.from_numpy(pos).cuda(), torch.from_numpy(off).cuda()
    t_kw = dict(kw, group=torch.from_numpy(kw['group']).cuda())
    first = None
    for _ in range(2):                           # two calls: the same bytes
        got = ct.pair_correlation_arrays(t_pos, t_off, **t_kw)
        assert all(torch.is_tensor(x) and x.device == t_pos.device for x in got)
        assert got.status.dtype == torch.int32 and got.status.shape == (1,) and int(got.status) == _abi.PCF_OK
        assert got.count.dtype == got.n_ref.dtype == got.n_rows.dtype == torch.int64
        host = ct.static.PairCorrelation(*(x.cpu().numpy() for x in got))
        compare(host, ref, 'arc', 'tensors')
        blob = b''.join(x.tobytes() for x in host)
        first = first or blob
        assert blob == first
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = ct.pair_correlation_arrays(t_pos, t_off, **t_kw)
    s.synchronize()
    assert b''.join(x.cpu().numpy().tobytes() for x in other) == first
    # the same bytes from ndarrays
    again = ct.pair_correlation_arrays(pos, off, **kw)
    assert b''.join(np.asarray(x).tobytes() for x in again[:-1]) == first[:-4]
    for bad in ([0, 5, 3, len(pos)], [0, 3, 3, len(pos) + 1], [-1, 3, 4, 4]):
        b_off = np.array(bad, dtype=np.int64)
        res = ct.pair_correlation_arrays(t_pos, torch.from_numpy(b_off).cuda(), **t_kw)
        assert int(res.status) == _abi.PCF_BAD_TABLE
        assert res.g.isnan().all() and res.g_frame.isnan().all() and res.weight.isnan().all()
        assert not res.count.any() and not res.n_ref.any() and not res.n_rows.any() and res.g_frame.shape == (3, 20)
        with pytest.raises(ValueError, match='frame_offset'):
            ct.pair_correlation_arrays(pos, b_off, **kw)
    with pytest.raises(ValueError, match='float64'):
        ct.pair_correlation_arrays(t_pos.float(), t_off, 4.)
    with pytest.raises(ValueError, match='int64'):
        ct.pair_correlation_arrays(t_pos, t_off, 4., group=t_kw['group'].int(), pairs='same')


def test_scratch_grows_and_comes_back(engine):
    """a small call, a large one (one frame of 3000 rows: twelve work items and their partial weights),
    the small one again: the first bytes"""
    pos, off, kw = CASES['mixed_arc']
    big_pos, big_off = yard.uniform_frames(12, (3000,), (300., 200.))
    first = ct.pair_correlation_arrays(pos, off, **kw)
    grown = ct.pair_correlation_arrays(big_pos, big_off, 40., 0.5, edge='arc')
    last = ct.pair_correlation_arrays(pos, off, **kw)
    for a, b in zip(first[:-1], last[:-1]):
        assert a.tobytes() == b.tobytes()
    compare(first, want('mixed_arc'), 'arc', 'first')
    compare(grown, yard.pair_correlation(big_pos, big_off, 40., 0.5, edge='arc'), 'arc', 'grown')


def test_table_form(engine):
    """a shuffled DataFrame with a frame gap and a first frame other than 0; no particle column"""
    pos, off, kw = CASES['mixed_arc']
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    f = pd.DataFrame({'y': pos[:, 0], 'x': pos[:, 1], 'frame': (frame + 5).astype(np.int32)})
    f = f.iloc[np.random.RandomState(1).permutation(len(f))]
    order = np.argsort(f['frame'].values, kind='stable')
    s_pos = f[['y', 'x']].values[order]
    arrays = ct.pair_correlation_arrays(s_pos, off, **kw)
    r_edges, g = ct.pair_correlation(f, kw['cutoff'], kw['dr'], boundary=kw['boundary'], edge='arc')
    assert r_edges.tobytes() == arrays.r_edges.tobytes() and g.tobytes() == arrays.g.tobytes()
    compare(arrays, want('mixed_arc'), 'arc', 'shuffled')        # the counts do not depend on the row order
    r_edges, per = ct.pair_correlation(f, kw['cutoff'], kw['dr'], boundary=kw['boundary'], edge='arc', per_frame=True)
    assert per.index.tolist() == [5, 6, 7] and per.index.name == 'frame' and per.columns.tolist() == r_edges[:-1].tolist()
    assert per.values.tobytes() == arrays.g_frame.tobytes() and per.loc[6].isna().all()
    # the labels of find_clusters as groups: pairs inside a cluster are nearer than the separation
    pos, off = _wm
    clean = pd.DataFrame({'y': pos[:, 0], 'x': pos[:, 1], 'frame': np.repeat(np.arange(len(off) - 1), np.diff(off))})
    labelled = ct.find_clusters(clean, 1.5)
    assert 'cluster' in labelled and labelled['cluster'].values.dtype.kind in 'iu'
    r_edges, same = ct.pair_correlation(labelled, 6., 0.5, boundary=kw['boundary'], edge='none', group_column='cluster', pairs='same',
                                        per_frame=True)
    r_edges, other = ct.pair_correlation(labelled, 6., 0.5, boundary=kw['boundary'], edge='none', group_column='cluster', pairs='other',
                                         per_frame=True)
    r_edges, both = ct.pair_correlation(labelled, 6., 0.5, boundary=kw['boundary'], edge='none', per_frame=True)
    assert np.nansum(same.values[:, :3]) > 0 and np.nansum(other.values[:, :3]) == 0       # r < 1.5
    np.testing.assert_allclose(np.nan_to_num(same.values + other.values), np.nan_to_num(both.values), rtol=4 * U, atol=0)


def test_chain_from_located_tensors(engine):
    """the tensors of find_link_arrays go in as they are: six Gaussians at integer centres in every frame"""
    import torch
    centres = np.array([(10, 8), (10, 14), (25, 18), (40, 9), (45, 40), (55, 24)])
    frames = np.zeros((4, 64, 64), dtype=np.uint8)
    for t in range(4):
        for y, x in centres:
            ct.artificial.draw_gaussian(frames[t], (y, x), 1.5, 200)
    r = ct.find_link_arrays(torch.from_numpy(frames).cuda(), search_range=4, separation=5, diameter=5, minmass=100, _on_device=True)
    res = ct.pair_correlation_arrays(r.pos, r.frame_offset, 10., 1., boundary=[[0., 0.], [64., 64.]], edge='arc')
    assert all(torch.is_tensor(x) for x in res) and int(res.status) == 0
    count = res.count.cpu().numpy()
    assert count.shape == (4, 10) and (count[:, 6] == 2).all() and (count.sum(1) == 2).all()      # the pair at distance 6
    ref = yard.pair_correlation(r.pos.cpu().numpy(), r.frame_offset.cpu().numpy(), 10., 1., boundary=[[0., 0.], [64., 64.]], edge='arc')
    compare(ct.static.PairCorrelation(*(x.cpu().numpy() for x in res)), ref, 'arc', 'chain')
