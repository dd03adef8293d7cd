"""Drift of a linked video on the device against the yardstick ``tests/_drift.py``:
``n_pairs`` and the stub outputs exactly, ``drift`` within the derived bound ``_drift.bound`` --
|d drift[t]| <= 2^-50 n_max (t + 1) D, n_max the largest n_pairs and D the largest absolute
displacement component of a pair: the first-order bound of reordering a sum of n doubles, twice
over and through the running sum, is below it and a logic error nine orders above -- and the
subtraction bit for bit against NumPy on the device's own drift.  The two long tables (the scan's
chunks of 256 frames, more frames than the grid has workgroups) have steps that are multiples of 1/4
and windows of one or two frames: every operation on them is exact."""
import numpy as np
import pandas as pd
import pytest

import _drift as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi

pytestmark = pytest.mark.gpu

SMOOTHINGS = (0, 1, 3)          # and T + 2, per table


def _repeated_small():
    return yard.table([[(1, (9., 9.)), (0, (0., 0.)), (0, (10., 10.))],
                       [(0, (1., 1.)), (0, (3., 5.)), (1, (9.5, 9.75))],
                       [(1, (10., 10.)), (0, (2., 2.))]])


def _repeated_across_tiles():
    """frame 0 of 2500 rows: the id of row 100 again in row 2300 (another tile of 2048 rows) and the
    id of row 5 again in row 6 (the same tile); frame 1 has every id once"""
    rng = np.random.RandomState(11)
    n = 2500
    pos = rng.uniform(0., 1000., (2 * n, 2))
    par = np.concatenate([rng.permutation(n), rng.permutation(n)]).astype(np.int64)
    par[2300], par[6] = par[100], par[5]
    return pos, np.array([0, n, 2 * n], dtype=np.int64), par


def _empty_middle():
    return yard.table([[(0, (0., 0.)), (1, (5., 5.))], [(0, (1., 0.5)), (1, (6., 5.5))], [],
                       [(1, (8., 6.)), (0, (3., 1.))], [(0, (4., 1.5)), (1, (9., 6.25))]])


TABLES = {
    'drift_2d': lambda: yard.drifting_video(0, ndim=2),
    'drift_3d': lambda: yard.drifting_video(1, ndim=3),
    'relabelled': lambda: yard.relabelled_video(2),
    'shuffled_3000': lambda: yard.shuffled_video(3),
    'empty_middle': _empty_middle,
    'one_frame': lambda: yard.table([[(0, (1., 2.)), (1, (3., 4.))]]),
    'no_rows': lambda: (np.zeros((0, 2)), np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64)),
    'no_frames': lambda: (np.zeros((0, 3)), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64)),
    'repeated_small': _repeated_small,
    'repeated_tiles': _repeated_across_tiles,
    'frames_600': lambda: yard.long_video(4, 600, 4, empty=300),         # the scan's chunks of 256 frames and their carry
    'frames_70000': lambda: yard.long_video(5, 70000, 1),               # more frames than workgroups in the grid
}
LONG = {'frames_600': (0, 2), 'frames_70000': (0,), 'repeated_tiles': (0,)}
_cache = {}


def _table(name):
    """(pos, off, par) and the yardstick's result per smoothing: computed once, never changed"""
    if name not in _cache:
        pos, off, par = TABLES[name]()
        T = len(off) - 1
        smoothings = LONG[name] if name in LONG else SMOOTHINGS + (T + 2,) if T > 1 else (0,)
        want = {s: yard.compute_drift(pos, off, par, s) for s in smoothings}
        _cache[name] = (pos, off, par, want)
    return _cache[name]


@pytest.mark.parametrize('name', sorted(TABLES))
def test_drift_equals_the_yardstick(engine, name):
    pos, off, par, wants = _table(name)
    T = len(off) - 1
    if name == 'relabelled':
        assert wants[0].n_pairs[3] == 0
    for s, want in wants.items():
        got = ct.compute_drift_arrays(pos, off, par, smoothing=s)
        assert isinstance(got.drift, np.ndarray) and got.drift.dtype == np.float64 and got.drift.shape == (T, pos.shape[1])
        assert got.n_pairs.dtype == np.int32 and got.status == _abi.DRIFT_OK
        np.testing.assert_array_equal(got.n_pairs, want.n_pairs)
        err, bound = np.abs(got.drift - want.drift), yard.bound(want, pos)
        print(name, 'smoothing', s, 'max |d drift|', err.max() if err.size else 0., 'bound at it',
              bound[err.max(1).argmax(), 0] if err.size else 0.)
        assert (err <= bound).all(), (name, s, err.max(), bound.max())
        again = ct.compute_drift_arrays(pos, off, par, smoothing=s)
        assert again.drift.tobytes() == got.drift.tobytes() and again.n_pairs.tobytes() == got.n_pairs.tobytes()
        # the subtraction: NumPy's bytes for the device's own drift
        out = ct.subtract_drift_arrays(pos, off, got.drift)
        assert isinstance(out, np.ndarray) and out.tobytes() == (pos - got.drift[yard.frame_of(off, len(pos))]).tobytes()


def test_drift_is_carried_through_a_frame_without_pairs(engine):
    pos, off, par, wants = _table('relabelled')
    got = ct.compute_drift_arrays(pos, off, par)
    assert got.n_pairs.tolist() == [0, 4, 4, 0, 4] and got.drift[3].tobytes() == got.drift[2].tobytes()
    pos, off, par, wants = _table('empty_middle')
    got = ct.compute_drift_arrays(pos, off, par)
    assert got.n_pairs.tolist() == [0, 2, 0, 0, 2]
    np.testing.assert_array_equal(got.drift, [[0., 0.], [1., 0.5], [1., 0.5], [1., 0.5], [2., 0.875]])


def test_lowest_row_of_a_repeated_id(engine):
    pos, off, par, _ = _table('repeated_small')
    got = ct.compute_drift_arrays(pos, off, par)
    assert got.n_pairs.tolist() == [0, 3, 2]
    np.testing.assert_array_equal(got.drift[1], [1.5, 2.25])       # ((1, 1) + (3, 5) + (.5, .75)) / 3


@pytest.mark.parametrize('name,threshold', [('drift_2d', 6), ('drift_2d', 1), ('shuffled_3000', 3), ('shuffled_3000', 4),
                                            ('no_rows', 1), ('repeated_tiles', 2)])
def test_stubs_equal_the_yardstick(engine, name, threshold):
    _, _, par, _ = _table(name)
    for P in (None, (int(par.max()) + 4 if len(par) else 3)):
        want = yard.filter_stubs(par, threshold, P)
        got = ct.filter_stubs_arrays(par, threshold, n_particles=P)
        assert got.particle.dtype == np.int64 and got.count.dtype == np.int32
        np.testing.assert_array_equal(got.particle, want.particle)
        np.testing.assert_array_equal(got.count, want.count)


def test_tensors_in_tensors_out(engine):
    import torch
    pos, off, par, wants = _table('drift_3d')
    host = ct.compute_drift_arrays(pos, off, par, smoothing=3)
    t_pos, t_off, t_par = (torch.from_numpy(np.array(a)).cuda() for a in (pos, off, par))
    P = int(par.max()) + 1
    for n_particles in (P, None):
        got = ct.compute_drift_arrays(t_pos, t_off, t_par, smoothing=3, n_particles=n_particles)
        assert all(torch.is_tensor(x) and x.device == t_pos.device for x in got)
        assert got.drift.cpu().numpy().tobytes() == host.drift.tobytes()
        assert got.n_pairs.cpu().numpy().tobytes() == host.n_pairs.tobytes() and int(got.status) == _abi.DRIFT_OK
    out = ct.subtract_drift_arrays(t_pos, t_off, got.drift)
    assert torch.is_tensor(out) and out.device == t_pos.device and out.data_ptr() != t_pos.data_ptr()
    assert out.cpu().numpy().tobytes() == ct.subtract_drift_arrays(pos, off, host.drift).tobytes()
    stubs = ct.filter_stubs_arrays(t_par, 6, n_particles=P)
    want = yard.filter_stubs(par, 6, P)
    assert all(torch.is_tensor(x) and x.device == t_par.device for x in stubs)
    np.testing.assert_array_equal(stubs.particle.cpu().numpy(), want.particle)
    np.testing.assert_array_equal(stubs.count.cpu().numpy(), want.count)
    # on another stream: the same bytes
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = ct.compute_drift_arrays(t_pos, t_off, t_par, smoothing=3, n_particles=P)
    s.synchronize()
    assert other.drift.cpu().numpy().tobytes() == host.drift.tobytes()
    with pytest.raises(ValueError, match='float64'):
        ct.compute_drift_arrays(t_pos.float(), t_off, t_par, n_particles=P)


def test_refused_tables(engine):
    import torch
    pos, off, par, _ = _table('drift_2d')
    falling = np.array(off)
    falling[2], falling[3] = falling[3], falling[2]
    beyond = np.array(off)
    beyond[-1] += 1
    drift = np.zeros((len(off) - 1, 2))
    for bad in (falling, beyond):
        with pytest.raises(ValueError, match='frame_offset'):
            ct.compute_drift_arrays(pos, bad, par)
        with pytest.raises(ValueError, match='frame_offset'):
            ct.subtract_drift_arrays(pos, bad, drift)
    with pytest.raises(ValueError, match='n_particles'):
        ct.compute_drift_arrays(pos, off, par, n_particles=4)
    with pytest.raises(ValueError, match='n_particles'):
        ct.filter_stubs_arrays(par, 2, n_particles=4)
    t_pos, t_par = torch.from_numpy(np.array(pos)).cuda(), torch.from_numpy(np.array(par)).cuda()
    for t_off, P in ((torch.from_numpy(falling).cuda(), 5), (torch.from_numpy(np.array(off)).cuda(), 4)):
        got = ct.compute_drift_arrays(t_pos, t_off, t_par, n_particles=P)
        assert int(got.status) == _abi.DRIFT_BAD_TABLE != 0
        assert torch.isnan(got.drift).all() and got.drift.shape == (6, 2) and not got.n_pairs.any()
    assert torch.isnan(ct.subtract_drift_arrays(t_pos, torch.from_numpy(falling).cuda(), torch.from_numpy(drift).cuda())).all()
    stubs = ct.filter_stubs_arrays(t_par, 2, n_particles=4)
    assert (stubs.particle == -1).all() and not stubs.count.any()
    # the calls after a refused one are not affected
    assert ct.compute_drift_arrays(pos, off, par).status == _abi.DRIFT_OK


def test_table_forms_equal_the_array_forms(engine):
    """non-dense particle ids and a first frame other than 0"""
    pos, off, par, wants = _table('drift_2d')
    frame = yard.frame_of(off, len(pos))
    f = pd.DataFrame({'y': pos[:, 0], 'x': pos[:, 1], 'frame': frame + 3, 'particle': (10 * par + 7).astype(np.int32),
                      'mass': np.arange(len(pos), dtype=np.float64)})
    # in a table every id is a particle: the unlinked row is a particle of one row, without a pair
    arrays = ct.compute_drift_arrays(pos, off, par, smoothing=3)
    d = ct.compute_drift(f, smoothing=3)
    assert list(d.columns) == ['y', 'x', 'n_pairs'] and d.index.tolist() == list(range(3, 9)) and d.index.name == 'frame'
    assert d[['y', 'x']].values.tobytes() == arrays.drift.tobytes() and d['n_pairs'].tolist() == arrays.n_pairs.tolist()
    shifted = ct.subtract_drift_arrays(pos, off, arrays.drift)
    for out in (ct.subtract_drift(f, smoothing=3), ct.subtract_drift(f, d)):
        assert out[['y', 'x']].values.tobytes() == shifted.tobytes() and out is not f
        assert out.drop(columns=['y', 'x']).equals(f.drop(columns=['y', 'x'])) and f['y'].values.tobytes() == pos[:, 0].tobytes()
    # rows in another order: the same table
    perm = np.random.RandomState(5).permutation(len(f))
    out = ct.subtract_drift(f.iloc[perm], d)
    assert out.index.tolist() == perm.tolist() and out.sort_index()[['y', 'x']].values.tobytes() == shifted.tobytes()
    d3 = ct.compute_drift(f.rename(columns={'frame': 't'}), pos_columns=['x', 'y'], t_column='t')
    assert list(d3.columns) == ['x', 'y', 'n_pairs']
    np.testing.assert_array_equal(d3[['y', 'x']].values, ct.compute_drift_arrays(pos, off, par).drift)
    kept = ct.filter_stubs(f, threshold=6)
    assert kept.equals(f[(par >= 0) & (par != 1)]) and len(kept) == 24
    assert ct.filter_stubs(f, threshold=1).equals(f) and len(ct.filter_stubs(f, threshold=7)) == 0


def test_chain_from_frames_to_corrected_positions(engine):
    """six Gaussians at integer centres, all shifted by (0, +1) per frame, no noise: the located
    positions are the centres, the drift is (0, t) exactly and the corrected tracks stand still"""
    import torch
    centres = np.array([(10, 8), (12, 30), (25, 18), (40, 9), (45, 40), (55, 24)])
    frames = np.zeros((8, 64, 64), dtype=np.uint8)
    for t in range(8):
        for y, x in centres:
            ct.artificial.draw_gaussian(frames[t], (y, x + t), 1.5, 200)
    r = ct.find_link_arrays(torch.from_numpy(frames).cuda(), search_range=4, separation=5, diameter=5, minmass=100,
                            _on_device=True)
    off = r.frame_offset.cpu().numpy()
    located = r.pos.cpu().numpy()
    assert np.diff(off).tolist() == [6] * 8
    for t in range(8):
        rows = located[off[t]:off[t + 1]]
        np.testing.assert_array_equal(rows[np.lexsort(rows.T[::-1])], centres + [0, t])
    P = int(r.n_tracks)
    assert P == 6
    stubs = ct.filter_stubs_arrays(r.particle, threshold=8, n_particles=P)
    assert (stubs.count == 8).all() and torch.equal(stubs.particle, r.particle)
    res = ct.compute_drift_arrays(r.pos, r.frame_offset, stubs.particle, n_particles=P)
    assert all(torch.is_tensor(x) for x in res) and int(res.status) == 0
    np.testing.assert_array_equal(res.n_pairs.cpu().numpy(), [0] + [6] * 7)
    np.testing.assert_array_equal(res.drift.cpu().numpy(), np.stack([np.zeros(8), np.arange(8.)], 1))
    fixed = ct.subtract_drift_arrays(r.pos, r.frame_offset, res.drift).cpu().numpy()
    particle = r.particle.cpu().numpy()
    for p in range(P):
        rows = fixed[particle == p]
        assert len(rows) == 8 and (rows == rows[0]).all()
    assert sorted(map(tuple, fixed[particle.argsort(kind='stable')][::8].tolist())) == sorted(map(tuple, centres.tolist()))
