"""Van Hove displacement distributions on the device against the yardstick
``tests/_vanhove.py``.  The exact tables (steps that are multiples of 1/4, mpp a power of two: every
sum of d, d^2 and d^4 is exact in any order) must equal it bit for bit -- counts, tails, the three
means, alpha2 and the densities -- on the edges of the launch: three chunks of ids of which the last
holds one, a track of more than two strides of the workgroup, a gap, a repeated row and an unlinked
row, one lag, several and one beyond every span, H = 1 and H = 1024.  Displacements on, just below
and just above every edge go where the comparison with the host's edges puts them.  On rounded tables
the counts stay exact, ``mean_d`` and ``mean_d2`` are the bytes of ``emsd_arrays`` and ``mean_d4`` stays
within the derived bound ``_vanhove.bound_d4``."""
import numpy as np
import pandas as pd
import pytest

import _msd
import _vanhove as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi

pytestmark = pytest.mark.gpu

CHUNK = _abi.MSD_CHUNK


def _mixed(ndim):
    """T = 6: a gap, a track of one row, an id without rows (3), a repeated id, unlinked rows"""
    tracks = [[0, 1, 4, 5], [2], [0, 1, 2, 3, 4], [], [1, 2, 3, 4, 5], [4, 5]]
    return _msd.exact_tracks(3 + ndim, tracks, n_frames=6, ndim=ndim, extra=[(1, 2), (2, -1), (3, -5), (4, 0), (4, -1)])


def _long(ndim):
    """one track of 600 rows: more than two strides of 256, with a gap and a repeated row behind which
    row i + k is not the partner, and an unlinked row"""
    return _msd.exact_tracks(20 + ndim, [_msd.span_with_gap(0, 605, (300, 305))], ndim=ndim, extra=[(150, 0), (151, -1)])


# name: (table, mpp, lags, bin_width, max_disp)
EXACT = {
    'chunks_2d': (lambda: _msd.exact_tracks(11, [[0, 1, 2]] * (2 * CHUNK + 1)), 0.5, [1, 2, 7], 0.25, 1.),     # H = 4; lag 7 beyond every span
    'chunks_3d_one_lag': (lambda: _msd.exact_tracks(12, [[0, 1, 2]] * (2 * CHUNK + 1), ndim=3), (0.5, 1., 4.), [1], 0.5, 3.),
    'long_2d_h1': (lambda: _long(2), 0.5, [1], 2., 2.),                                               # H = 1
    'long_3d_h1024': (lambda: _long(3), (0.5, 1., 4.), [1, 3, 7], 0.03125, 32.),                      # H = 1024
    'long_2d': (lambda: _long(2), 2., [1, 3, 7], 0.75, 5.),                                           # tails in use
    'mixed_2d': (lambda: _mixed(2), 0.5, [1, 3, 7], 0.25, 1.5),
    'mixed_3d': (lambda: _mixed(3), (0.5, 1., 4.), [1, 3, 7], 0.125, 128.),                           # H = 1024
    'mixed_3d_one_lag': (lambda: _mixed(3), (0.5, 1., 4.), [1], 1., 1.),                              # H = 1
    'beyond': (lambda: _mixed(2), 1., [6], 0.5, 2.),                                                  # one lag, beyond every span
    'no_rows': (lambda: (np.zeros((0, 2)), np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64)), 1., [1, 2], 0.5, 2.),
    'unlinked_only': (lambda: _msd.table([[(-1, (0., 0.)), (-2, (1., 1.))], [(-1, (0.5, 0.)), (-2, (1., 2.))]]), 1., [1], 0.5, 2.),
}
ROUNDED = {
    'jitter_2d': (lambda: _msd.jittered_video(0, ndim=2), 0.16, [1, 2, 5], 0.01, 0.2),
    'jitter_3d': (lambda: _msd.jittered_video(1, ndim=3), (0.21, 0.16, 0.16), [1, 3], 0.02, 0.25),
}
_cache = {}


def _table(name):
    """(pos, off, par, mpp, lags, bin_width, max_disp, the yardstick's Result): computed once, never changed"""
    if name not in _cache:
        make, mpp, lags, width, reach = (EXACT.get(name) or ROUNDED[name])
        pos, off, par = make()
        _cache[name] = (pos, off, par, mpp, lags, width, reach, yard.vanhove(pos, off, par, lags, width, reach, mpp))
    return _cache[name]


@pytest.mark.parametrize('name', sorted(EXACT))
def test_exact_tables_equal_the_yardstick_bit_for_bit(engine, name):
    pos, off, par, mpp, lags, width, reach, want = _table(name)
    got = ct.vanhove_arrays(pos, off, par, lags if len(lags) > 1 else lags[0], width, reach, mpp)
    assert isinstance(got.count, np.ndarray) and got.status == _abi.VANHOVE_OK
    yard.assert_equal_bits(got, want, name)
    # clause 7 on finite positions
    assert (got.count.sum(-1) + got.below + got.above == got.n[:, None]).all()
    assert (got.count_r.sum(-1) + got.above_r == got.n).all()


def test_the_exact_tables_hold_what_they_are_for(engine):
    want = _table('chunks_2d')[7]
    P = 2 * CHUNK + 1
    assert want.n.tolist() == [2 * P, P, 0] and np.isnan(want.density[2]).all() and np.isnan(want.alpha2[2]).all()
    # |d| <= 1 at lag 1, where -1 is edges[0] (bin 0) and +1 is edges[2H] (above); up to 2 at lag 2
    assert want.count.shape == (3, 2, 8) and want.below[0].sum() == 0 and want.below[1].sum() > 0 and want.above[:2].sum(-1).min() > 0
    pos, off, par, _, _, _, _, want = _table('long_2d')
    tracks = _msd.tracks_of(off, par)
    assert len(tracks[0]) == 600 and (par == 0).sum() == 601 and (par < 0).sum() == 1
    assert want.n.tolist() == [598, 594, 588] and want.above_r.min() > 0
    assert want.below[1:].sum(-1).min() > 0 and want.above[1:].sum(-1).min() > 0 and not want.below[0].any()
    assert _table('long_2d_h1')[7].count.shape == (1, 2, 2) and _table('long_3d_h1024')[7].count.shape == (3, 3, 2048)
    assert _table('long_3d_h1024')[7].above[:2].sum() == 0 and _table('mixed_3d')[7].count_r.shape == (3, 1024)
    assert _table('mixed_2d')[7].n.tolist() == [11, 5, 0] and _table('beyond')[7].n.tolist() == [0]
    assert _table('unlinked_only')[7].n.tolist() == [0] and _table('no_rows')[7].n.tolist() == [0, 0]


@pytest.mark.parametrize('reach', [0.35, 25.55, 102.4], ids=['H4', 'H256', 'H1024'])
def test_displacements_on_and_next_to_every_edge(engine, reach):
    """bin_width = 0.1 is no double, so floor(d / 0.1) and the comparison with (b - H) * 0.1 disagree at
    some edges; the displacements are exactly edges[b], the doubles next to it on either side, -0.0 and
    a NaN.  The pair moves along axis 0 only: d2 = d * d is edge2[|b - H|] where d is an edge."""
    width = 0.1
    half, edges, r_edges, edge2 = yard.bins(width, reach)
    assert half == {0.35: 4, 25.55: 256, 102.4: 1024}[reach] and edges[half] == 0.
    ds = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [-0., np.nan]])
    guess = np.floor(edges[1:-1] / width).astype(int) + half
    assert reach == 0.35 or (guess != np.arange(1, 2 * half)).any()         # the division alone would misplace an edge
    n = len(ds)
    pos = np.zeros((2 * n, 2))
    pos[n:, 0] = ds
    off, par = np.array([0, n, 2 * n]), np.tile(np.arange(n), 2)
    got = ct.vanhove_arrays(pos, off, par, 1, width, reach)
    want = yard.vanhove(pos, off, par, [1], width, reach)
    yard.assert_counts(got, want, reach)
    B = 2 * half
    # bin b holds edges[b], the double above it and the double below edges[b + 1]; bin H also -0.0
    expect = np.full(B, 3)
    expect[half] += 1
    assert got.n[0] == n and (got.count[0, 0] == expect).all()
    assert got.below[0, 0] == 1 and got.above[0, 0] == 2                     # below edges[0]; edges[2H] and above it
    assert got.count[0, 0].sum() + got.below[0, 0] + got.above[0, 0] == n - 1         # the NaN: in n and in no bin
    assert got.count[0, 1, half] == n and got.count[0, 1].sum() == n          # axis 1 stands still: 0.0 is in bin H
    # radial: d2 == edge2[b] is in bin b, d2 == edge2[H] in above_r; the NaN nowhere
    d2 = ds * ds
    finite = ~np.isnan(d2)
    assert got.above_r[0] == (d2[finite] >= edge2[half]).sum() >= 4 and got.count_r[0].sum() + got.above_r[0] == n - 1
    for b in (0, 1, half - 1):
        assert got.count_r[0, b] == ((d2[finite] >= edge2[b]) & (d2[finite] < edge2[b + 1])).sum() >= 2
    assert np.isnan(got.mean_d[0, 0]) and got.mean_d[0, 1] == 0.


@pytest.mark.parametrize('name', sorted(ROUNDED))
def test_conservation_and_rounded_tables(engine, name):
    """clause 7 on finite jittered positions; the counts equal the yardstick's; mean_d4 within (n + 3)
    max|d|^4 2^-53 of the fsum restatement (mean_d and mean_d2 within _msd.bound's (n + 3) X 2^-53:
    their fused sums round once where the plain sums round twice); alpha2 is clause 9 on the returned means"""
    pos, off, par, mpp, lags, width, reach, want = _table(name)
    got = ct.vanhove_arrays(pos, off, par, lags, width, reach, mpp)
    assert np.isfinite(pos).all() and (got.n > 0).all()
    assert (got.count.sum(-1) + got.below + got.above == got.n[:, None]).all()
    assert (got.count_r.sum(-1) + got.above_r == got.n).all()
    assert got.above.sum() > 0 and got.above_r.sum() > 0 and got.count.sum() > 0
    yard.assert_counts(got, want, name)
    for what, lim in (('mean_d', (want.n[:, None] + 3.) * want.max_d * yard.U),
                      ('mean_d2', (want.n[:, None] + 3.) * want.max_d ** 2 * yard.U), ('mean_d4', yard.bound_d4(want))):
        err = np.abs(getattr(got, what) - getattr(want, what))
        print(name, what, 'max error', err.max(), 'bound there', lim.reshape(-1)[err.argmax()])
        assert (err <= lim).all(), (name, what, err.max())
    assert yard.same_floats(got.alpha2, yard.alpha2_of(got.mean_d2, got.mean_d4))
    assert yard.same_floats(got.density, got.count / (got.n * width)[:, None, None])
    assert yard.same_floats(got.density_r, got.count_r / (got.n * width)[:, None])


def test_every_pair_in_one_bin(engine):
    """tracks at rest: every pair of every lag adds to the same LDS counter of its workgroup and the same
    int64 cell; 2000 tracks of 50 frames, 8 chunks"""
    P, T = 2000, 50
    rng = np.random.RandomState(5)
    pos = np.tile(rng.uniform(0., 100., (P, 3)), (T, 1))
    off, par = np.arange(T + 1) * P, np.tile(np.arange(P), T)
    lags = [1, 7, 49, 50]
    got = ct.vanhove_arrays(pos, off, par, lags, 0.1, 0.8, mpp=(0.5, 0.25, 1.))
    assert got.n.tolist() == [P * (T - k) for k in lags] and got.n[3] == 0
    assert (got.count[:, :, 8] == got.n[:, None]).all() and (got.count.sum(-1) == got.n[:, None]).all()
    assert (got.count_r[:, 0] == got.n).all() and not got.below.any() and not got.above.any() and not got.above_r.any()
    assert (got.mean_d[:3] == 0.).all() and (got.mean_d4[:3] == 0.).all() and np.isnan(got.alpha2).all()      # 0 / 0
    assert (got.density[:3, :, 8] == 1. / 0.1).all() and np.isnan(got.density[3]).all()


def test_mean_d_and_mean_d2_are_the_bytes_of_emsd(engine):
    """clause 8's ordering promise on a table whose sums round: 300 ids (two chunks) in 8 frames"""
    pos, off, par = _msd.jittered_video(7, n_frames=8, n_particles=300, ndim=3, absent=(17, 4))
    mpp, lags = (0.21, 0.16, 0.16), [1, 3, 7, 8]
    got = ct.vanhove_arrays(pos, off, par, lags, 0.02, 0.5, mpp)
    ens = ct.emsd_arrays(pos, off, par, 8, mpp)
    rows = [k - 1 for k in lags]
    assert (got.n == ens.n[rows]).all() and got.n[3] == 0 and got.n[0] == 7 * 300 - 2
    assert got.mean_d.tobytes() == ens.mean_d[rows].tobytes() and got.mean_d2.tobytes() == ens.mean_d2[rows].tobytes()
    alone = ct.vanhove_arrays(pos, off, par, 3, 0.02, 0.5, mpp)              # a lag alone: the bytes of the batch
    for name in yard.FLOATS + yard.COUNTS:
        assert np.asarray(getattr(alone, name))[0].tobytes() == np.asarray(getattr(got, name))[1].tobytes(), name


def test_refused_tables(engine):
    import torch
    pos, off, par, mpp, lags, width, reach, want = _table('mixed_2d')
    falling = np.array(off)
    falling[2], falling[3] = falling[3] + 1, falling[2]
    beyond = np.array(off)
    beyond[-1] += 1
    P = int(par.max()) + 1
    for bad in (falling, beyond):
        with pytest.raises(ValueError, match='frame_offset'):
            ct.vanhove_arrays(pos, bad, par, lags, width, reach, mpp)
    with pytest.raises(ValueError, match='n_particles'):
        ct.vanhove_arrays(pos, off, par, lags, width, reach, mpp, n_particles=P - 1)
    t_pos, t_par = torch.from_numpy(np.array(pos)).cuda(), torch.from_numpy(np.array(par)).cuda()
    for t_off, n_particles in ((torch.from_numpy(falling).cuda(), P), (torch.from_numpy(np.array(off)).cuda(), P - 1)):
        res = ct.vanhove_arrays(t_pos, t_off, t_par, lags, width, reach, mpp, n_particles=n_particles)
        assert int(res.status) == _abi.VANHOVE_BAD_TABLE != 0 and tuple(res.count.shape) == want.count.shape
        for name in yard.FLOATS:
            assert torch.isnan(getattr(res, name)).all(), name
        for name in yard.COUNTS:
            assert not getattr(res, name).any(), name
    # the same call after the refused ones
    yard.assert_equal_bits(ct.vanhove_arrays(pos, off, par, lags, width, reach, mpp), want, 'after')


def test_tensors_in_tensors_out_and_repeatable(engine):
    import torch
    pos, off, par, mpp, lags, width, reach, want = _table('jitter_3d')
    host = ct.vanhove_arrays(pos, off, par, lags, width, reach, mpp)
    again = ct.vanhove_arrays(pos, off, par, lags, width, reach, mpp)
    names = ('lags', 'edges', 'r_edges') + yard.COUNTS + yard.FLOATS
    for name in names:
        assert getattr(host, name).tobytes() == getattr(again, name).tobytes(), name
    t_pos, t_off, t_par = (torch.from_numpy(np.array(a)).cuda() for a in (pos, off, par))
    P = int(par.max()) + 1
    for n_particles in (P, None):
        res = ct.vanhove_arrays(t_pos, t_off, t_par, lags, width, reach, mpp, n_particles=n_particles)
        assert all(torch.is_tensor(x) and x.device == t_pos.device for x in res)
        assert res.status.dtype == torch.int32 and tuple(res.status.shape) == (1,) and int(res.status) == _abi.VANHOVE_OK
        assert res.count.dtype == torch.int64 and res.n.dtype == torch.int64 and res.lags.dtype == torch.int64
        for name in names:
            assert getattr(res, name).cpu().numpy().tobytes() == getattr(host, name).tobytes(), name
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = ct.vanhove_arrays(t_pos, t_off, t_par, lags, width, reach, mpp, n_particles=P)
    s.synchronize()
    assert other.density.cpu().numpy().tobytes() == host.density.tobytes()
    with pytest.raises(ValueError, match='float64'):
        ct.vanhove_arrays(t_pos.float(), t_off, t_par, 1, width, reach, n_particles=P)


def test_scratch_grows_and_the_msd_after_it_still_holds(engine):
    """a small msd call, a van Hove call that needs more of the shared block (more rows, more ids, 64
    lags of partials), then msd again: its own yardstick's bytes"""
    pos, off, par = _mixed(3)
    mpp = (0.5, 1., 4.)
    want = _msd.msd(pos, off, par, 5, mpp)
    _msd.assert_equal_bits(ct.msd_arrays(pos, off, par, 5, mpp), want, 'before')
    big = _table('chunks_2d')
    lags = list(range(1, 65))
    grown = ct.vanhove_arrays(big[0], big[1], big[2], lags, big[5], big[6], big[3])
    assert grown.count.shape == (64, 2, 8) and (grown.n[2:] == 0).all()
    for name in yard.COUNTS + yard.FLOATS:
        assert yard.same_floats(getattr(grown, name)[:2].astype(np.float64), getattr(big[7], name)[:2].astype(np.float64)), name
    assert np.isnan(grown.mean_d[2:]).all() and not grown.count[2:].any()
    _msd.assert_equal_bits(ct.msd_arrays(pos, off, par, 5, mpp), want, 'after')
    _msd.assert_equal_bits(ct.emsd_arrays(pos, off, par, 5, mpp), _msd.emsd(pos, off, par, 5, mpp), 'ensemble after')
    yard.assert_equal_bits(ct.vanhove_arrays(*_table('mixed_3d')[:3], [1, 3, 7], 0.125, 128., mpp), _table('mixed_3d')[7], 'small again')


def test_table_form(engine):
    """non-dense particle ids, a first frame other than 0, rows in another order"""
    pos, off, par, mpp, lags, width, reach, want = _table('jitter_2d')
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    f = pd.DataFrame({'y': pos[:, 0], 'x': pos[:, 1], 'frame': frame + 3, 'particle': (10 * par + 7).astype(np.int32)})
    ids, dense = np.unique(f['particle'].values, return_inverse=True)         # the unlinked row (-3) is a particle of one row
    arrays = ct.vanhove_arrays(pos, off, dense, 2, width, reach, mpp)
    table = ct.vanhove(f.iloc[np.random.RandomState(0).permutation(len(f))], 2, mpp, width, reach)       # rows in another order
    centres = (arrays.edges[:-1] + arrays.edges[1:]) / 2.
    assert isinstance(table, pd.DataFrame) and list(table.columns) == ['y', 'x'] and table.index.tolist() == centres.tolist()
    assert table.shape == (len(centres), 2)
    assert np.ascontiguousarray(table.values.T).tobytes() == arrays.density[0].tobytes()
    assert arrays.n[0] == want.n[1] and (arrays.count[0] == want.count[1]).all()      # the particle of one row adds no pair
    swapped = ct.vanhove(f, 2, mpp, width, reach, pos_columns=['x', 'y'])
    assert list(swapped.columns) == ['x', 'y'] and swapped['y'].values.tobytes() == table['y'].values.tobytes()
    radial = ct.vanhove(f, 2, mpp, width, reach, radial=True)
    assert isinstance(radial, pd.Series) and radial.values.tobytes() == arrays.density_r[0].tobytes()
    assert radial.index.tolist() == ((arrays.r_edges[:-1] + arrays.r_edges[1:]) / 2.).tolist()


def test_chain_from_frames_to_a_distribution_without_drift(engine):
    """six Gaussians at integer centres, all shifted by (0, +1) per frame, no noise: every displacement of
    lag k is (0, k); after the drift is subtracted every displacement is 0 -- exactly, as the MSD
    chain's msd is exactly 0 -- and nothing is copied to the host in between"""
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
    lags = [1, 2, 7, 8]
    res = ct.vanhove_arrays(r.pos, r.frame_offset, r.particle, lags, 0.5, 4., n_particles=P)
    assert all(torch.is_tensor(x) and x.is_cuda for x in res) and int(res.status) == 0
    n = res.n.cpu().numpy()
    assert n.tolist() == [42, 36, 6, 0]
    count, above = res.count.cpu().numpy(), res.above.cpu().numpy()
    for q, k in enumerate(lags[:3]):
        assert count[q, 0, 8] == n[q] and (count[q, 1, 8 + 2 * k] == n[q] if k < 4 else above[q, 1] == n[q])
    np.testing.assert_array_equal(res.mean_d.cpu().numpy()[:3], [[0., 1.], [0., 2.], [0., 7.]])
    drift = ct.compute_drift_arrays(r.pos, r.frame_offset, r.particle, n_particles=P)
    fixed = ct.subtract_drift_arrays(r.pos, r.frame_offset, drift.drift)
    assert torch.is_tensor(fixed) and fixed.is_cuda
    res = ct.vanhove_arrays(fixed, r.frame_offset, r.particle, lags, 0.5, 4., mpp=0.5, n_particles=P)
    assert all(torch.is_tensor(x) and x.is_cuda for x in res)
    np.testing.assert_array_equal(res.mean_d.cpu().numpy(), np.where(np.array(lags)[:, None] <= 7, 0., np.nan) * np.ones(2))
    count = res.count.cpu().numpy()
    assert (count[:3, :, 8] == n[:3, None]).all() and (res.count_r.cpu().numpy()[:3, 0] == n[:3]).all()
