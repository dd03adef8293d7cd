"""``ctr_cluster_tracks_device`` / ``ctr_track_positions_device`` on the MI355X against the yardstick
``tests/_cluster_tracks.py``: integers and copies of doubles, so ``assert_array_equal`` everywhere.

Launch geometry under test: every kernel runs workgroups of 256 threads (4 wavefronts of 64); a frame
goes through LDS in tiles of 256 rows (255 / 256 / 257 rows per frame), the tracks are numbered per
block of 256 particles by wavefront ballots (P = 63 / 64 / 65 and 255 / 256 / 257), the block counts are scanned by one
workgroup in chunks of 256 blocks (P = 65 535 / 65 536 / 65 537 / 131 073)."""
import functools
import sys

import numpy as np
import pandas as pd
import pytest

import _cluster_tracks as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, motion

pytestmark = pytest.mark.gpu
ctmod = sys.modules['clustertracking_amd.cluster_tracks']     # ct.cluster_tracks is the function


@functools.lru_cache(maxsize=None)
def _video(seed, cs, ndim):
    return yard.random_video(seed, n_frames=40, n_clusters=30, cluster_size=cs, ndim=ndim, extra=3)


@functools.lru_cache(maxsize=None)
def _want(seed, cs, ndim, mf):
    off, par, clu, pos = _video(seed, cs, ndim)
    res = yard.cluster_tracks(off, par, clu, cs, mf)
    return res, yard.track_positions(pos, off, par, res.track_of_particle, res.n_tracks, cs)


def check(off, par, clu, pos, cs, mf=1, want=None, n_particles=None, **kw):
    """both calls equal the yardstick; returns the device results"""
    if want is None:
        res = yard.cluster_tracks(off, par, clu, cs, mf, n_particles)
        want = res, yard.track_positions(pos, off, par, res.track_of_particle, res.n_tracks, cs)
    (w_track, w_n, w_members), (w_pos, w_present) = want
    got = ct.cluster_tracks_arrays(off, par, clu, cs, mf, n_particles=n_particles, **kw)
    assert got.status == _abi.TRACKS_OK
    assert got.n_tracks == w_n and isinstance(got.n_tracks, int)
    assert got.track_of_particle.dtype == np.int32 and got.n_members.dtype == np.int32
    np.testing.assert_array_equal(got.track_of_particle, w_track)
    np.testing.assert_array_equal(got.n_members, w_members)
    block = ct.track_positions_arrays(pos, off, par, got.track_of_particle, got.n_tracks, cs)
    assert block.present.dtype == np.int32 and block.pos.shape == w_pos.shape
    np.testing.assert_array_equal(block.present, w_present)
    np.testing.assert_array_equal(block.pos, w_pos)
    return got, block


@pytest.mark.parametrize('name', sorted(yard.KNOWN))
def test_known_answers(engine, name):
    (off, par, clu, pos), cs, mf, (track_of, n_members, present) = yard.known(name)
    got, block = check(off, par, clu, pos, cs, mf)
    np.testing.assert_array_equal(got.track_of_particle, track_of)
    np.testing.assert_array_equal(got.n_members, n_members)
    np.testing.assert_array_equal(block.present, present)


@pytest.mark.parametrize('mf', [1, 3])
@pytest.mark.parametrize('cs,ndim', [(2, 2), (2, 3), (3, 2), (3, 3), (4, 2), (4, 3)])
def test_seeded_random_video(engine, cs, ndim, mf):
    """40 frames, 30 clusters: features dropped, strangers in the group, clusters touching, ids changed
    mid-track, unlinked rows, labels that repeat across frames and negative ones"""
    off, par, clu, pos = _video(11 + cs, cs, ndim)
    got, block = check(off, par, clu, pos, cs, mf, want=_want(11 + cs, cs, ndim, mf))
    assert got.n_tracks >= 10 and (block.present == cs).any() and (block.present != cs).any()
    assert (clu < 0).any() and len(np.unique(clu)) < len(clu) // 10


def test_empty_and_tiny_tables(engine):
    none = np.zeros(0, dtype=np.int64)
    for off in (np.zeros(1, dtype=np.int64), np.zeros(4, dtype=np.int64)):        # T = 0 and N = 0
        got, block = check(off, none, none, np.zeros((0, 2)), 2)
        assert got.n_tracks == 0 and got.track_of_particle.shape == (0,) and block.pos.shape == (0, len(off) - 1, 2, 2)
    # T = 1
    check(*yard.table([[(0, 0), (1, 0), (2, 1)]]), 2)
    # an empty frame in the middle, a frame with one row, a frame of unlinked rows
    got, block = check(*yard.table([[(0, 0), (1, 0)], [], [(1, 5)], [(-1, 0), (-1, 0)], [(1, 0), (0, 0)]]), 2)
    np.testing.assert_array_equal(block.present, [[2, 0, 1, 0, 2]])
    # particles that never appear, beyond the largest id that does
    got, _ = check(*yard.table([[(0, 0), (1, 0)]]), 2, n_particles=7)
    np.testing.assert_array_equal(got.track_of_particle, [0, 0, -1, -1, -1, -1, -1])
    # no complete group at all
    got, _ = check(*yard.table([[(0, 0), (1, 0), (2, 0)], [(0, 1), (1, 2), (2, 3)]]), 2)
    assert got.n_tracks == 0


@pytest.mark.parametrize('rows', [255, 256, 257, 513])
def test_rows_per_frame_at_the_tile(engine, rows):
    """dimers and trimers whose members lie in different LDS tiles of the frame"""
    rng = np.random.RandomState(rows)
    for cs in (2, 3):
        n_groups = rows // cs
        par = np.arange(rows, dtype=np.int64)
        clu = np.r_[np.repeat(rng.permutation(n_groups) - 5, cs), np.full(rows - n_groups * cs, 10 ** 12)].astype(np.int64)
        frames = []
        for t in range(3):
            order = rng.permutation(rows)
            frames.append((par[order], clu[order]))
        off = np.arange(4, dtype=np.int64) * rows
        par3, clu3 = np.concatenate([f[0] for f in frames]), np.concatenate([f[1] for f in frames])
        got, block = check(off, par3, clu3, rng.uniform(0, 99, (3 * rows, 3)), cs, 3)
        assert got.n_tracks == n_groups and (block.present == cs).all()


@pytest.mark.parametrize('P', [63, 64, 65, 255, 256, 257, 600, 65535, 65536, 65537, 131073])
def test_particles_at_the_wavefront_and_workgroup(engine, P):
    """every second pair of neighbours bonded, ids shuffled: the roots fall on both sides of the
    ballot and block boundaries of the numbering; from 65 536 particles on the scan of the block
    counts (256, 256, 257 and 513 blocks) takes more than one chunk of its workgroup"""
    rng = np.random.RandomState(P)
    ids = rng.permutation(P).astype(np.int64)
    pairs = ids[:P // 2 * 2].reshape(-1, 2)[::2]
    par = np.tile(pairs.reshape(-1), 2)
    clu = np.tile(np.repeat(np.arange(len(pairs), dtype=np.int64), 2), 2)
    off = np.array([0, 2 * len(pairs), 4 * len(pairs)], dtype=np.int64)
    got, _ = check(off, par, clu, rng.uniform(0, 9, (len(par), 2)), 2, 2, n_particles=P)
    assert got.n_tracks == len(pairs)


@pytest.mark.parametrize('star', [False, True], ids=['path', 'star'])
def test_largest_component_settles_within_the_round_bound(engine, star):
    """4097 particles in one component, ids shuffled, one bond per frame: status 0 within
    R = 2 ceil(log2 P) + 2 rounds, queued blind and with the host reading a word"""
    n = 4097
    off, par, clu = yard.chain_table(n, star)
    max_rounds, jumps = ctmod.round_bound(n)
    assert (max_rounds, jumps) == (28, 14)
    used = []
    for check_every in (0, 2):
        got, rounds = ct.cluster_tracks_arrays(off, par, clu, 2, check_every=check_every, return_rounds=True)
        assert got.status == _abi.TRACKS_OK and got.n_tracks == 1
        np.testing.assert_array_equal(got.track_of_particle, np.zeros(n, dtype=np.int32))
        np.testing.assert_array_equal(got.n_members, [n])
        assert 1 <= rounds < max_rounds
        used.append(rounds)
    print('rounds used %s of %d' % (used, max_rounds))
    # and a forest: paths of 1, 2, 3, ... particles
    sizes = np.arange(1, 60)
    start = np.r_[0, np.cumsum(sizes)]
    ids = np.random.RandomState(3).permutation(start[-1]).astype(np.int64)
    a = np.concatenate([np.arange(s, s + k - 1) for s, k in zip(start[:-1], sizes)])
    par = np.stack([ids[a], ids[a + 1]], axis=1).reshape(-1)
    off = np.arange(0, len(par) + 1, 2, dtype=np.int64)
    got, _ = check(off, par, np.zeros(len(par), dtype=np.int64), np.zeros((len(par), 2)), 2, n_particles=len(ids))
    assert got.n_tracks == len(sizes) - 1 and sorted(got.n_members) == list(sizes[1:])


def test_same_bytes_twice_and_on_two_streams(engine):
    import torch
    cs, mf = 3, 1
    off, par, clu, pos = _video(14, cs, 3)
    want = _want(14, cs, 3, mf)
    first, first_block = check(off, par, clu, pos, cs, mf, want=want)
    for check_every in (0, 1, 2):
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for s in streams:
            with torch.cuda.stream(s):
                got, block = check(off, par, clu, pos, cs, mf, want=want, check_every=check_every)
            for a, b in zip((got.track_of_particle, got.n_members, block.pos, block.present),
                            (first.track_of_particle, first.n_members, first_block.pos, first_block.present)):
                assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('cs,ndim', [(2, 2), (3, 3), (4, 3)])
def test_tensors_chain_into_orientation(engine, cs, ndim):
    """tensors in give tensors out, orientation_arrays takes them; on a clean table (every member in
    one complete group per frame) the result equals orientation_df(track_column=...) bit for bit"""
    import torch
    off, par, clu, pos = yard.clean_video(cs, 9, 7, cs, ndim)
    dev = torch.device('cuda', 0)
    t = [torch.from_numpy(a).to(dev) for a in (off, par, clu, pos)]
    got = ct.cluster_tracks_arrays(t[0], t[1], t[2], cs, n_particles=7 * cs)
    assert isinstance(got.track_of_particle, torch.Tensor) and isinstance(got.n_members, torch.Tensor)
    assert got.track_of_particle.device == dev and got.status == 0 and got.n_tracks == 7
    block = ct.track_positions_arrays(t[3], t[0], t[1], got.track_of_particle, got.n_tracks, cs)
    assert isinstance(block.pos, torch.Tensor) and block.pos.device == dev and block.pos.dtype == torch.float64
    res = yard.cluster_tracks(off, par, clu, cs)
    w_pos, w_present = yard.track_positions(pos, off, par, res.track_of_particle, res.n_tracks, cs)
    np.testing.assert_array_equal(got.track_of_particle.cpu().numpy(), res.track_of_particle)
    np.testing.assert_array_equal(block.pos.cpu().numpy(), w_pos)
    np.testing.assert_array_equal(block.present.cpu().numpy(), w_present)
    # without n_particles: one more host read, the same result
    again = ct.cluster_tracks_arrays(t[0], t[1], t[2], cs)
    assert torch.equal(again.track_of_particle, got.track_of_particle)
    com, bases = motion.orientation_arrays(block.pos, cs, ndim, mpp=0.5)
    assert isinstance(com, torch.Tensor)
    columns = ['y', 'x'] if ndim == 2 else ['z', 'y', 'x']
    f = pd.DataFrame(pos, columns=columns)
    f['frame'] = np.repeat(np.arange(len(off) - 1), np.diff(off)) + 3
    f['particle'] = par * 10 + 7                     # any integers: mapped through their sorted unique
    f['cluster'] = clu
    f = f.sample(frac=1., random_state=1)
    ft = ct.cluster_tracks(f, cs)
    assert ft.attrs == {'n_tracks': 7, 'n_conflict': 0, 'n_incomplete': 0} and list(ft.index) == list(f.index)
    np.testing.assert_array_equal(ft['cluster_track'].values, res.track_of_particle[(ft['particle'].values - 7) // 10])
    com_df, bases_df, ids = motion.orientation_df(ft, cs, mpp=0.5, ndim=ndim, track_column='cluster_track')
    np.testing.assert_array_equal(ids, np.arange(7))
    assert com.cpu().numpy().tobytes() == com_df.tobytes() and bases.cpu().numpy().tobytes() == bases_df.tobytes()
    assert np.isfinite(com_df).all()
    dense, track_ids, first = ct.track_positions(f, cs)
    assert first == 3 and list(track_ids) == list(range(7))
    np.testing.assert_array_equal(dense, w_pos)


def test_dataframe_counts_cells_and_missing_frames(engine):
    off, par, clu, pos = yard.table([[(10, 0), (20, 0)], [(10, 0), (30, 0), (20, 9)], [(20, 1)], [(10, 2), (20, 2)]])
    f = pd.DataFrame({'frame': np.repeat([2, 3, 6, 7], np.diff(off)), 'y': pos[:, 0], 'x': pos[:, 1],
                      'particle': par.astype(np.int32), 'cluster': clu})
    ft = ct.cluster_tracks(f, 2)
    np.testing.assert_array_equal(ft['cluster_track'].values, np.zeros(len(f), dtype=np.int64))
    # frames 2 .. 7: complete, conflict, two missing, incomplete, complete
    assert ft.attrs == {'n_tracks': 1, 'n_conflict': 1, 'n_incomplete': 3}
    dense, ids, first = ct.track_positions(f, 2)
    assert first == 2 and dense.shape == (1, 6, 2, 2)
    np.testing.assert_array_equal(np.isnan(dense[0, :, 0, 0]), [False, True, True, True, True, False])
    np.testing.assert_array_equal(dense[0, 5], pos[[6, 7]])
    lonely = ct.cluster_tracks(f[f['particle'] == 10], 2)
    assert (lonely['cluster_track'] == -1).all() and lonely.attrs['n_tracks'] == 0


def test_bad_tables_are_refused_by_the_setup_kernel(engine):
    """a particle >= P and offsets that fall or leave [0, N]: status, no track, nothing followed"""
    import torch
    off, par, clu, pos = yard.table([[(0, 0), (1, 0)], [(0, 0), (1, 0)], [(2, 1), (3, 1)]])
    for bad_off, bad_par, P in ((off, par, 3), (np.array([0, 4, 2, 6]), par, 4), (np.array([0, 2, 4, 7]), par, 4),
                                (np.array([-1, 2, 4, 6]), par, 4)):
        got = ct.cluster_tracks_arrays(bad_off, bad_par, clu, 2, n_particles=P)
        assert got.status == _abi.TRACKS_BAD_TABLE and got.n_tracks == 0 and len(got.n_members) == 0
        np.testing.assert_array_equal(got.track_of_particle, np.full(P, -1))
    good = ct.cluster_tracks_arrays(off, par, clu, 2)
    assert good.status == 0 and good.n_tracks == 2
    for bad_off, bad_par, bad_track in ((np.array([0, 4, 2, 6]), par, good.track_of_particle),
                                        (off, par + 1, good.track_of_particle),
                                        (off, par, good.track_of_particle + 1)):
        with pytest.raises(ValueError, match='frame_offset must rise'):
            ct.track_positions_arrays(pos, bad_off, bad_par, bad_track, 2, 2)
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pos, bad_off, bad_par, bad_track)]
        block = ct.track_positions_arrays(t[0], t[1], t[2], t[3], 2, 2)
        assert torch.isnan(block.pos).all() and not block.present.any()


def _dimer_video(n_frames=16, shape=(64, 64)):
    rng = np.random.RandomState(0)
    centre = np.array([[18., 20.], [44., 42.]])
    angle = np.array([0.3, 1.9])
    grid = np.indices(shape).astype(np.float64)
    frames = np.zeros((n_frames,) + shape, dtype=np.uint8)
    for t in range(n_frames):
        centre += rng.normal(0, 0.4, centre.shape)
        angle += rng.normal(0, 0.08, 2)
        im = np.zeros(shape)
        for c, a in zip(centre, angle):
            half = 4.5 * np.array([np.sin(a), np.cos(a)])
            for p in (c - half, c + half):
                im += 160. * np.exp(-((grid[0] - p[0]) ** 2 + (grid[1] - p[1]) ** 2) / (2 * 1.6 ** 2))
        frames[t] = np.clip(im, 0, 255).astype(np.uint8)
    return frames


def test_end_to_end_from_frames_to_the_diffusion_tensor(engine):
    frames = _dimer_video()
    r = ct.find_link_arrays(frames, search_range=4, separation=5, diameter=7)
    f = pd.DataFrame({'y': r.pos[:, 0], 'x': r.pos[:, 1], 'particle': r.particle,
                      'frame': np.repeat(np.arange(len(frames)), np.diff(r.frame_offset))})
    assert len(f) == 4 * len(frames) and r.n_tracks == 4
    f = ct.find_clusters(f, 12, labels='device')
    ft = ct.cluster_tracks(f, 2, min_frames=3)
    assert ft.attrs == {'n_tracks': 2, 'n_conflict': 0, 'n_incomplete': 0}
    assert sorted(np.bincount(ft['cluster_track'].values)) == [2 * len(frames)] * 2
    pos, ids, first = ct.track_positions(ft, 2, min_frames=3)
    assert pos.shape == (2, len(frames), 2, 2) and first == 0 and np.isfinite(pos).all()
    com, bases = motion.orientation_arrays(pos, 2, 2)
    tensor = motion.diffusion_tensor(com, bases, lagtime=1, fps=1., ndim=2)
    assert tensor.shape == (2, 3, 3) and np.isfinite(tensor).all()
