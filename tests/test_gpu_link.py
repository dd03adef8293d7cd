"""Linking on the device (``ctr_link_device``) against the reference's recorded ids
(tests/golden/link_cases.npz, tests/golden/link/link_edge_cases.npz) and the unchanged host
``link.link_levels``."""
import os

import numpy as np
import pandas as pd
import pytest
from numpy.testing import assert_equal
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import _cases
import clustertracking_amd as cta
from clustertracking_amd import _lib
from clustertracking_amd import link as lk

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(_cases.GOLDEN, 'link_cases.npz'))
E = np.load(os.path.join(_cases.GOLDEN, 'link', 'link_edge_cases.npz'))
FIXTURES = ([(Z, k[:-4]) for k in sorted(Z.files) if k.endswith('_ids') and k != 'dense2d_ids'] +
            [(E, k[:-4]) for k in sorted(E.files) if k.endswith('_ids')])


def _levels(z, name):
    offs = np.r_[0, np.cumsum(z[name + '_counts'])]
    return [z[name + '_pos'][a:b] for a, b in zip(offs[:-1], offs[1:])]


def walkers(seed, n, n_frames, ndim, box, step, p_drop=0., p_birth=0.):
    rng = np.random.RandomState(seed)
    pos = rng.uniform(0, box, (n, ndim))
    levels = []
    for t in range(n_frames):
        pos = pos + rng.normal(0, step, pos.shape)
        lvl = pos[rng.rand(len(pos)) >= p_drop]
        n_new = rng.poisson(p_birth) if p_birth else 0
        if n_new:
            born = rng.uniform(0, box, (n_new, ndim))
            pos = np.concatenate([pos, born])
            lvl = np.concatenate([lvl, born])
        levels.append(lvl[rng.permutation(len(lvl))])
    return levels


def _level_links(prev_ids, cur_ids, src_pos_of, cur_pos, sr):
    """(links, sum d^2) of one level; src_pos_of: id -> last position"""
    n, cost = 0, 0.
    for j, p in enumerate(cur_ids):
        if p in src_pos_of:
            cost += np.sum(((src_pos_of[p] - cur_pos[j]) / sr) ** 2)
            n += 1
    return n, cost


def assert_same_ids(levels, sr, memory, got, want):
    """ids identical level by level; a failure names the level, the link counts and sum d^2"""
    sr = np.asarray(lk.validate_tuple(sr, levels[0].shape[1]), dtype=float)
    assert [len(g) for g in got] == [len(l) for l in levels]
    last_g, last_w = {}, {}
    for t, lv in enumerate(levels):
        if not np.array_equal(got[t], want[t]):
            n_g, c_g = _level_links(None, got[t], last_g, lv, sr)
            n_w, c_w = _level_links(None, want[t], last_w, lv, sr)
            raise AssertionError("level %d (memory %d): device %d links, sum d^2 %.12g; host %d links, "
                                 "sum d^2 %.12g; %d of %d ids differ"
                                 % (t, memory, n_g, c_g, n_w, c_w, int((got[t] != want[t]).sum()), len(lv)))
        for j, p in enumerate(got[t]):
            last_g[p] = last_w[p] = lv[j]


def largest_subnet_sources(levels, sr, destinations=False):
    """largest number of sources in one sub-network (memory 0), on the host; ``destinations``:
    (sources, destinations) of the sub-network with the most sources + destinations"""
    best, both = 0, (0, 0)
    for a, b in zip(levels[:-1], levels[1:]):
        if not len(a) or not len(b):
            continue
        d, i = cKDTree(a / sr).query(b / sr, min(10, len(a)), distance_upper_bound=1 + 1e-7)
        d, i = d.reshape(len(b), -1), i.reshape(len(b), -1)
        ok = np.isfinite(d)
        src, dst = i[ok], np.nonzero(ok)[0]
        if not len(src):
            continue
        g = coo_matrix((np.ones(len(src)), (src, dst + len(a))), shape=(len(a) + len(b),) * 2)
        _, comp = connected_components(g, directed=False)
        per = np.bincount(comp[np.unique(src)])
        best = max(best, int(per.max()))
        per_d = np.bincount(comp[np.unique(dst) + len(a)], minlength=len(per))
        k = int(np.argmax(per + per_d[:len(per)]))
        if per[k] + per_d[k] > sum(both):
            both = (int(per[k]), int(per_d[k]))
    return both if destinations else best


@pytest.mark.parametrize('z,name', FIXTURES, ids=[f[1] for f in FIXTURES])
def test_ids_equal_reference(z, name):
    levels = _levels(z, name)
    sr, memory = tuple(z[name + '_sr']), int(z[name + '_memory'])
    got = lk.link_levels(levels, sr, memory, engine='device')
    assert [len(g) for g in got] == list(z[name + '_counts'])
    assert_same_ids(levels, sr, memory, got, [np.asarray(i) for i in np.split(z[name + '_ids'], np.cumsum(z[name + '_counts'])[:-1])])
    assert all(g.dtype == np.int64 for g in got)


def test_dense2d_fixture_equals_host():
    levels = _levels(Z, 'dense2d')
    sr = tuple(Z['dense2d_sr'])
    assert largest_subnet_sources(levels, np.asarray(sr)) >= 10
    assert_same_ids(levels, sr, 0, lk.link_levels(levels, sr, 0, engine='device'), lk.link_levels(levels, sr, 0))


RANDOM = [
    # seed, walkers, frames, ndim, box, step, drop, birth, search_range
    (1, 60, 12, 2, 200., 1.0, 0.05, 1.0, 5.),
    (2, 150, 10, 2, 100., 1.5, 0.05, 1.0, 5.),            # dense: sub-networks of 10 x 10 and more
    (3, 150, 8, 2, 100., 1.5, 0., 0., (5., 5.)),
    (4, 80, 10, 3, 60., 1.0, 0.1, 0.5, (3., 6., 6.)),     # anisotropic
    (5, 100, 10, 2, 150., 1.2, 0.1, 1.0, (3., 6.)),
    (6, 3000, 4, 2, 2000., 1.0, 0.02, 3.0, 5.),           # a level larger than one workgroup
    (7, 300, 6, 3, 60., 1.0, 0.05, 1.0, 4.),
    (8, 0, 6, 2, 100., 1.0, 0., 2.0, 5.),                 # starts empty, only births
]


@pytest.mark.parametrize('memory', [0, 1, 2, 3])
@pytest.mark.parametrize('case', RANDOM, ids=lambda c: 'seed%d' % c[0])
def test_random_walkers_equal_host(case, memory):
    seed, n, frames, ndim, box, step, drop, birth, sr = case
    levels = walkers(seed, n, frames, ndim, box, step, drop, birth)
    want = lk.link_levels(levels, sr, memory)
    got = lk.link_levels(levels, sr, memory, engine='device')
    assert_same_ids(levels, sr, memory, got, want)


def test_random_cases_reach_large_subnets_and_large_levels():
    sizes = {c[0]: largest_subnet_sources(walkers(*c[:8]), np.asarray(lk.validate_tuple(c[8], c[3]), float))
             for c in RANDOM if c[0] in (2, 3)}
    print('largest sub-networks (sources):', sizes)
    assert max(sizes.values()) >= 10
    assert max(len(l) for l in walkers(*RANDOM[5][:8])) > 1024


def test_integer_positions_same_objective():
    """ties are real on a grid: per level the same number of links and the same sum d^2, every
    link within range, every id once per level"""
    for seed in (11, 12, 13):
        levels = [np.round(l) for l in walkers(seed, 100, 8, 2, 80., 1.5, 0.05, 1.0)]
        sr = np.array([4., 4.])
        want = lk.link_levels(levels, tuple(sr), 0)
        got = lk.link_levels(levels, tuple(sr), 0, engine='device')
        for t in range(1, len(levels)):
            assert len(set(got[t])) == len(got[t])
            sides = []
            for ids in (got, want):
                where = {p: i for i, p in enumerate(ids[t - 1])}
                d2 = np.array([np.sum(((levels[t - 1][where[p]] - levels[t][j]) / sr) ** 2)
                               for j, p in enumerate(ids[t]) if p in where])
                assert np.all(d2 <= (1 + 1e-7) ** 2)
                sides.append((len(d2), d2.sum()))
            print('seed %d level %d: device %r host %r' % (seed, t, sides[0], sides[1]))
            assert sides[0][0] == sides[1][0], (seed, t, sides)
            assert abs(sides[0][1] - sides[1][1]) <= 1e-9 * max(sides[1][1], 1e-300), (seed, t, sides)
        assert_equal(got[0], want[0])
        assert max(map(max, got)) == max(map(max, want))     # as many tracks


def test_oversize_subnet_raises_and_engine_recovers():
    levels = None
    for n in (220, 260, 300):
        cand = walkers(20 + n, n, 4, 2, 100., 1.5)
        try:
            lk.link_levels(cand, 5., 0)
        except lk.SubnetOversizeException:
            levels = cand
            break
    assert levels is not None, "no seed tried makes the host linker raise"
    with pytest.raises(lk.SubnetOversizeException):
        lk.link_levels(levels, 5., 0)
    with pytest.raises(lk.SubnetOversizeException) as info:
        lk.link_levels(levels, 5., 0, engine='device')
    assert 'Subnetwork contains' in str(info.value)
    with pytest.raises(lk.SubnetOversizeException):
        lk.link_levels(levels, 5., 2, engine='device')
    sparse = _levels(Z, 'sparse2d')
    got = lk.link_levels(sparse, tuple(Z['sparse2d_sr']), 0, engine='device')
    assert_equal(np.concatenate(got), Z['sparse2d_ids'])


def test_destination_capacity_is_reported():
    """one source in range of 70 destinations: 1 x 70, beyond the solver's 64 columns"""
    rng = np.random.RandomState(5)
    levels = [np.array([[50., 50.]]), 50. + rng.uniform(-1, 1, (70, 2))]
    with pytest.raises(_lib.EngineError) as info:
        lk.link_levels(levels, 5., 0, engine='device')
    assert 'level 1' in str(info.value) and '70' in str(info.value)
    levels[1] = levels[1][:64]
    assert_same_ids(levels, 5., 0, lk.link_levels(levels, 5., 0, engine='device'), lk.link_levels(levels, 5., 0))


def test_empty_inputs():
    assert lk.link_levels([], 5., engine='device') == []
    got = lk.link_levels([np.zeros((0, 2))] * 3, 5., engine='device')
    assert [g.shape for g in got] == [(0,)] * 3 and all(g.dtype == np.int64 for g in got)
    assert cta.link_arrays(np.zeros((0, 3)), [0], (5., 5., 5.)).shape == (0,)
    assert cta.link_arrays(np.zeros((0, 2)), [0, 0, 0], 5.).shape == (0,)


def test_tensors_and_stream():
    import torch
    levels = walkers(31, 80, 10, 2, 120., 1.0, 0.1, 1.0)
    offs = np.r_[0, np.cumsum([len(l) for l in levels])].astype(np.int64)
    pos = np.concatenate(levels)
    for memory in (0, 2):
        want = np.concatenate(lk.link_levels(levels, 5., memory))
        assert_equal(cta.link_arrays(pos, offs, 5., memory), want)
        pt, ot = torch.from_numpy(pos).cuda(), torch.from_numpy(offs).cuda()
        assert_equal(cta.link_arrays(pt, ot, 5., memory), want)
        t = lk.link_arrays(pt, ot, 5., memory, _on_device=True)
        assert t.is_cuda and t.dtype == torch.int64
        assert_equal(t.cpu().numpy(), want)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            got = cta.link_arrays(pt, offs, 5., memory)
        stream.synchronize()
        assert_equal(got, want)
    with pytest.raises(ValueError):
        cta.link_arrays(pos, offs, 0.)
    with pytest.raises(ValueError):
        cta.link_arrays(pos, offs, 5., memory=-1)
    with pytest.raises(ValueError):
        cta.link_arrays(pos, offs[:-1], 5.)


def test_dataframe_api_on_a_shuffled_table():
    counts, pos = Z['sparse2d_counts'], Z['sparse2d_pos']
    f = pd.DataFrame(pos, columns=['y', 'x'])
    f['frame'] = np.repeat(np.arange(len(counts)), counts)
    shuffled = f.sample(frac=1., random_state=0)
    for memory in (0, 2):
        want = lk.link(shuffled, 5., memory)
        got = lk.link(shuffled, 5., memory, engine='device')
        assert list(got.columns) == list(want.columns) and got.index.equals(want.index)
        assert_equal(got['particle'].values, want['particle'].values)
    assert_equal(cta.link_df(f, 5., engine='device')['particle'].values, Z['sparse2d_ids'])


def test_chained_from_locate_and_refine():
    """locate -> refine_leastsq -> link on a small cfg-2 crop: the device ids are the host's"""
    from clustertracking_amd import workloads
    frames, _, truth, opts = workloads.cfg2(n_frames=4)
    f = cta.locate(frames, 13, minmass=2000)
    start = f.copy()
    start['background'] = 5.
    res = cta.refine_leastsq(start, cta.ArrayReader(frames), diameter=13, separation=13)
    for table in (f, res):
        for memory in (0, 1):
            want = lk.link(table, 6., memory, pos_columns=['y', 'x'])
            got = lk.link(table, 6., memory, pos_columns=['y', 'x'], engine='device')
            assert_equal(got['particle'].values, want['particle'].values)


def test_cfg4_shard_at_full_size():
    """one GPU's shard of cfg 4: 1250 levels x 200 walkers in 512^2, steps 0.5 px, search_range 3"""
    rng = np.random.RandomState(4)
    pos = rng.uniform(0, 512, (200, 2))
    levels = []
    for t in range(1250):
        pos = pos + rng.normal(0, 0.5, pos.shape)
        levels.append(pos[rng.permutation(200)].copy())
    want = lk.link_levels(levels, 3., 0)
    got = lk.link_levels(levels, 3., 0, engine='device')
    assert_same_ids(levels, 3., 0, got, want)
