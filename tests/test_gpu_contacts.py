"""Contact episodes and bond lifetimes on the device (ctr_contacts_device) against the restatement of
tests/_contacts.py: exact equality in every output, the bytes of min_d2 / max_d2 included.  The mixed
table (a frame of three tiles, empty frames, unlinked rows, NaN positions, a repeated particle), dense
frames whose entries span several scan tiles and more than one trip of the scan over their sums, a chain
longer than any workgroup with its episodes written by hand, a lowered grid cap, the capacity, refused
tables, empty inputs, determinism and the types of the outputs."""
import numpy as np
import pandas as pd
import pytest

import _contacts as rule
import clustertracking_amd as ct
from clustertracking_amd import _abi

pytestmark = pytest.mark.gpu

_tables, _want = {}, {}
PARAMS = {'no_hysteresis': dict(r_off=None, gap=0), 'hysteresis': dict(r_off=rule.R_OFF, gap=0),
          'hysteresis_gap': dict(r_off=rule.R_OFF, gap=2)}


def mixed(ndim):
    if ndim not in _tables:
        _tables[ndim] = rule.mixed_table(ndim)
    return _tables[ndim]


def want(ndim, params, pairs):
    """the restatement on the mixed table: computed once, shared by the tests, never changed"""
    key = (ndim, params, pairs)
    if key not in _want:
        pos, off, par, group, P = mixed(ndim)
        _want[key] = rule.contacts(pos, off, par, rule.R_ON, mpp=rule.MIXED_MPP[ndim], group=group, pairs=pairs, n_particles=P,
                                   **PARAMS[params])
    return _want[key]


def call(ndim, params, pairs, **kw):
    pos, off, par, group, P = mixed(ndim)
    return ct.contacts_arrays(pos, off, par, rule.R_ON, mpp=rule.MIXED_MPP[ndim], group=group, pairs=pairs, n_particles=P,
                              **dict(PARAMS[params], **kw))


def blob(res):
    """every output of a result of ndarrays as bytes"""
    return b''.join(np.ascontiguousarray(np.asarray(x)).tobytes() for x in res)


# ---- the mixed table ----
@pytest.mark.parametrize('pairs', ['all', 'same', 'other'])
@pytest.mark.parametrize('params', sorted(PARAMS))
@pytest.mark.parametrize('ndim', [2, 3])
def test_mixed_table(engine, ndim, params, pairs):
    got, ref = call(ndim, params, pairs), want(ndim, params, pairs)
    print(ndim, params, pairs, 'entries', ref.n_entries, 'duplicates', ref.duplicates, 'episodes', ref.n_episodes, 'pairs', ref.n_pairs)
    assert ref.n_entries > 200 and (pairs == 'same' or ref.n_episodes > 20)
    rule.assert_same(got, ref, (ndim, params, pairs))
    assert got.lifetime.sum() == got.active.sum() and got.lifetime_count.sum() + got.lifetime_above.sum() == got.n_episodes


def test_same_plus_other_is_all(engine):
    n = {pairs: call(2, 'hysteresis', pairs).n_entries for pairs in ('all', 'same', 'other')}
    assert n['all'] == n['same'] + n['other'] and n['same'] > 0 and n['other'] > 0


def test_max_lifetime_shortens_the_histogram(engine):
    pos, off, par, group, P = mixed(2)
    ref = rule.contacts(pos, off, par, rule.R_ON, rule.R_OFF, gap=2, max_lifetime=7, n_particles=P)
    got = ct.contacts_arrays(pos, off, par, rule.R_ON, rule.R_OFF, gap=2, max_lifetime=7, n_particles=P)
    rule.assert_same(got, ref)
    assert got.lifetime_count.shape == (2, 7) and got.lifetime_above.sum() > 0
    counted = ct.contacts_arrays(pos, off, par, rule.R_ON, rule.R_OFF, gap=2, max_lifetime=7)      # P from the column
    rule.assert_same(counted, ref)


# ---- dense frames: several scan tiles, more than one trip over their sums ----
def test_dense_frames(engine):
    pos, off, par = rule.dense_frames()
    ref = rule.contacts(pos, off, par, 5., rule.R_OFF)
    assert ref.n_entries == 3 * 44850 and ref.n_entries > 256 * 256 and ref.n_episodes > 256 * 64 and ref.n_pairs > 256 * 64
    got = ct.contacts_arrays(pos, off, par, 5., rule.R_OFF)
    rule.assert_same(got, ref, 'dense')
    assert not got.left_open.any() and not got.right_open.any()              # frames 0 and 4 hold everyone, far apart


# ---- a chain longer than any workgroup ----
def test_long_chain(engine):
    pos, off, par, episodes = rule.long_chain()
    got = ct.contacts_arrays(pos, off, par, rule.LONG_R_ON, rule.LONG_R_OFF, gap=rule.LONG_GAP)
    assert [tuple(getattr(got, name)[x].item() for name in rule.EPISODE) for x in range(got.n_episodes)] == episodes
    assert (got.n_entries, got.duplicates, got.n_episodes, got.n_pairs, got.status) == (rule.LONG_T - 7, 0, 3, 1, _abi.CON_OK)
    assert [getattr(got, name).tolist() for name in rule.PAIR] == [[0], [1], [3], [500 + 698 + 1794], [0], [2999]]
    assert got.formed.nonzero()[0].tolist() == [502, 1206] and got.broken.nonzero()[0].tolist() == [500, 1200]
    assert got.active.sum() == 500 + 698 + 1794 and got.active[[499, 500, 501, 502, 1200, 1205, 1206, 2000]].tolist() == [1, 0, 0, 1, 0, 0, 1, 1]
    rule.assert_same(got, rule.contacts(pos, off, par, rule.LONG_R_ON, rule.LONG_R_OFF, gap=rule.LONG_GAP), 'long')


# ---- a lowered grid cap ----
def test_under_a_lowered_grid_cap(engine):
    """one, two and three workgroups walk the work items of the mixed table, the tiles of every scan, the
    chains, the episodes and the pairs: the bytes of the default run"""
    base = call(2, 'hysteresis_gap', 'all')
    rule.assert_same(base, want(2, 'hysteresis_gap', 'all'))
    for cap in (1, 2, 3):
        with engine.stage_max_grid(cap):
            got = call(2, 'hysteresis_gap', 'all')
        assert got.status == _abi.CON_OK and blob(got) == blob(base), cap
    assert engine.set_stage_max_grid(0) == 65536


# ---- capacity ----
def test_capacity(engine):
    import torch
    ref = want(2, 'hysteresis_gap', 'all')
    base = call(2, 'hysteresis_gap', 'all')
    exact = call(2, 'hysteresis_gap', 'all', max_entries=ref.n_entries)
    assert exact.status == _abi.CON_OK and blob(exact) == blob(base)
    roomy = call(2, 'hysteresis_gap', 'all', max_entries=ref.n_entries + 1000)
    assert blob(roomy) == blob(base)
    short = call(2, 'hysteresis_gap', 'all', max_entries=ref.n_entries - 1)
    pos, off, par, group, P = mixed(2)
    rule.assert_same(short, rule.defaults(len(off) - 1, P, status=_abi.CON_OVERFLOW, n_entries=ref.n_entries), 'overflow')
    none = call(2, 'hysteresis_gap', 'all', max_entries=0)
    rule.assert_same(none, rule.defaults(len(off) - 1, P, status=_abi.CON_OVERFLOW, n_entries=ref.n_entries), 'no room')
    # tensors: the columns at their capacity, -1 and NaN in every row
    t = [torch.from_numpy(x).cuda() for x in (pos, off, par)]
    m = ref.n_entries - 1
    got = ct.contacts_arrays(*t, rule.R_ON, rule.R_OFF, gap=2, n_particles=P, max_entries=m)
    assert int(got.status) == _abi.CON_OVERFLOW and int(got.n_entries) == ref.n_entries
    rule.assert_same(rule.of_tensors(got, m), rule.defaults(len(off) - 1, P, status=_abi.CON_OVERFLOW, n_entries=ref.n_entries))


# ---- refused tables ----
BAD_TABLES = {'offsets_fall': lambda off, par, P: (np.where(np.arange(len(off)) == 5, off[4] - 1, off), par, P),
              'offsets_beyond': lambda off, par, P: (np.where(np.arange(len(off)) == len(off) - 1, off[-1] + 1, off), par, P),
              'offsets_negative': lambda off, par, P: (np.where(np.arange(len(off)) == 0, -1, off), par, P),
              'particle_at_P': lambda off, par, P: (off, par, P - 1)}


@pytest.mark.parametrize('name', sorted(BAD_TABLES))
def test_refused_tables(engine, name):
    import torch
    pos, off, par, group, P = mixed(2)
    off, par, P = BAD_TABLES[name](off, par, P)
    with pytest.raises(ValueError, match='frame_offset must rise'):
        ct.contacts_arrays(pos, off, par, rule.R_ON, n_particles=P)
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (pos, off, par)]
    for m in (None, 500):
        got = ct.contacts_arrays(*t, rule.R_ON, n_particles=P, max_entries=m)
        assert int(got.status) == _abi.CON_BAD_TABLE
        rule.assert_same(rule.of_tensors(got, m or 0), rule.defaults(len(off) - 1, P))


# ---- empty inputs ----
def test_empty_inputs(engine):
    none = ct.contacts_arrays(np.zeros((0, 2)), np.array([0]), np.zeros(0, dtype=np.int64), 2.)          # N = 0, T = 0
    rule.assert_same(none, rule.contacts(np.zeros((0, 2)), np.array([0]), np.zeros(0, dtype=np.int64), 2.))
    assert none.formed.shape == (0,) and none.lifetime_count.shape == (2, 1) and none.first_seen.shape == (0,)
    off = np.zeros(4, dtype=np.int64)
    frames = ct.contacts_arrays(np.zeros((0, 3)), off, np.zeros(0, dtype=np.int64), 2., n_particles=3, max_entries=10)       # N = 0, T = 3
    rule.assert_same(frames, rule.contacts(np.zeros((0, 3)), off, np.zeros(0, dtype=np.int64), 2., n_particles=3))
    assert frames.first_seen.tolist() == [3, 3, 3] and frames.last_seen.tolist() == [-1, -1, -1]
    pos = np.array([[0., 0.], [0., 50.], [0., 0.], [0., 50.]])                                          # no contact at all
    apart = ct.contacts_arrays(pos, np.array([0, 2, 4]), np.array([0, 1, 0, 1]), 2., 4.)
    rule.assert_same(apart, rule.contacts(pos, np.array([0, 2, 4]), np.array([0, 1, 0, 1]), 2., 4.))
    assert apart.n_entries == 0 and apart.a.shape == (0,) and apart.active.tolist() == [0, 0]
    unlinked = ct.contacts_arrays(pos, np.array([0, 2, 4]), np.array([-1, -1, -1, -1]), 100.)           # P = 0
    assert unlinked.n_entries == 0 and unlinked.status == _abi.CON_OK and unlinked.first_seen.shape == (0,)


# ---- determinism and types ----
def test_tensors_in_tensors_out(engine):
    import torch
    pos, off, par, group, P = mixed(3)
    ref = want(3, 'hysteresis_gap', 'other')
    kw = dict(r_off=rule.R_OFF, gap=2, mpp=rule.MIXED_MPP[3], pairs='other', n_particles=P)
    t_pos, t_off, t_par, t_group = (torch.from_numpy(x).cuda() for x in (pos, off, par, group))
    m = ref.n_entries + 77
    first = None
    for _ in range(2):                               # two calls: the same bytes
        got = ct.contacts_arrays(t_pos, t_off, t_par, rule.R_ON, group=t_group, max_entries=m, **kw)
        assert all(torch.is_tensor(x) and x.device == t_pos.device for x in got)
        assert got.status.dtype == torch.int32 and got.status.shape == (1,) and int(got.status) == _abi.CON_OK
        assert all(getattr(got, name).dtype == torch.int64 and getattr(got, name).shape == (1,) for name in rule.SCALARS[:4])
        assert got.left_open.dtype == got.right_open.dtype == torch.int32 and got.min_d2.dtype == torch.float64
        assert got.lifetime_count.shape == (2, len(off) - 1) and got.first_seen.shape == (P,)
        as_arrays = rule.of_tensors(got, m)
        first = first or blob(as_arrays)
        assert blob(as_arrays) == first
    rule.assert_same(as_arrays, ref, 'tensors')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = ct.contacts_arrays(t_pos, t_off, t_par, rule.R_ON, group=t_group, max_entries=m, **kw)
    s.synchronize()
    assert blob(rule.of_tensors(other, m)) == first
    again = ct.contacts_arrays(pos, off, par, rule.R_ON, group=group, **kw)          # the same bytes from ndarrays, the default path
    assert isinstance(again.a, np.ndarray) and isinstance(again.n_entries, int) and blob(again) == first
    exact = ct.contacts_arrays(t_pos, t_off, t_par, rule.R_ON, group=t_group, **kw)  # tensors, the default path: exactly n_entries rows
    assert exact.a.shape == (ref.n_entries,) and blob(rule.of_tensors(exact, ref.n_entries)) == first
    with pytest.raises(ValueError, match='float64'):
        ct.contacts_arrays(t_pos.float(), t_off, t_par, rule.R_ON)
    with pytest.raises(ValueError, match='int64'):
        ct.contacts_arrays(t_pos, t_off, t_par.int(), rule.R_ON)


def test_the_table_forms(engine):
    """the original ids and frames, on a table whose frames do not start at 0 and come in any order"""
    pos, off, par, group, P = mixed(2)
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    linked = par >= 0
    ids = 7 * np.arange(P) + 1000                                            # ascending: the dense ids keep their order
    seen = np.unique(par[linked])
    f = pd.DataFrame({'y': pos[linked, 0], 'x': pos[linked, 1], 'frame': frame[linked] + 100, 'particle': ids[par[linked]],
                      'cluster': group[linked]})
    # the frames in any order, the rows of a frame in theirs: which row of a repeated particle comes first is part of the rule
    f = f.iloc[np.argsort(np.random.RandomState(3).permutation(len(off) - 1)[frame[linked]], kind='stable')]
    assert not f['frame'].is_monotonic_increasing
    dense = np.searchsorted(seen, par[linked])
    sizes = np.bincount(frame[linked], minlength=len(off) - 1)
    ref = rule.contacts(pos[linked], np.concatenate([[0], np.cumsum(sizes)]), dense, rule.R_ON, rule.R_OFF, gap=2, n_particles=len(seen))
    eps = ct.contacts(f, rule.R_ON, rule.R_OFF, gap=2)
    assert eps.columns.tolist() == ['particle_a', 'particle_b', 'first_frame', 'last_frame', 'lifetime', 'n_seen', 'left_open',
                                    'right_open', 'min_dist', 'max_dist']
    assert eps['particle_a'].tolist() == ids[seen[ref.a]].tolist() and eps['particle_b'].tolist() == ids[seen[ref.b]].tolist()
    assert eps['first_frame'].tolist() == (ref.first + 100).tolist() and eps['last_frame'].tolist() == (ref.last + 100).tolist()
    assert eps['lifetime'].tolist() == ref.lifetime.tolist() and eps['n_seen'].tolist() == ref.n_seen.tolist()
    assert eps['left_open'].tolist() == ref.left_open.tolist() and eps['right_open'].tolist() == ref.right_open.tolist()
    rule.assert_equal_bits(eps['min_dist'].values, np.sqrt(ref.min_d2))
    rule.assert_equal_bits(eps['max_dist'].values, np.sqrt(ref.max_d2))
    assert eps.attrs == {'n_entries': ref.n_entries, 'duplicates': ref.duplicates, 'n_episodes': ref.n_episodes, 'n_pairs': ref.n_pairs}
    assert ref.duplicates > 0
    b = ct.bonds(f, rule.R_ON, rule.R_OFF, gap=2, min_frames=20)
    keep = ref.pair_frames >= 20
    assert 0 < keep.sum() < ref.n_pairs
    assert b.columns.tolist() == ['particle_a', 'particle_b', 'episodes', 'frames', 'first_frame', 'last_frame']
    assert b.values.tolist() == np.stack([ids[seen[ref.pair_a[keep]]], ids[seen[ref.pair_b[keep]]], ref.pair_episodes[keep],
                                          ref.pair_frames[keep], ref.pair_first[keep] + 100, ref.pair_last[keep] + 100], axis=1).tolist()
    h = ct.contact_lifetimes(f, rule.R_ON, rule.R_OFF, gap=2, max_lifetime=25)
    short = rule.contacts(pos[linked], np.concatenate([[0], np.cumsum(sizes)]), dense, rule.R_ON, rule.R_OFF, gap=2, max_lifetime=25,
                          n_particles=len(seen))
    assert h.index.tolist() == list(range(1, 26)) and h.columns.tolist() == ['complete', 'open']
    assert h['complete'].tolist() == short.lifetime_count[0].tolist() and h['open'].tolist() == short.lifetime_count[1].tolist()
    assert (h.attrs['above_complete'], h.attrs['above_open']) == tuple(short.lifetime_above.tolist())
    same = ct.contacts(f, rule.R_ON, rule.R_OFF, gap=2, group_column='cluster', pairs='same')
    assert 0 < len(same) < len(eps) and (same['particle_a'] + 7 == same['particle_b']).all()      # the two of a dimer
