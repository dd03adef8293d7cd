"""The contact rule (clustertracking_amd/contacts.py, include/ctrefine.h) on the CPU: the restatement of
tests/_contacts.py against expectations written by hand, the identities that follow from the rule on a
random table, every argument error of the public calls (raised before the engine is looked up), and the
stage path of the call -- descriptor before handle, the header's prototype, struct and constants, and
ctr_contacts_plan.  No device."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import _cases
import _contacts as rule
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib

con = importlib.import_module('clustertracking_amd.contacts')      # ct.contacts is the function


def two(dists, others=()):
    """particle 0 at the origin in every frame and particle 1 at distance ``dists[t]`` along x (None: it is
    missing); others: ``(frame, particle, (y, x))`` rows appended to their frames"""
    pos, particle, off = [], [], [0]
    for t, dist in enumerate(dists):
        pos.append((0., 0.))
        particle.append(0)
        if dist is not None:
            pos.append((0., float(dist)))
            particle.append(1)
        for frame, p, at in others:
            if frame == t:
                pos.append(at)
                particle.append(p)
        off.append(len(pos))
    return np.array(pos, dtype=np.float64).reshape(-1, 2), np.array(off, dtype=np.int64), np.array(particle, dtype=np.int64)


def episodes(res):
    return [tuple(getattr(res, name)[x].item() for name in rule.EPISODE) for x in range(res.n_episodes)]


ON, BAND, FAR = 1., 3., 9.          # with r_on = 2 and r_off = 4


def test_band_band_on_band_far():
    res = rule.contacts(*two([BAND, BAND, ON, BAND, FAR]), 2., 4.)
    assert (res.n_entries, res.duplicates, res.n_episodes, res.n_pairs, res.status) == (4, 0, 1, 1, 0)
    # begins at the first entry below r_on, ends at the chain's last entry: complete, and not left_open
    assert episodes(res) == [(0, 1, 2, 3, 2, 2, False, False, 1., 9.)]
    assert res.formed.tolist() == [0, 0, 1, 0, 0] and res.broken.tolist() == [0, 0, 0, 0, 1]
    assert res.active.tolist() == [0, 0, 1, 1, 0]
    assert res.lifetime_count.tolist() == [[0, 1, 0, 0, 0], [0, 0, 0, 0, 0]] and res.lifetime_above.tolist() == [0, 0]
    assert [getattr(res, n).tolist() for n in rule.PAIR] == [[0], [1], [1], [2], [2], [3]]
    assert res.first_seen.tolist() == [0, 0] and res.last_seen.tolist() == [4, 4]


def test_without_hysteresis_the_band_ends_the_contact():
    res = rule.contacts(*two([FAR, ON, BAND, ON, FAR]), 2.)
    assert [e[2:6] for e in episodes(res)] == [(1, 1, 1, 1), (3, 3, 1, 1)]
    assert res.pair_episodes.tolist() == [2] and res.pair_frames.tolist() == [2]
    assert (res.pair_first.tolist(), res.pair_last.tolist()) == ([1], [3])
    res = rule.contacts(*two([FAR, ON, BAND, ON, FAR]), 2., 4.)
    assert [e[2:6] for e in episodes(res)] == [(1, 3, 3, 3)]


@pytest.mark.parametrize('between', [None, FAR], ids=['missing', 'apart'])
def test_a_gap_of_exactly_gap_frames_is_bridged(between):
    table = two([FAR, FAR, FAR, ON, between, between, ON, FAR, FAR, FAR])
    one = rule.contacts(*table, 2., 4., gap=2)
    # bridged frames count in the lifetime and not in n_seen
    assert [e[2:] for e in episodes(one)] == [(3, 6, 4, 2, False, False, 1., 1.)]
    assert one.active.tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    assert one.formed.nonzero()[0].tolist() == [3] and one.broken.nonzero()[0].tolist() == [7]
    split = rule.contacts(*table, 2., 4., gap=1)
    assert [e[2:] for e in episodes(split)] == [(3, 3, 1, 1, False, False, 1., 1.), (6, 6, 1, 1, False, False, 1., 1.)]
    assert split.active.tolist() == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0]
    assert split.formed.nonzero()[0].tolist() == [3, 6] and split.broken.nonzero()[0].tolist() == [4, 7]


def test_open_at_the_first_and_last_frame_of_the_table():
    res = rule.contacts(*two([ON, ON, ON]), 2., 4.)
    assert episodes(res) == [(0, 1, 0, 2, 3, 3, True, True, 1., 1.)]
    assert res.formed.sum() == 0 and res.broken.sum() == 0 and res.active.tolist() == [1, 1, 1]
    assert res.lifetime_count.tolist() == [[0, 0, 0], [0, 0, 1]]


def test_open_at_a_particles_own_first_and_last_frame():
    res = rule.contacts(*two([None, None, ON, ON, ON, None, None]), 2., 4.)
    assert res.first_seen.tolist() == [0, 2] and res.last_seen.tolist() == [6, 4]
    assert episodes(res) == [(0, 1, 2, 4, 3, 3, True, True, 1., 1.)]
    # one frame apart first: the contact begins after particle 1 was seen, and ends before it was last seen
    res = rule.contacts(*two([None, FAR, ON, ON, ON, FAR, None]), 2., 4.)
    assert episodes(res) == [(0, 1, 2, 4, 3, 3, False, False, 1., 1.)]
    assert res.formed.tolist() == [0, 0, 1, 0, 0, 0, 0] and res.broken.tolist() == [0, 0, 0, 0, 0, 1, 0]
    res = rule.contacts(*two([None, FAR, ON, ON, ON, FAR, None]), 2., 4., gap=1)     # ... but within the gap of both
    assert episodes(res) == [(0, 1, 2, 4, 3, 3, True, True, 1., 1.)]


def test_a_chain_that_begins_in_the_band_is_not_left_open():
    res = rule.contacts(*two([BAND, ON, ON, FAR, FAR, FAR]), 2., 4., gap=1)
    assert episodes(res) == [(0, 1, 1, 2, 2, 2, False, False, 1., 1.)]      # first - first_seen = 1 <= gap, yet it was seen forming
    res = rule.contacts(*two([ON, ON, ON, FAR, FAR, FAR]), 2., 4., gap=1)
    assert episodes(res)[0][6:8] == (True, False)


def test_a_repeated_particle_the_first_entry_counts():
    near_first = two([ON, ON], others=[(0, 1, (0., 3.))])                   # rows of frame 0: p0, p1 at 1, p1 at 3
    res = rule.contacts(*near_first, 2., 4.)
    assert (res.n_entries, res.duplicates) == (3, 1)
    assert episodes(res) == [(0, 1, 0, 1, 2, 2, True, True, 1., 1.)]
    pos, off, par = near_first
    pos[[1, 2]] = pos[[2, 1]]                                               # ... p1 at 3 first: frame 0 is band only
    res = rule.contacts(pos, off, par, 2., 4.)
    assert (res.n_entries, res.duplicates) == (3, 1)
    assert episodes(res) == [(0, 1, 1, 1, 1, 1, False, True, 1., 1.)]
    # the repeated particle as the smaller id: two rows i with one j
    res = rule.contacts(*two([ON, ON], others=[(1, 0, (0., 1.))]), 2., 4.)
    assert (res.n_entries, res.duplicates, res.n_episodes) == (3, 1, 1) and res.min_d2.tolist() == [1.]      # not the duplicate's 0


def test_coincident_rows_are_in_contact():
    res = rule.contacts(*two([0., 0.]), 2.)
    assert episodes(res) == [(0, 1, 0, 1, 2, 2, True, True, 0., 0.)]


def test_a_particle_that_never_takes_part():
    pos, off, par = two([ON, ON, ON], others=[(0, 2, (0., np.nan)), (2, 2, (np.inf, 0.)), (1, -1, (0., 0.5))])
    res = rule.contacts(pos, off, par, 2., 4.)
    assert res.first_seen.tolist() == [0, 0, 3] and res.last_seen.tolist() == [2, 2, -1]
    assert res.n_entries == 3 and res.n_pairs == 1                          # the unlinked row at 0.5 is nobody's contact
    res = rule.contacts(pos, off, par, 2., 4., n_particles=5)
    assert res.first_seen.tolist() == [0, 0, 3, 3, 3] and res.n_entries == 3


def test_entries_lie_in_frame_i_j_order_and_mpp_scales():
    pos = np.array([[0., 0.], [0., 1.], [0., 2.], [0., 0.], [0., 1.]])
    off, par = np.array([0, 3, 5]), np.array([2, 0, 1, 1, 0])
    a, b, frame, d2, takes = rule.entries(pos, off, par, 4.)
    assert (a.tolist(), b.tolist(), frame.tolist(), d2.tolist()) == ([0, 0, 1, 0], [2, 1, 2, 1], [0, 0, 0, 1], [1., 1., 4., 1.])
    assert takes.all()
    assert rule.entries(pos, off, par, 4., mpp=(1., 3.))[3].tolist() == [9., 9., 9.]
    group = np.array([7, 7, 8, -1, -1])
    assert rule.entries(pos, off, par, 4., group=group, pairs='same')[3].tolist() == [1.]
    assert rule.entries(pos, off, par, 4., group=group, pairs='other')[3].tolist() == [1., 4., 1.]      # -1 is no group


def test_the_long_chain_by_hand():
    pos, off, par, want = rule.long_chain()
    res = rule.contacts(pos, off, par, rule.LONG_R_ON, rule.LONG_R_OFF, gap=rule.LONG_GAP)
    assert episodes(res) == want
    assert res.n_entries == rule.LONG_T - 3 - 3 - 1 and res.duplicates == 0
    assert res.formed.nonzero()[0].tolist() == [502, 1206] and res.broken.nonzero()[0].tolist() == [500, 1200]


@pytest.fixture(scope='module')
def mixed():
    return rule.mixed_table(2)


def test_the_mixed_table_is_what_its_text_says(mixed):
    pos, off, par, group, P = mixed
    sizes = np.diff(off)
    assert len(sizes) == 40 and sizes[7] == 600 and sizes[3] == sizes[20] == 0
    assert all(30 <= s <= 60 for t, s in enumerate(sizes) if t not in (3, 7, 20))
    assert np.isnan(pos).any(1).sum() == 3 and (par < 0).sum() > 100 and par.max() + 1 == P
    assert (par[off[12]:off[13]] == 4).sum() == 2
    res = rule.contacts(pos, off, par, rule.R_ON, rule.R_OFF, gap=2)
    assert res.duplicates > 0 and res.n_episodes > 20 and (res.lifetime > 30).sum() >= 5
    assert res.left_open.any() and res.right_open.any() and (~res.left_open & ~res.right_open).any()


def test_identities(mixed):
    pos, off, par, group, P = mixed
    counts = []
    for r_off, gap in ((rule.R_ON, 0), (rule.R_OFF, 0), (rule.R_OFF, 1), (rule.R_OFF, 2), (rule.R_OFF, 5)):
        res = rule.contacts(pos, off, par, rule.R_ON, r_off, gap=gap, max_lifetime=10)
        assert res.lifetime.sum() == res.active.sum()
        assert res.formed.sum() == (~res.left_open).sum() and res.broken.sum() == (~res.right_open).sum()
        assert res.lifetime_count.sum() + res.lifetime_above.sum() == res.n_episodes
        assert res.lifetime_above.sum() == (res.lifetime > 10).sum()
        assert res.pair_frames.sum() == res.lifetime.sum() and res.pair_episodes.sum() == res.n_episodes
        assert (res.a < res.b).all() and (res.n_seen <= res.lifetime).all() and (res.min_d2 <= res.max_d2).all()
        key = list(zip(res.a.tolist(), res.b.tolist(), res.first.tolist()))
        assert key == sorted(key) and len(set(key)) == len(key)
        counts.append(res.n_episodes)
    assert counts[1] >= counts[2] >= counts[3] >= counts[4]                 # the episodes do not rise with the gap
    n = {pairs: rule.contacts(pos, off, par, rule.R_ON, rule.R_OFF, group=group, pairs=pairs).n_entries
         for pairs in ('all', 'same', 'other')}
    assert n['all'] == n['same'] + n['other'] and n['same'] > 0 and n['other'] > 0


# ---- argument errors: raised before the engine is looked up ----
POS2, POS3, OFF = np.zeros((4, 2)), np.zeros((4, 3)), np.array([0, 2, 4])
PAR = np.array([0, 1, 0, 1], dtype=np.int64)
BAD_CALLS = {
    'r_on_zero': (dict(r_on=0.), 'r_on'), 'r_on_negative': (dict(r_on=-1.), 'r_on'), 'r_on_nan': (dict(r_on=float('nan')), 'r_on'),
    'r_on_text': (dict(r_on='2'), 'r_on'), 'r_off_below_r_on': (dict(r_off=1.5), 'r_off'), 'r_off_inf': (dict(r_off=float('inf')), 'r_off'),
    'r_off_huge': (dict(r_off=1e200), 'squares'),
    'gap_negative': (dict(gap=-1), 'gap'), 'gap_float': (dict(gap=1.5), 'gap'), 'gap_bool': (dict(gap=True), 'gap'),
    'gap_text': (dict(gap='1'), 'gap'), 'gap_none': (dict(gap=None), 'gap'), 'gap_huge': (dict(gap=2 ** 31), 'gap'),
    'pairs_unknown': (dict(pairs='cross', group=PAR), 'pairs'), 'same_without_group': (dict(pairs='same'), 'group'),
    'other_without_group': (dict(pairs='other'), 'group'),
    'max_lifetime_zero': (dict(max_lifetime=0), 'max_lifetime'), 'max_lifetime_above': (dict(max_lifetime=2 ** 20 + 1), 'max_lifetime'),
    'max_lifetime_float': (dict(max_lifetime=2.5), 'max_lifetime'), 'max_lifetime_bool': (dict(max_lifetime=True), 'max_lifetime'),
    'max_entries_negative': (dict(max_entries=-1), 'max_entries'), 'max_entries_float': (dict(max_entries=1.5), 'max_entries'),
    'n_particles_negative': (dict(n_particles=-1), 'n_particles'), 'n_particles_2_31': (dict(n_particles=2 ** 31), 'particles'),
    'mpp_zero': (dict(mpp=0.), 'mpp'), 'mpp_three_for_2d': (dict(mpp=(1., 1., 1.)), 'mpp'), 'mpp_two_for_3d': (dict(pos=POS3, mpp=(1., 1.)), 'mpp'),
    'group_length': (dict(group=np.zeros(3, dtype=np.int64)), 'group'), 'group_dtype': (dict(group=np.zeros(4)), 'group'),
    'particle_length': (dict(particle=np.zeros(5, dtype=np.int64)), 'particle'), 'particle_dtype': (dict(particle=np.zeros(4)), 'particle'),
    'pos_1d': (dict(pos=np.zeros(4)), 'pos'), 'pos_4d': (dict(pos=np.zeros((4, 4))), 'pos'),
    'offsets_float': (dict(frame_offset=np.array([0., 4.])), 'frame_offset'), 'offsets_empty': (dict(frame_offset=np.zeros(0, dtype=np.int64)), 'frame_offset'),
}


@pytest.mark.parametrize('name', sorted(BAD_CALLS))
def test_argument_errors_of_the_arrays_form(name, monkeypatch):
    monkeypatch.setattr(_lib, 'default_engine', lambda device=0: pytest.fail('the engine was asked for'))
    extra, word = BAD_CALLS[name]
    kw = dict(pos=POS2, frame_offset=OFF, particle=PAR, r_on=2.)
    kw.update(extra)
    with pytest.raises(ValueError, match=word):
        ct.contacts_arrays(**kw)


def _linked():
    return pd.DataFrame({'y': [0., 0., 0., 0.], 'x': [0., 1., 0., 1.], 'frame': [3, 3, 4, 4], 'particle': [10, 20, 10, 20],
                         'cluster': [0, 0, 0, 0]})


def test_argument_errors_of_the_table_forms(monkeypatch):
    monkeypatch.setattr(_lib, 'default_engine', lambda device=0: pytest.fail('the engine was asked for'))
    f = _linked().assign(size=1.5)
    for call in (ct.contacts, ct.bonds, ct.contact_lifetimes):
        for kw, word in ((dict(r_on=0.), 'r_on'), (dict(r_off=1.), 'r_off'), (dict(gap=-1), 'gap'), (dict(gap=0.5), 'gap'), (dict(mpp=0.), 'mpp'),
                         (dict(pairs='same'), 'group_column'), (dict(pairs='x'), 'pairs'), (dict(group_column='label'), 'label'),
                         (dict(group_column='size'), 'integers'), (dict(pos_columns=['y']), 'pos_columns'), (dict(t_column='t'), "'t'")):
            with pytest.raises(ValueError, match=word):
                call(f, **dict(dict(r_on=2.), **kw))
        with pytest.raises(ValueError, match='empty'):
            call(f.iloc[:0], 2.)
        with pytest.raises(ValueError, match='link it first'):
            call(f.drop(columns='particle'), 2.)
    with pytest.raises(ValueError, match='min_frames'):
        ct.bonds(f, 2., min_frames=0)
    with pytest.raises(ValueError, match='max_lifetime'):
        ct.contact_lifetimes(f, 2., max_lifetime=0)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the calls would run")
    with pytest.raises(_lib.EngineError):
        ct.contacts_arrays(POS2, OFF, PAR, 2.)
    with pytest.raises(_lib.EngineError):
        ct.contacts(_linked(), 2.)


def _arrays_on_the_yardstick(pos, frame_offset, particle, r_on, r_off=None, gap=0, mpp=1., group=None, pairs='all',
                             max_lifetime=None, n_particles=None, max_entries=None, device=0):
    return rule.contacts(pos, frame_offset, particle, r_on, r_off, gap, mpp, group, pairs, max_lifetime, n_particles)


def test_the_table_forms_carry_the_tables_ids_and_frames(monkeypatch):
    monkeypatch.setattr(con, 'contacts_arrays', _arrays_on_the_yardstick)
    f = pd.DataFrame({'y': 0., 'x': [0., 1., 50., 0., 3., 0., 9., 0., 1.], 'frame': [5, 5, 5, 6, 6, 7, 7, 9, 9],
                      'particle': [30, 10, 20, 30, 10, 30, 10, 30, 10]})
    f = f.sample(frac=1., random_state=1)
    eps = ct.contacts(f, 2., 4.)
    assert eps.columns.tolist() == ['particle_a', 'particle_b', 'first_frame', 'last_frame', 'lifetime', 'n_seen', 'left_open',
                                    'right_open', 'min_dist', 'max_dist']
    assert eps.values.tolist() == [[10, 30, 5, 6, 2, 2, True, False, 1., 3.], [10, 30, 9, 9, 1, 1, False, True, 1., 1.]]
    assert eps.attrs == {'n_entries': 3, 'duplicates': 0, 'n_episodes': 2, 'n_pairs': 1}
    b = ct.bonds(f, 2., 4.)
    assert b.columns.tolist() == ['particle_a', 'particle_b', 'episodes', 'frames', 'first_frame', 'last_frame']
    assert b.values.tolist() == [[10, 30, 2, 3, 5, 9]]
    assert len(ct.bonds(f, 2., 4., min_frames=3)) == 1 and len(ct.bonds(f, 2., 4., min_frames=4)) == 0
    assert ct.bonds(f, 2., 4., gap=2).values.tolist() == [[10, 30, 1, 5, 5, 9]]
    h = ct.contact_lifetimes(f, 2., 4.)
    assert h.index.name == 'lifetime' and h.index.tolist() == [1, 2, 3, 4, 5] and h.columns.tolist() == ['complete', 'open']
    assert h['complete'].tolist() == [0] * 5 and h['open'].tolist() == [1, 1, 0, 0, 0]
    h = ct.contact_lifetimes(f, 2., 4., max_lifetime=1)
    assert h['open'].tolist() == [1] and h.attrs['above_open'] == 1 and h.attrs['above_complete'] == 0


# ---- the stage path ----
CALL = 'ctr_contacts_device'


def _descriptor(phase=_abi.CON_EPISODES):
    d = con.descriptor(phase, 2, 'all', 0, 0, 0, 4., 16., 0, (1., 1.), 1, 0)
    for name in ('status', 'n_entries', 'frame_offset', 'entry_start', 'lifetime_count', 'lifetime_above', 'duplicates', 'n_episodes',
                 'n_pairs'):
        setattr(d, name, 64)                  # never dereferenced: there is no handle
    return d


def _refused(d):
    lib = _lib.load()
    assert getattr(lib, CALL)(None, ctypes.byref(d), None) == _abi.ERR_INVALID
    return (lib.ctr_last_error(None) or b'').decode()


def test_descriptor_then_handle():
    lib = _lib.load()
    assert getattr(lib, CALL)(None, None, None) == _abi.ERR_INVALID
    assert (lib.ctr_last_error(None) or b'').decode() == CALL + ': null descriptor'
    for phase in (_abi.CON_COUNT, _abi.CON_FILL, _abi.CON_EPISODES):
        assert _refused(_descriptor(phase)) == CALL + ': null handle'
    d = _descriptor()
    d.max_lifetime, d.gap, d.off2, d.ndim = _abi.CON_MAX_LIFETIME, 2 ** 31 - 1, 4., 3          # the edges that pass
    d.mpp[2] = 1.
    assert _refused(d) == CALL + ': null handle'


BAD = [('phase', 3, 'phase'), ('ndim', 1, 'ndim'), ('ndim', 4, 'ndim'), ('pairs', 3, 'pairs'), ('gap', -1, 'gap'), ('gap', 2 ** 31, 'gap'),
       ('on2', 0., 'on2'), ('on2', float('nan'), 'on2'), ('off2', 3., 'on2'), ('off2', float('inf'), 'on2'),
       ('max_lifetime', 0, 'max_lifetime'), ('max_lifetime', _abi.CON_MAX_LIFETIME + 1, 'CTR_CON_MAX_LIFETIME'),
       ('n_frames', -1, 'negative'), ('n_features', -1, 'negative'), ('n_particles', -1, 'negative'), ('max_entries', -1, 'negative'),
       ('n_frames', 2 ** 31 - 2, 'too many'), ('n_features', 2 ** 31, 'too many'), ('n_particles', 2 ** 31, 'too many'),
       ('max_entries', 2 ** 40 + 1, '2^40'),
       ('status', None, 'null status'), ('n_entries', None, 'null status'), ('n_particles', 1, 'first_seen'),
       ('max_entries', 1, 'key, frame or d2'), ('n_frames', 1, 'formed'), ('n_pairs', None, 'null output'),
       ('lifetime_count', None, 'null output')]


@pytest.mark.parametrize('field,value,word', BAD)
def test_descriptor_is_refused_under_the_entry_point_name(field, value, word):
    d = _descriptor()
    setattr(d, field, value)
    msg = _refused(d)
    assert msg.startswith(CALL + ': ') and word in msg, msg


def test_columns_of_the_phases_are_refused():
    d = _descriptor(_abi.CON_COUNT)
    d.entry_start = None
    assert 'entry_start' in _refused(d)
    d = _descriptor(_abi.CON_COUNT)
    d.n_features = 1
    assert _refused(d) == CALL + ': features without pos'
    d.pos = 64
    assert _refused(d) == CALL + ': features without particle'
    d.particle, d.pairs = 64, _abi.PCF_PAIRS_SAME
    assert 'without group' in _refused(d)
    d.group = 64
    assert _refused(d) == CALL + ': null handle'
    d = _descriptor(_abi.CON_EPISODES)
    d.max_entries = 1
    d.key = d.frame = d.d2 = 64
    assert 'episode columns' in _refused(d)
    for name in rule.EPISODE:
        setattr(d, name, 64)
    assert 'pair columns' in _refused(d)
    d.mpp[0] = 0.
    assert _refused(d) == CALL + ': mpp must be finite and positive'


def test_prototype_signature_constants_and_docs():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8     # an addition, not a new ABI
    for clause in ('1. Inputs.', '2. Thresholds.', '3. Entries.', '4. Pair order.', '5. Duplicates.', '6. Chains.', '7. Episodes.',
                   '8. Censoring.', '9. Series', '10. Lifetimes.', '11. Pairs.', '12. A refused table.', '13. Capacity.'):
        assert clause in header and clause in con.__doc__, clause
    assert 'whether one of the two' in header and 'whether one of the two' in con.__doc__      # what a gap bridges, said plainly
    assert 'Bytes that a call allocates per entry' in header
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', header))
    assert set(protos) == set(_lib.SIGNATURES)
    assert [p.strip() for p in protos[CALL].split(',')] == ['ctr_handle* h', 'const ctr_contacts* d', 'void* hip_stream']
    assert [p.strip() for p in protos['ctr_contacts_plan'].split(',')] == ['const ctr_contacts* d', 'int64_t* scratch_bytes',
                                                                            'int64_t* scan_tiles', 'int64_t* grids']
    assert _lib.SIGNATURES[CALL] == _lib._stage(_abi.Contacts) and CALL in _lib.EXPORTS
    assert hasattr(_lib.load(), CALL) and callable(_lib.Engine.contacts_device)
    body = re.search(r'typedef struct ctr_contacts \{(.*?)\} ctr_contacts;', header, flags=re.S).group(1)
    assert re.findall(r'\b(\w+)(?:\[\w+\])?\s*;', body) == [f[0] for f in _abi.Contacts._fields_]
    defines = dict(re.findall(r'#define\s+(CTR_CON_\w+)\s+(\d+)', header))
    assert defines == {'CTR_CON_COUNT': '0', 'CTR_CON_FILL': '1', 'CTR_CON_EPISODES': '2', 'CTR_CON_OK': '0', 'CTR_CON_BAD_TABLE': '1',
                       'CTR_CON_OVERFLOW': '2', 'CTR_CON_MAX_LIFETIME': str(2 ** 20)}
    assert (_abi.CON_COUNT, _abi.CON_FILL, _abi.CON_EPISODES, _abi.CON_OK, _abi.CON_BAD_TABLE, _abi.CON_OVERFLOW,
            _abi.CON_MAX_LIFETIME) == (0, 1, 2, 0, 1, 2, 2 ** 20)
    assert (rule.OK, rule.BAD_TABLE, rule.OVERFLOW) == (_abi.CON_OK, _abi.CON_BAD_TABLE, _abi.CON_OVERFLOW)


def test_struct_layout_matches_the_compiler(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_contacts));\n'
    expect = [ctypes.sizeof(_abi.Contacts)]
    for f, _ in _abi.Contacts._fields_:
        src += 'printf("%%zu\\n", offsetof(ctr_contacts, %s));\n' % f
        expect.append(getattr(_abi.Contacts, f).offset)
    src += 'return 0;}\n'
    (tmp_path / 'layout.c').write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == expect


def _plan(n_frames, n_features, n_particles, max_entries, phase=_abi.CON_EPISODES):
    return _lib.contacts_plan(con.descriptor(phase, 2, 'all', n_frames, n_features, n_particles, 4., 16., 0, (1., 1.), 1, max_entries))


def test_the_plan_answers_without_a_device():
    up = lambda b: (b + 255) // 256 * 256
    empty = _plan(0, 0, 0, 0)
    assert empty.scan_tiles == (0, 0) and empty.grids == (1, 0, 1, 1)
    assert empty.scratch_bytes == 4 * up(8)                                 # item_start, diff, one sum, the word of the chains
    p = _plan(40, 2355, 600, 5000)
    assert p.scan_tiles == (10, 20) and p.grids == (10, 40 + 2355 // 256, 20, 1250)
    assert p.scratch_bytes == 2 * up(8 * 41) + up(8 * (5000 // 256 + 1)) + up(8) + 7 * up(8 * 5000)
    # 300 rows in each of three frames with every pair an entry: more than 256 tiles, so the scan of the sums takes trips
    p = _plan(6, 1500, 300, 3 * 44850)
    assert p.scan_tiles == (6, 526) and p.grids[2] == 526 and p.grids[3] == (3 * 44850 + 3) // 4
    big = _plan(10, 2 ** 24, 1000, 2 ** 26)
    assert big.grids == (65536, 65536, 65536, 65536) and big.scan_tiles == (2 ** 16, 2 ** 18)      # capped: the kernels stride
    count = _plan(40, 2355, 600, 0, _abi.CON_COUNT)
    assert count.scan_tiles == (10, 0) and count.scratch_bytes == 2 * up(8 * 41) + up(8 * (2355 // 256 + 1)) + up(8)
    with pytest.raises(ValueError, match='ctr_contacts_plan: ndim'):
        _lib.contacts_plan(con.descriptor(_abi.CON_COUNT, 4, 'all', 1, 1, 1, 4., 16., 0, (1., 1., 1.)))


def test_public_names_and_docstrings():
    assert {'contacts_arrays', 'contacts', 'bonds', 'contact_lifetimes'} <= set(ct.__all__)
    assert ct.contacts is con.contacts and ct.contacts_arrays is con.contacts_arrays and ct.bonds is con.bonds
    assert list(con.Contacts._fields) == rule.FIELDS
    doc = con.contacts_arrays.__doc__
    for word in ('one synchronisation', 'nothing is read back and nothing waits', 'CON_OVERFLOW', 'stably', 'bytes per entry'):
        assert word in doc, word
    assert 'no CPU fallback' in con.__doc__ and 'Schmitt trigger' in con.__doc__
