"""Two-point displacement correlations, without a device: the yardstick
``tests/_twopoint.py`` against an independent pair-by-pair loop and on known answers, the identities of the
rule, the unit of the fixed point, the reshaping of the table form, the argument errors of the two calls,
and the stage path of the call -- descriptor before handle, the header's prototype, struct and constants
against ``_lib`` and ``_abi``, the public names."""
import ctypes
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _cases
import _twopoint as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib

tp = importlib.import_module('clustertracking_amd.twopoint')       # ct.twopoint is the function


# ---- the restatement against plain loops ----
def by_pairs(pos, off, particle, lags, cutoff, dr, max_disp, mpp, group=None, pairs='all'):
    """the rule pair by pair with Python floats and integers: (n, sums, n_moved, beyond) as nested lists"""
    N, ndim = len(pos), len(pos[0])
    T = len(off) - 1
    B = int(math.ceil(cutoff / dr))
    edge2 = [(b * dr) * (b * dr) for b in range(B + 1)]
    max2 = max_disp * max_disp
    e = 0
    while 2. ** e < max2:
        e += 1
    while 2. ** (e - 1) >= max2:
        e -= 1
    q = [[float(pos[i][a]) * mpp[a] for a in range(ndim)] for i in range(N)]
    n = [[0] * B for _ in lags]
    sums = [[[0, 0, 0] for _ in range(B)] for _ in lags]
    n_moved, beyond = [0] * len(lags), [0] * len(lags)
    for ki, k in enumerate(lags):
        for t in range(T):
            moved = {}
            for i in range(off[t], off[t + 1]):
                if t + k >= T or particle[i] < 0:
                    continue
                js = [j for j in range(off[t + k], off[t + k + 1]) if particle[j] == particle[i]]
                if not js:
                    continue
                u = [q[js[0]][a] - q[i][a] for a in range(ndim)]
                if not all(math.isfinite(x) for x in u):
                    continue
                u2 = u[0] * u[0]
                for a in range(1, ndim):
                    u2 = u2 + u[a] * u[a]
                if u2 <= max2:
                    moved[i] = (u, u2)
                    n_moved[ki] += 1
                else:
                    beyond[ki] += 1
            for i, (ui, u2i) in moved.items():
                for j, (uj, u2j) in moved.items():
                    if j == i:
                        continue
                    R = [q[j][a] - q[i][a] for a in range(ndim)]
                    d2 = R[0] * R[0]
                    dot, ai, aj = ui[0] * uj[0], ui[0] * R[0], uj[0] * R[0]
                    for a in range(1, ndim):
                        d2 = d2 + R[a] * R[a]
                        dot, ai, aj = dot + ui[a] * uj[a], ai + ui[a] * R[a], aj + uj[a] * R[a]
                    if not 0. < d2 < edge2[B]:
                        continue
                    if pairs != 'all':
                        same = group[i] == group[j] and group[i] >= 0
                        if same != (pairs == 'same'):
                            continue
                    b = max(bb for bb in range(B) if edge2[bb] <= d2)
                    L = (ai * aj) / d2
                    uu = u2i * u2j
                    c = dot / math.sqrt(uu) if uu > 0. else 0.
                    n[ki][b] += 1
                    for s, (x, unit) in enumerate(((dot, 2. ** (e - 40)), (L, 2. ** (e - 40)), (c, 2. ** -40))):
                        sums[ki][b][s] += round(x / unit)              # ties to even
    return n, sums, n_moved, beyond


def _tiny(ndim, seed=4):
    """4 frames of up to 14 rows: an unlinked row, a repeated id, a NaN row, a coincident pair, a big step"""
    pos, off, particle = yard.walkers((14, 12, 14, 9), 6., 0.3, seed, ndim, 14)
    pos, particle = pos.copy(), particle.copy()
    particle[2] = -1
    particle[off[1] + 5] = particle[off[1] + 1]
    pos[4] = np.nan
    pos[off[2] + 3, 0] = np.inf
    pos[8] = pos[9]
    pos[off[1] + 2] += 3.
    group = np.random.RandomState(seed).randint(-1, 3, len(pos)).astype(np.int64)
    return pos, off, particle, group


@pytest.mark.parametrize('ndim', [2, 3])
@pytest.mark.parametrize('pairs', ['all', 'same', 'other'])
def test_restatement_agrees_with_a_loop_over_pairs(ndim, pairs):
    pos, off, particle, group = _tiny(ndim)
    mpp = (0.5, 1., 2.)[:ndim]
    kw = dict(cutoff=3.2, dr=0.5, max_disp=1.25)
    res = yard.twopoint(pos, off, particle, [1, 2, 3], mpp=mpp, group=group, pairs=pairs, **kw)
    n, sums, n_moved, beyond = by_pairs(pos.tolist(), off.tolist(), particle.tolist(), [1, 2, 3], 3.2, 0.5, 1.25, mpp, group.tolist(), pairs)
    assert res.n.tolist() == n and res.sums == sums
    assert res.n_moved.tolist() == n_moved and res.beyond.tolist() == beyond
    assert res.n.shape == (3, 7) and res.r_edges.tolist() == [0.5 * b for b in range(8)] and res.n.sum() > 0
    assert sum(beyond) > 0 and res.unit == 2. ** -39              # 1 < 1.5625 <= 2


def test_evenness_and_same_plus_other():
    pos, off, particle, group = _tiny(2, seed=7)
    kw = dict(cutoff=4., dr=0.25, max_disp=1.5)
    res = {p: yard.twopoint(pos, off, particle, [1, 2], group=group, pairs=p, **kw) for p in ('all', 'same', 'other')}
    for p, r in res.items():
        assert (r.n % 2 == 0).all() and all(v % 2 == 0 for lag in r.sums for cell in lag for v in cell), p
    assert (res['all'].n == res['same'].n + res['other'].n).all()
    assert res['same'].n.sum() > 0 and res['other'].n.sum() > 0
    for k in range(2):
        for b in range(16):
            assert res['all'].sums[k][b] == [x + y for x, y in zip(res['same'].sums[k][b], res['other'].sums[k][b])]
    assert (res['all'].n_moved == res['same'].n_moved).all()          # the rows do not depend on `pairs`


def test_rigid_translation_and_known_answers():
    """every row moves by (0.25, -0.5) per frame: dot = |v|^2 k^2 and cos = 1 in every bin, exactly; along
    the line and across it: two rows on the y axis moving along it are all longitudinal"""
    pos, off, particle = yard.lattice_frames(6, 5, [(0.25, -0.5)] * 3)
    res = yard.twopoint(pos, off, particle, [1, 2, 3], 4., 0.5, 4.)
    assert res.unit == 2. ** -36 and res.n_moved.tolist() == [90, 60, 30] and not res.beyond.any()
    m = yard.means(res.n, yard.words(res.sums), res.unit, 2)
    for ki, k in enumerate((1, 2, 3)):
        has = res.n[ki] > 0
        assert has.sum() == 5 and (m.dot[ki][has] == 0.3125 * k * k).all() and (m.cos[ki][has] == 1.).all()
        assert np.isnan(m.dot[ki][~has]).all() and np.isnan(m.transverse[ki][~has]).all()
        assert all(res.sums[ki][b][2] == int(res.n[ki, b]) << 40 for b in range(8))
        assert np.abs(m.transverse[ki][has] - (m.dot[ki][has] - m.longitudinal[ki][has])).max() <= 2. ** -50
    two = np.array([[0., 0.], [2., 0.], [1., 0.], [3., 0.]])           # both move by +1 along the line between them
    r = yard.twopoint(two, [0, 2, 4], [0, 1, 0, 1], 1, 4., 1., 2.)
    mm = yard.means(r.n, yard.words(r.sums), r.unit, 2)
    assert r.n[0].tolist() == [0, 0, 2, 0] and mm.dot[0, 2] == 1. and mm.longitudinal[0, 2] == 1. and mm.transverse[0, 2] == 0.
    two[2:] = [[0., 1.], [2., 1.]]                                       # ... and across it
    r = yard.twopoint(two, [0, 2, 4], [0, 1, 0, 1], 1, 4., 1., 2.)
    mm = yard.means(r.n, yard.words(r.sums), r.unit, 2)
    assert mm.dot[0, 2] == 1. and mm.longitudinal[0, 2] == 0. and mm.transverse[0, 2] == 1.
    two[3] = [2., -1.]                                                   # opposite ways
    r = yard.twopoint(two, [0, 2, 4], [0, 1, 0, 1], 1, 4., 1., 2.)
    mm = yard.means(r.n, yard.words(r.sums), r.unit, 2)
    assert mm.dot[0, 2] == -1. and mm.cos[0, 2] == -1. and r.sums[0][2][2] == -(2 << 40)


def test_the_unit_at_exact_powers_of_two():
    for max_disp, e in ((2., 2), (1., 0), (0.5, -2), (1.5, 2), (2.0000001, 3), (math.sqrt(2.), 2), (1.4142135623730949, 1), (3., 4), (4., 4)):
        max2, got, unit = yard.fixed_point(max_disp)
        assert max2 == max_disp * max_disp and got == e and unit == 2. ** (e - 40), (max_disp, got)
        assert 2. ** e >= max2 > 2. ** (e - 1)
        assert tp.fixed_point(max_disp) == (max2, e, unit)


def test_words_and_means_of_large_sums():
    big = [[[(1 << 70) + 3, -(1 << 70) - 3, -1]], [[(1 << 63) - 1, -(1 << 63), 1 << 63]]]
    w = yard.words(big)
    assert w.dtype == np.int64 and w.shape == (2, 1, 3, 2) and yard.integers(w) == big
    assert w[0, 0, 0].tolist() == [64, 3] and w[0, 0, 1].tolist() == [-65, -3] and w[0, 0, 2].tolist() == [-1, -1]
    assert w[1, 0, 0].tolist() == [0, (1 << 63) - 1] and w[1, 0, 1].tolist() == [-1, -(1 << 63)] and w[1, 0, 2].tolist() == [0, -(1 << 63)]
    assert yard.as_double((1 << 70) + 3) == 2. ** 70 and yard.as_double(-(1 << 63)) == -2. ** 63 and yard.as_double(1 << 63) == 2. ** 63
    m = yard.means(np.array([[4], [0]]), w, 2. ** -30, 3)
    assert m.dot[0, 0] == 2. ** 38 and m.longitudinal[0, 0] == -2. ** 38 and m.transverse[0, 0] == 2. ** 38 and m.cos[0, 0] == -2. ** -42
    assert all(np.isnan(x[1, 0]) for x in m)


# ---- the table form: its reshaping, on the restatement in place of the engine ----
_linked = yard.linked_table


def _arrays_on_the_yardstick(pos, frame_offset, particle, lagtime, cutoff, dr=0.5, max_disp=None, mpp=1., group=None, pairs='all',
                             n_particles=None, device=0):
    r = yard.twopoint(pos, frame_offset, particle, lagtime, cutoff, dr, max_disp, mpp, group, pairs)
    w = yard.words(r.sums)
    m = yard.means(r.n, w, r.unit, pos.shape[1])
    return tp.TwoPoint(r.r_edges, r.lags, r.n, m.dot, m.longitudinal, m.transverse, m.cos, w, r.n_moved, r.beyond, r.unit, 0)


def test_the_table_form_reshapes(monkeypatch):
    monkeypatch.setattr(tp, 'twopoint_arrays', _arrays_on_the_yardstick)
    f = _linked()
    one = ct.twopoint(f, 1, 4., 1., 2.)
    assert one.index.name == 'r' and one.index.tolist() == [0., 1., 2., 3.]
    assert one.columns.tolist() == ['n', 'dot', 'longitudinal', 'transverse', 'cos']
    assert one['n'].tolist() == [0, 0, 0, 12] and one['n'].dtype == np.int64
    assert one.loc[3., 'dot'] == (0.25 - 0.0625) / 2 and np.isnan(one.loc[0., 'dot'])
    same = ct.twopoint(f, 1, 4., 1., 2., group_column='cluster', pairs='same')
    assert same['n'].tolist() == one['n'].tolist()
    assert ct.twopoint(f, 1, 4., 1., 2., group_column='cluster', pairs='other')['n'].sum() == 0
    many = ct.twopoint(f, [1, 3], 4., 1., 2., mpp=(1., 1.))
    assert many.index.names == ['lag', 'r'] and many.index.tolist() == [(k, r) for k in (1, 3) for r in (0., 1., 2., 3.)]
    assert many.loc[1].equals(one) and many.loc[(3, 3.), 'n'] == 4 and many.loc[(3, 3.), 'dot'] == 9 * (0.25 - 0.0625) / 2
    listed = ct.twopoint(f, [1], 4., 1., 2.)
    assert listed.index.names == ['lag', 'r'] and len(listed) == 4


# ---- argument errors: raised before the engine is looked up ----
POS2, POS3, OFF = np.zeros((4, 2)), np.zeros((4, 3)), np.array([0, 2, 4])
PAR = np.array([0, 1, 0, 1], dtype=np.int64)
BAD_CALLS = {
    'lag_zero': (dict(lagtime=0), 'lagtime'), 'lag_float': (dict(lagtime=1.5), 'lagtime'), 'lag_bool': (dict(lagtime=True), 'lagtime'),
    'lag_text': (dict(lagtime='1'), 'lagtime'), 'lags_empty': (dict(lagtime=[]), 'lagtime'), 'lags_descending': (dict(lagtime=[2, 1]), 'ascending'),
    'lags_repeated': (dict(lagtime=[1, 1]), 'distinct'), 'lags_17': (dict(lagtime=list(range(1, _abi.TP_MAX_LAGS + 2))), '16 lags'),
    'lag_huge': (dict(lagtime=2 ** 31), 'lagtime'),
    'cutoff_zero': (dict(cutoff=0.), 'cutoff'), 'cutoff_nan': (dict(cutoff=float('nan')), 'cutoff'), 'dr_zero': (dict(dr=0.), 'dr'),
    'dr_text': (dict(dr='1'), 'dr'), 'bins_513': (dict(cutoff=513., dr=1.), '512 bins'), 'bins_many': (dict(cutoff=1e6, dr=1.), '512 bins'),
    'max_disp_missing': (dict(max_disp=None), 'max_disp'), 'max_disp_zero': (dict(max_disp=0.), 'max_disp'),
    'max_disp_inf': (dict(max_disp=float('inf')), 'max_disp'), 'max_disp_tiny': (dict(max_disp=1e-200), 'max_disp'),
    'max_disp_huge': (dict(max_disp=1e200), 'max_disp'), 'max_disp_2_251': (dict(max_disp=2. ** 251), 'max_disp'),
    'reach_times_max_disp': (dict(cutoff=2. ** 260, dr=2. ** 252, max_disp=2. ** 245), '2\\^1000'), 'max_disp_text': (dict(max_disp='2'), 'max_disp'),
    'mpp_zero': (dict(mpp=0.), 'mpp'), 'mpp_three_for_2d': (dict(mpp=(1., 1., 1.)), 'mpp'), 'mpp_two_for_3d': (dict(pos=POS3, mpp=(1., 1.)), 'mpp'),
    'pairs_unknown': (dict(pairs='cross', group=PAR), 'pairs'), 'same_without_group': (dict(pairs='same'), 'group'),
    'other_without_group': (dict(pairs='other'), 'group'),
    'group_length': (dict(group=np.zeros(3, dtype=np.int64)), 'group'), 'group_dtype': (dict(group=np.zeros(4)), 'group'),
    'particle_length': (dict(particle=np.zeros(5, dtype=np.int64)), 'particle'), 'particle_dtype': (dict(particle=np.zeros(4)), 'particle'),
    'particle_2d': (dict(particle=np.zeros((4, 1), dtype=np.int64)), 'particle'), 'n_particles_negative': (dict(n_particles=-1), 'n_particles'),
    'pos_1d': (dict(pos=np.zeros(4)), 'pos'), 'pos_4d': (dict(pos=np.zeros((4, 4))), 'pos'), 'pos_text': (dict(pos=np.array([['a', 'b']])), 'pos'),
    'offsets_float': (dict(frame_offset=np.array([0., 4.])), 'frame_offset'), 'offsets_empty': (dict(frame_offset=np.zeros(0, dtype=np.int64)), 'frame_offset'),
}


@pytest.mark.parametrize('name', sorted(BAD_CALLS))
def test_argument_errors_of_the_arrays_form(name, monkeypatch):
    monkeypatch.setattr(_lib, 'default_engine', lambda device=0: pytest.fail('the engine was asked for'))
    extra, word = BAD_CALLS[name]
    kw = dict(pos=POS2, frame_offset=OFF, particle=PAR, lagtime=1, cutoff=4., dr=0.5, max_disp=2.)
    kw.update(extra)
    with pytest.raises(ValueError, match=word):
        ct.twopoint_arrays(**kw)


def test_max_disp_has_no_default():
    with pytest.raises(ValueError, match='max_disp is required'):
        ct.twopoint_arrays(POS2, OFF, PAR, 1, 4.)
    with pytest.raises(TypeError):
        ct.twopoint(_linked(), 1, 4., 1.)


def test_argument_errors_of_the_table_form(monkeypatch):
    monkeypatch.setattr(_lib, 'default_engine', lambda device=0: pytest.fail('the engine was asked for'))
    f = _linked().assign(size=1.5)
    base = dict(lagtime=1, cutoff=4., dr=1., max_disp=2.)
    for kw, word in ((dict(lagtime=0), 'lagtime'), (dict(lagtime=[2, 1]), 'ascending'), (dict(cutoff=-1.), 'cutoff'), (dict(dr=0.), 'dr'),
                     (dict(cutoff=600.), '512 bins'), (dict(max_disp=0.), 'max_disp'), (dict(max_disp=None), 'max_disp'), (dict(mpp=0.), 'mpp'),
                     (dict(pairs='same'), 'group_column'), (dict(pairs='x'), 'pairs'), (dict(group_column='label'), 'label'),
                     (dict(group_column='size'), 'integers'), (dict(pos_columns=['y']), 'pos_columns'), (dict(pos_columns=['y', 'q']), 'pos_columns'),
                     (dict(t_column='t'), "'t'")):
        with pytest.raises(ValueError, match=word):
            ct.twopoint(f, **dict(base, **kw))
    with pytest.raises(ValueError, match='empty'):
        ct.twopoint(f.iloc[:0], **base)
    with pytest.raises(ValueError, match='link it first'):
        ct.twopoint(f.drop(columns='particle'), **base)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the calls would run")
    with pytest.raises(_lib.EngineError):
        ct.twopoint_arrays(POS2, OFF, PAR, 1, 4., max_disp=2.)
    with pytest.raises(_lib.EngineError):
        ct.twopoint(_linked(), 1, 4., 1., 2.)


# ---- the stage path ----
CALL = 'ctr_twopoint_device'


def _descriptor():
    d = _abi.TwoPoint()
    d.ndim, d.pairs, d.n_lags, d.n_bins, d.dr, d.max2 = 2, _abi.PCF_PAIRS_ALL, 2, 8, 0.5, 4.
    d.lag[0], d.lag[1] = 1, 5
    d.mpp[0] = d.mpp[1] = d.mpp[2] = 1.
    for name in ('status', 'frame_offset', 'edge2', 'n', 'dot', 'longitudinal', 'transverse', 'cos', 'sums', 'n_moved', 'beyond'):
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
    assert _refused(_descriptor()) == CALL + ': null handle'
    d = _descriptor()
    d.n_bins, d.n_lags, d.ndim, d.max2 = _abi.TP_MAX_BINS, _abi.TP_MAX_LAGS, 3, 2. ** -500       # the edges that pass
    for k in range(_abi.TP_MAX_LAGS):
        d.lag[k] = k + 1
    assert _refused(d) == CALL + ': null handle'


BAD = [('ndim', 1, 'ndim'), ('ndim', 4, 'ndim'), ('pairs', 3, 'pairs'), ('n_lags', 0, 'n_lags'), ('n_lags', _abi.TP_MAX_LAGS + 1, 'CTR_TP_MAX_LAGS'),
       ('n_bins', 0, 'n_bins'), ('n_bins', _abi.TP_MAX_BINS + 1, 'CTR_TP_MAX_BINS'), ('dr', 0., 'dr'), ('dr', float('inf'), 'dr'),
       ('max2', 0., 'max2'), ('max2', float('nan'), 'max2'), ('max2', float('inf'), 'max2'), ('max2', 2. ** -501, 'max2'), ('max2', 2. ** 501, 'max2'), ('dr', 2. ** 499, 'cutoff squared'),
       ('n_frames', -1, 'negative'), ('n_features', -1, 'negative'), ('n_particles', -1, 'negative'),
       ('n_frames', 2 ** 31 - 2, 'too many'), ('n_features', 2 ** 31, 'too many'), ('n_particles', 2 ** 31 - 1, 'too many'),
       ('status', None, 'null status'), ('frame_offset', None, 'null status'), ('edge2', None, 'edge2'), ('n_features', 1, 'without pos'),
       ('sums', None, 'null output'), ('cos', None, 'null output'), ('beyond', None, 'null output')]


@pytest.mark.parametrize('field,value,word', BAD)
def test_descriptor_is_refused_under_the_entry_point_name(field, value, word):
    d = _descriptor()
    setattr(d, field, value)
    msg = _refused(d)
    assert msg.startswith(CALL + ': ') and word in msg, msg


def test_lags_columns_and_mpp_are_refused():
    for lags, word in (((0, 5), 'a lag must'), ((5, 5), 'ascending'), ((5, 1), 'ascending'), ((1, 2 ** 31 - 2), 'a lag must')):
        d = _descriptor()
        d.lag[0], d.lag[1] = lags
        assert word in _refused(d)
    d = _descriptor()
    d.mpp[1] = 0.
    assert _refused(d) == CALL + ': mpp must be finite and positive'
    d = _descriptor()
    d.n_features, d.pos = 1, 64
    assert _refused(d) == CALL + ': features without particle'
    d.particle, d.pairs = 64, _abi.PCF_PAIRS_OTHER
    assert 'without group' in _refused(d)
    d.group = 64
    assert _refused(d) == CALL + ': null handle'


def test_prototype_signature_constants_and_docs():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    for clause in ('Bins.', 'Scaling and existence.', 'Lags.', 'Partner.', 'Displacement.', 'Pairs.', 'Per pair', 'Fixed point.', 'Sums.',
                   'Means.', 'A refused table.'):
        assert clause in header and clause in tp.__doc__, clause
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', header))
    assert set(protos) == set(_lib.SIGNATURES)
    assert [p.strip() for p in protos[CALL].split(',')] == ['ctr_handle* h', 'const ctr_twopoint* d', 'void* hip_stream']
    assert _lib.SIGNATURES[CALL] == _lib._stage(_abi.TwoPoint) and CALL in _lib.EXPORTS
    assert hasattr(_lib.load(), CALL) and callable(_lib.Engine.twopoint_device)
    body = re.search(r'typedef struct ctr_twopoint \{(.*?)\} ctr_twopoint;', header, flags=re.S).group(1)
    assert re.findall(r'\b(\w+)(?:\[\w+\])?\s*;', body) == [f[0] for f in _abi.TwoPoint._fields_]
    defines = dict(re.findall(r'#define\s+(CTR_TP_\w+)\s+(\d+)', header))
    assert defines == {'CTR_TP_OK': '0', 'CTR_TP_BAD_TABLE': '1', 'CTR_TP_MAX_BINS': '512', 'CTR_TP_MAX_LAGS': '16'}
    assert (_abi.TP_OK, _abi.TP_BAD_TABLE, _abi.TP_MAX_BINS, _abi.TP_MAX_LAGS) == (0, 1, 512, 16)


def test_struct_layout_matches_the_compiler(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_twopoint));\n'
    expect = [ctypes.sizeof(_abi.TwoPoint)]
    for f, _ in _abi.TwoPoint._fields_:
        src += 'printf("%%zu\\n", offsetof(ctr_twopoint, %s));\n' % f
        expect.append(getattr(_abi.TwoPoint, f).offset)
    src += 'return 0;}\n'
    (tmp_path / 'layout.c').write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == expect


def test_public_names_and_docstrings():
    assert {'twopoint_arrays', 'twopoint'} <= set(ct.__all__)
    assert ct.twopoint is tp.twopoint and ct.twopoint_arrays is tp.twopoint_arrays
    assert tp.TwoPoint._fields == ('r_edges', 'lags', 'n', 'dot', 'longitudinal', 'transverse', 'cos', 'sums', 'n_moved', 'beyond',
                                   'unit', 'status')
    doc = tp.twopoint.__doc__
    assert 'Subtract the drift first' in doc and 'velocity_corr' in doc and 'direction_corr' in doc
    for word in ('binned', 'pooled over all frames', 'ordered', 'any lag', 'max_disp', 'not pinned', 'not a dependency'):
        assert word in doc, word
    assert 'Subtract the drift first' in tp.twopoint_arrays.__doc__
