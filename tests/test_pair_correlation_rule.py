"""Pair correlation function g(r), without a device: the argument errors of the two
calls, the yardstick ``tests/_pair_correlation.py`` on known answers (the arc fraction against Monte
Carlo, a square lattice, an ideal gas, a plain double loop), and the stage path of the call --
descriptor before handle, the header's prototype, struct and constants against ``_lib`` and ``_abi``,
the ABI version and the public names."""
import bisect
import ctypes
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import _cases
import _pair_correlation as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib
from clustertracking_amd import static as st


# ---- argument errors: raised before the engine is looked up ----
POS2, POS3, OFF = np.zeros((4, 2)), np.zeros((4, 3)), np.array([0, 2, 4])
GROUP = np.zeros(4, dtype=np.int64)
BAD_CALLS = {
    'cutoff_zero': (dict(cutoff=0.), 'cutoff'), 'cutoff_negative': (dict(cutoff=-1.), 'cutoff'),
    'cutoff_nan': (dict(cutoff=float('nan')), 'cutoff'), 'cutoff_inf': (dict(cutoff=float('inf')), 'cutoff'),
    'cutoff_text': (dict(cutoff='4'), 'cutoff'), 'cutoff_bool': (dict(cutoff=True), 'cutoff'),
    'dr_zero': (dict(dr=0.), 'dr'), 'dr_negative': (dict(dr=-0.5), 'dr'), 'dr_nan': (dict(dr=float('nan')), 'dr'),
    'dr_inf': (dict(dr=float('inf')), 'dr'),
    'too_many_bins': (dict(cutoff=_abi.PCF_MAX_BINS + 0.5, dr=1.), 'bins'),
    'mpp_zero': (dict(mpp=0.), 'mpp'), 'mpp_negative': (dict(mpp=(1., -1.)), 'mpp'), 'mpp_nan': (dict(mpp=float('nan')), 'mpp'),
    'mpp_inf': (dict(mpp=(float('inf'), 1.)), 'mpp'), 'mpp_three_for_2d': (dict(mpp=(1., 1., 1.)), 'mpp'),
    'edge_unknown': (dict(edge='cap'), 'edge'), 'edge_none_object': (dict(edge=None), 'edge'),
    'arc_in_3d': (dict(pos=POS3, edge='arc'), 'arc'),
    'pairs_unknown': (dict(pairs='cross', group=GROUP), 'pairs'),
    'same_without_group': (dict(pairs='same'), 'group'), 'other_without_group': (dict(pairs='other'), 'group'),
    'boundary_shape': (dict(boundary=[[0., 0., 0.], [1., 1., 1.]]), 'boundary'), 'boundary_flat': (dict(boundary=[0., 0., 1., 1.]), 'boundary'),
    'boundary_hi_below_lo': (dict(boundary=[[0., 5.], [9., 4.]]), 'boundary'),
    'group_length': (dict(group=np.zeros(3, dtype=np.int64)), 'group'), 'group_dtype': (dict(group=np.zeros(4)), 'group'),
    'group_2d': (dict(group=np.zeros((4, 1), dtype=np.int64)), 'group'),
    'pos_1d': (dict(pos=np.zeros(4)), 'pos'), 'pos_4d': (dict(pos=np.zeros((4, 4))), 'pos'),
    'offsets_float': (dict(frame_offset=np.array([0., 4.])), 'frame_offset'),
}


@pytest.mark.parametrize('name', sorted(BAD_CALLS))
def test_argument_errors_of_the_arrays_form(name):
    extra, word = BAD_CALLS[name]
    kw = dict(pos=POS2, frame_offset=OFF, cutoff=4.)
    kw.update(extra)
    with pytest.raises(ValueError, match=word):
        ct.pair_correlation_arrays(**kw)


def test_the_cap_itself_is_no_argument_error():
    """B = PCF_MAX_BINS passes the checks: what is raised is about the engine or nothing"""
    r_edges, edge2, shell = st.bins(float(_abi.PCF_MAX_BINS), 1., 2)
    assert len(shell) == _abi.PCF_MAX_BINS and len(r_edges) == len(edge2) == _abi.PCF_MAX_BINS + 1
    assert len(st.bins(10.2, 0.5, 2)[2]) == 21          # a cutoff that is no multiple of dr: the last bin reaches past it


def test_argument_errors_of_the_table_form():
    f = pd.DataFrame({'frame': [0, 0, 1, 1], 'y': [0., 1., 2., 3.], 'x': [0., 1., 2., 3.], 'cluster': [0, 0, 1, 1], 'size': [1., 1., 1., 1.]})
    for kw, word in ((dict(cutoff=0.), 'cutoff'), (dict(cutoff=4., dr=-1.), 'dr'), (dict(cutoff=4., edge='cap'), 'edge'),
                     (dict(cutoff=4., pairs='same'), 'group_column'), (dict(cutoff=4., pairs='x'), 'pairs'),
                     (dict(cutoff=4., group_column='label'), 'label'), (dict(cutoff=4., group_column='size'), 'integers'),
                     (dict(cutoff=4., pos_columns=['y']), 'pos_columns'), (dict(cutoff=4., pos_columns=['y', 'q']), 'pos_columns'),
                     (dict(cutoff=4., t_column='t'), "'t'"), (dict(cutoff=4., mpp=0.), 'mpp'),
                     (dict(cutoff=4., boundary=[[0., 0.], [1., -1.]]), 'boundary')):
        with pytest.raises(ValueError, match=word):
            ct.pair_correlation(f, **kw)
    with pytest.raises(ValueError, match='empty'):
        ct.pair_correlation(f.iloc[:0], 4.)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(_lib.EngineError):
        ct.pair_correlation_arrays(POS2, OFF, 4.)
    f = pd.DataFrame({'frame': [0, 1], 'y': [0., 1.], 'x': [0., 1.]})       # no particle column
    with pytest.raises(_lib.EngineError):
        ct.pair_correlation(f, 4.)


# ---- the restatement on known answers ----
def test_arc_fraction_against_monte_carlo():
    """200 random points and radii in a 30 x 50 box, 2e5 uniform angles each: the closed form lies
    within 5 standard errors sqrt(phi (1 - phi) / n) of the sampled fraction"""
    rng = np.random.RandomState(11)
    lo, hi, n = np.array([0., 0.]), np.array([30., 50.]), 200000
    worst = 0.
    for _ in range(200):
        q0, q1, R = rng.uniform(0., 30.), rng.uniform(0., 50.), rng.uniform(0.5, 60.)
        theta = rng.uniform(0., 2 * np.pi, n)
        y, x = q0 + R * np.cos(theta), q1 + R * np.sin(theta)
        sampled = ((y >= 0.) & (y <= 30.) & (x >= 0.) & (x <= 50.)).mean()
        phi = float(yard.arc_fraction(q0, q1, lo, hi, R))
        assert 0. <= phi <= 1.
        worst = max(worst, abs(phi - sampled))
        assert abs(phi - sampled) <= 5. * np.sqrt(phi * (1. - phi) / n), (q0, q1, R, phi, sampled)
    print('largest deviation from the sample', worst)
    assert worst < 0.01


def test_arc_fraction_far_from_the_walls_and_in_a_corner():
    lo, hi = np.array([0., 0.]), np.array([30., 50.])
    for q0, q1, R in ((15., 25., 15.), (10., 40., 9.99), (3., 3., 3.), (27., 47., 2.5)):
        assert float(yard.arc_fraction(q0, q1, lo, hi, R)) == 1.0
    for q0, q1 in ((0., 0.), (30., 0.), (0., 50.), (30., 50.)):
        assert float(yard.arc_fraction(q0, q1, lo, hi, 7.)) == 0.25
    assert float(yard.arc_fraction(0., 25., lo, hi, 7.)) == 0.5              # on a wall
    assert float(yard.arc_fraction(15., 25., lo, hi, 1e3)) == 0.              # the circle misses the box


def test_square_lattice_counts_of_an_interior_row():
    """9 x 9 lattice, dr = 1, cutoff 4: the only interior row is the centre; its neighbours at
    d2 = 1, 2 | 4, 5, 8 | 9, 10, 13 number 4, 4 | 4, 8, 4 | 4, 8, 8; d2 = 4 and 9 sit on an edge and
    fall in the upper bin, the four at d2 = 16 = edge2[B] in none"""
    pos, off = yard.lattice(9, 9)
    res = yard.pair_correlation(pos, off, 4., 1., edge='interior')
    assert res.n_rows.tolist() == [81] and res.n_ref.tolist() == [1]
    assert res.count.tolist() == [[0, 8, 16, 20]]
    assert res.weight.tolist() == [[1., 1., 1., 1.]]
    rho = 80. / 64.
    np.testing.assert_array_equal(res.g_frame[0], res.count[0] / ((rho * (np.pi * np.array([1., 3., 5., 7.]))) * 1.))
    yard.assert_equal_bits(res.g, res.g_frame[0])
    every = yard.pair_correlation(pos, off, 4., 1., edge='none')
    assert every.n_ref.tolist() == [81] and every.count[0, 0] == 0 and every.count[0].sum() % 2 == 0      # ordered pairs


def _double_loop(pos, off, cutoff, dr, mpp, boundary, edge, group, pairs):
    """count, n_ref and n_rows with a plain loop over the pairs"""
    r_edges, edge2, _ = yard.bins(cutoff, dr, pos.shape[1])
    B = len(edge2) - 1
    q = pos * (np.asarray(mpp, dtype=np.float64) * np.ones(pos.shape[1]))
    lo, hi = yard.box_of(q, boundary, np.asarray(mpp, dtype=np.float64) * np.ones(pos.shape[1]))
    count = np.zeros((len(off) - 1, B), dtype=np.int64)
    n_ref, n_rows = np.zeros(len(off) - 1, dtype=np.int64), np.zeros(len(off) - 1, dtype=np.int64)
    exists = [bool(np.isfinite(x).all() and (x >= lo).all() and (x <= hi).all()) for x in q]
    for t in range(len(off) - 1):
        for i in range(off[t], off[t + 1]):
            if not exists[i]:
                continue
            n_rows[t] += 1
            if edge == 'interior' and not ((q[i] - lo >= r_edges[B]).all() and (hi - q[i] >= r_edges[B]).all()):
                continue
            n_ref[t] += 1
            for j in range(off[t], off[t + 1]):
                if j == i or not exists[j]:
                    continue
                same = group is not None and group[i] == group[j] and group[i] >= 0
                if (pairs == 'same' and not same) or (pairs == 'other' and same):
                    continue
                d2 = sum(float(q[j, a] - q[i, a]) * float(q[j, a] - q[i, a]) for a in range(pos.shape[1]))
                b = bisect.bisect_right(edge2.tolist(), d2) - 1
                if b < B:
                    count[t, b] += 1
    return count, n_ref, n_rows


@pytest.mark.parametrize('ndim,edge,pairs', [(2, 'arc', 'all'), (2, 'interior', 'same'), (2, 'none', 'other'),
                                             (3, 'none', 'all'), (3, 'interior', 'other'), (3, 'none', 'same')])
def test_restatement_equals_the_double_loop(ndim, edge, pairs):
    rng = np.random.RandomState(5 + ndim)
    pos, off = yard.uniform_frames(9 + ndim, (0, 1, 7, 12, 2), (8., 6., 7.)[:ndim], ndim)
    pos[3] = np.nan
    pos[5] = pos[6]                                      # coincident rows
    pos[11] = 100.                                       # outside a given boundary
    group = rng.randint(-1, 3, len(pos)).astype(np.int64)
    mpp = (2., 1., 0.5)[:ndim]
    boundary = [[0.] * ndim, [8., 6., 7.][:ndim]]
    cutoff = 1.7 if edge == 'interior' else 5.2
    res = yard.pair_correlation(pos, off, cutoff, 0.5, mpp, boundary, edge, group, pairs)
    count, n_ref, n_rows = _double_loop(pos, off, cutoff, 0.5, mpp, boundary, edge, group, pairs)
    assert (res.count == count).all() and (res.n_ref == n_ref).all() and (res.n_rows == n_rows).all()
    assert (edge == 'interior' or res.count.sum() > 0) and res.n_rows.tolist()[:2] == [0, 1]
    if pairs == 'all':
        assert res.count[2, 0] >= 2                     # the coincident rows count each other in bin 0


def test_counts_of_same_and_other_add_up():
    pos, off = yard.uniform_frames(2, (40, 55), (20., 20.))
    group = np.random.RandomState(2).randint(-2, 6, len(pos)).astype(np.int64)
    parts = {p: yard.pair_correlation(pos, off, 6., 0.5, group=group, pairs=p) for p in ('all', 'same', 'other')}
    assert (parts['all'].count == parts['same'].count + parts['other'].count).all()
    assert parts['same'].count.sum() > 0 and parts['other'].count.sum() > 0


def test_ideal_gas_is_flat_with_the_arc_correction_and_falls_without():
    """64 frames of 400 uniform points in a 256 x 256 box, cutoff 40, dr 2: |g - 1| within 5 standard
    deviations sqrt(2 / count) of a count of ordered pairs in every bin; without a correction g leaves
    that band at large r"""
    pos, off = yard.uniform_frames(20261020, (400,) * 64, (256., 256.))
    box = [[0., 0.], [256., 256.]]
    arc = yard.pair_correlation(pos, off, 40., 2., boundary=box, edge='arc')
    total = arc.count.sum(0)
    band = 5. * np.sqrt(2. / total)
    print('largest |g - 1| in units of sqrt(2 / count):', (np.abs(arc.g - 1.) / np.sqrt(2. / total)).max())
    assert (np.abs(arc.g - 1.) <= band).all()
    none = yard.pair_correlation(pos, off, 40., 2., boundary=box, edge='none')
    assert (none.count == arc.count).all()
    assert (none.g[-5:] < 1. - band[-5:]).all() and (none.g <= arc.g).all()
    inner = yard.pair_correlation(pos, off, 40., 2., boundary=box, edge='interior')
    wide = 5. * np.sqrt(2. / inner.count.sum(0))
    assert (np.abs(inner.g - 1.) <= wide).all() and (inner.n_ref < inner.n_rows).all()


def test_degenerate_frames_are_nan_and_skipped_in_the_pool():
    pos, off = yard.table([np.zeros((0, 2)), [[1., 1.]], [[1., 1.], [2., 3.], [4., 1.]]])
    res = yard.pair_correlation(pos, off, 3., 1., edge='none')
    assert np.isnan(res.g_frame[:2]).all() and not np.isnan(res.g_frame[2]).any()
    yard.assert_equal_bits(res.g, res.g_frame[2])
    same = yard.pair_correlation(np.ones((5, 2)), np.array([0, 5]), 3., 1., edge='none')      # a box without volume
    assert same.count.tolist() == [[20, 0, 0]] and np.isnan(same.g).all() and np.isnan(same.g_frame).all()


# ---- the stage path ----
def _descriptor():
    d = _abi.PairCorrelation()
    d.ndim, d.edge, d.pairs, d.n_bins, d.dr = 2, _abi.PCF_EDGE_ARC, _abi.PCF_PAIRS_ALL, 8, 0.5
    d.mpp[0] = d.mpp[1] = d.mpp[2] = 1.
    d.status = d.frame_offset = d.box = d.edge2 = d.shell = d.g = 64        # never dereferenced: there is no handle
    return d


CALL = 'ctr_pair_correlation_device'


def test_descriptor_then_handle():
    lib = _lib.load()
    fn = getattr(lib, CALL)
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    assert fn(None, None, None) == _abi.ERR_INVALID
    assert msg() == CALL + ': null descriptor'
    assert fn(None, ctypes.byref(_descriptor()), None) == _abi.ERR_INVALID
    assert msg() == CALL + ': null handle'


BAD = [('ndim', 4, 'ndim'), ('ndim', 1, 'ndim'), ('n_bins', 0, 'n_bins'), ('n_bins', _abi.PCF_MAX_BINS + 1, 'CTR_PCF_MAX_BINS'),
       ('n_frames', -1, 'negative'), ('n_features', -1, 'negative'), ('n_frames', 2 ** 31 - 2, 'too many'),
       ('n_features', 2 ** 31, 'too many'), ('edge', 3, 'edge'), ('edge', -1, 'edge'), ('pairs', 3, 'pairs'),
       ('dr', 0., 'dr'), ('dr', float('nan'), 'dr'), ('dr', float('inf'), 'dr'),
       ('status', None, 'null status'), ('frame_offset', None, 'null status'), ('box', None, 'null box'),
       ('edge2', None, 'null box'), ('shell', None, 'null box'), ('n_features', 1, 'without pos'), ('g', None, 'null output'),
       ('n_frames', 1, 'null output')]


@pytest.mark.parametrize('field,value,word', BAD)
def test_descriptor_is_refused_under_the_entry_point_name(field, value, word):
    lib = _lib.load()
    d = _descriptor()
    setattr(d, field, value)
    assert getattr(lib, CALL)(None, ctypes.byref(d), None) == _abi.ERR_INVALID
    msg = (lib.ctr_last_error(None) or b'').decode()
    assert msg.startswith(CALL + ': ') and word in msg, msg


def test_arc_in_3d_mpp_and_group_are_refused():
    lib = _lib.load()
    last = lambda: (lib.ctr_last_error(None) or b'').decode()
    d = _descriptor()
    d.ndim = 3
    assert getattr(lib, CALL)(None, ctypes.byref(d), None) == _abi.ERR_INVALID and 'arc' in last()
    d.edge = _abi.PCF_EDGE_INTERIOR
    assert getattr(lib, CALL)(None, ctypes.byref(d), None) == _abi.ERR_INVALID and last() == CALL + ': null handle'
    for axis, value in ((0, float('nan')), (1, float('inf')), (1, 0.), (0, -1.)):
        d = _descriptor()
        d.mpp[axis] = value
        assert getattr(lib, CALL)(None, ctypes.byref(d), None) == _abi.ERR_INVALID
        assert last() == CALL + ': mpp must be finite and positive'
    d = _descriptor()
    d.n_features, d.pos, d.pairs = 1, 64, _abi.PCF_PAIRS_SAME
    assert getattr(lib, CALL)(None, ctypes.byref(d), None) == _abi.ERR_INVALID and 'without group' in last()


def test_prototype_signature_constants_and_abi():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    assert _lib.load().ctr_abi_version() == 8
    for clause in ('Bins.', 'Scaling.', 'Box.', 'A row exists', 'Reference rows.', 'Pairs.', 'Binning.', 'Weight.', 'g_frame[t, b]', 'denominators of clause 9'):
        assert clause in header and clause in st.__doc__, clause
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', header))
    assert set(protos) == set(_lib.SIGNATURES)
    params = [p.strip() for p in protos[CALL].split(',')]
    assert params == ['ctr_handle* h', 'const ctr_pair_correlation* d', 'void* hip_stream']
    assert _lib.SIGNATURES[CALL] == _lib._stage(_abi.PairCorrelation) and CALL in _lib.EXPORTS
    assert hasattr(_lib.load(), CALL) and callable(_lib.Engine.pair_correlation_device)
    body = re.search(r'typedef struct ctr_pair_correlation \{(.*?)\} ctr_pair_correlation;', header, flags=re.S).group(1)
    assert re.findall(r'\b(\w+)(?:\[\w+\])?\s*;', body) == [f[0] for f in _abi.PairCorrelation._fields_]
    defines = dict(re.findall(r'#define\s+(CTR_PCF_\w+)\s+(\d+)', header))
    assert defines == {'CTR_PCF_OK': '0', 'CTR_PCF_BAD_TABLE': '1', 'CTR_PCF_MAX_BINS': str(_abi.PCF_MAX_BINS),
                       'CTR_PCF_EDGE_NONE': '0', 'CTR_PCF_EDGE_INTERIOR': '1', 'CTR_PCF_EDGE_ARC': '2',
                       'CTR_PCF_PAIRS_ALL': '0', 'CTR_PCF_PAIRS_SAME': '1', 'CTR_PCF_PAIRS_OTHER': '2'}
    assert (_abi.PCF_OK, _abi.PCF_BAD_TABLE) == (0, 1) and _abi.PCF_MAX_BINS >= 256
    assert _abi.PCF_EDGE_CODES == {'none': 0, 'interior': 1, 'arc': 2} and _abi.PCF_PAIRS_CODES == {'all': 0, 'same': 1, 'other': 2}


def test_struct_layout_matches_the_compiler(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_pair_correlation));\n'
    expect = [ctypes.sizeof(_abi.PairCorrelation)]
    for f, _ in _abi.PairCorrelation._fields_:
        src += 'printf("%%zu\\n", offsetof(ctr_pair_correlation, %s));\n' % f
        expect.append(getattr(_abi.PairCorrelation, f).offset)
    src += 'return 0;}\n'
    (tmp_path / 'layout.c').write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == expect


def test_public_names():
    names = {'pair_correlation_arrays', 'pair_correlation'}
    assert names | {'static'} <= set(ct.__all__) and ct.static is st
    for name in names:
        assert getattr(ct, name) is getattr(st, name)
    assert st.PairCorrelation._fields == ('r_edges', 'g', 'g_frame', 'count', 'weight', 'n_ref', 'n_rows', 'status')
    for fn in (st.pair_correlation_arrays, st.pair_correlation):
        assert 'trackpy' in fn.__doc__
    assert 'not pinned' in st.__doc__
