"""The cases of tests/_aux_edges.py are what they claim to be (no GPU).

Cluster labelling: the yardstick is cKDTree, as in the reference; on every tie and near-tie pair
the float64 sum in axis order with rounded products gives the same answer, and a sum with fused
products -- what a kernel compiled with contraction computes -- gives another one on some pairs,
in both directions, in 2D and in 3D.  That is a condition on the inputs: only then can the GPU
test tell the two apart.  Frame maximum: every placement is where it says, the planted value is
the frame's only maximum, and NumPy's maximum is NaN for a NaN of either sign."""
import numpy as np
import pytest
from numpy.testing import assert_equal

import _aux_edges as A

_verdicts = {}


def verdicts(sep):
    """(two-feature configurations, by cKDTree, by the rule, by the fused sum), once per separation."""
    if sep not in _verdicts:
        two = [c for c in A.tie_configs(sep) if c.kind in ('tie', 'near')]
        _verdicts[sep] = (two,) + tuple(
            np.array([fn(c.pts[0], c.pts[1], sep) for c in two])
            for fn in (A.pair_by_ckdtree, A.pair_by_rule, A.pair_contracted))
    return _verdicts[sep]


def test_tie_offsets_are_the_pythagorean_ones():
    assert sorted(A.tie_offsets((13, 13))) == [(0, 13), (5, -12), (5, 12), (12, -5), (12, 5), (13, 0)]
    assert (20, 21) in A.tie_offsets((29, 29)) and (5, 24) in A.tie_offsets((13, 26))
    assert (1, 4, 8) in A.tie_offsets((9, 9, 9)) and (2, 3, 6) in A.tie_offsets((7, 7, 7))
    for sep in A.TIE_SEPARATIONS:
        offs = A.tie_offsets(sep)
        assert len(offs) >= len(sep)                # the axis-aligned ones at least
        assert len(A.origins(sep)) == A.N_ORIGINS + 1 and not A.origins(sep)[0].any()
        assert ((A.origins(sep) >= 0) & (A.origins(sep) < 64)).all()


@pytest.mark.parametrize('sep', A.TIE_SEPARATIONS, ids=str)
def test_rule_in_float64_equals_ckdtree_on_every_tie_case(sep):
    two, by_tree, by_rule, _ = verdicts(sep)
    assert len(two) == 3 * (A.N_ORIGINS + 1) * len(A.tie_offsets(sep))
    assert_equal(by_rule, by_tree)
    # the ties are real ones: rounding decides them, some each way over all separations
    for c in A.tie_configs(sep):
        if c.kind == 'triple':
            a, far, b = c.pts
            assert not A.pair_by_rule(a, far, sep)
        if c.kind == 'dup':
            assert (c.pts[0] == c.pts[-1]).all()


@pytest.mark.parametrize('ndim', (2, 3))
def test_fused_sum_disagrees_with_the_yardstick_in_both_directions(ndim):
    joins, splits = [], []
    for sep in A.TIE_SEPARATIONS:
        if len(sep) != ndim:
            continue
        two, by_tree, _, fused = verdicts(sep)
        for c, y, f in zip(two, by_tree, fused):
            if f != y:
                (joins if f else splits).append((sep, tuple(c.pts[0]), tuple(c.pts[1])))
    assert joins and splits, (len(joins), len(splits))
    if ndim == 2:
        assert ((13, 13), (0., 0.), (12., 5.)) in joins        # 1.0000000000000002 by the rule, 1.0 fused
        assert ((29, 29), (0., 0.), (20., 21.)) in splits


def test_assembled_table_keeps_every_configuration_in_its_own_frame():
    cfg = A.tie_configs((13, 13))
    pos, frames = A.assemble(cfg)
    assert len(pos) == sum(len(c.pts) for c in cfg) and (np.diff(frames) < 0).any()
    for k in (0, 17, len(cfg) - 1):
        got = pos[frames == k]
        assert sorted(map(tuple, got)) == sorted(map(tuple, cfg[k].pts))


@pytest.mark.parametrize('ndim', (2, 3))
def test_population_case_sits_on_the_edges_of_the_thread_stride(ndim):
    from clustertracking_amd import find
    pos, offset, sep = A.population_case(ndim)
    counts = np.diff(offset)
    assert_equal(counts, [257, 0, 513, 1, 0, 255, 256, 300, 40, 40, 0])
    assert pos.shape == (offset[-1], ndim)
    frames = np.repeat(np.arange(len(counts)), counts)
    _, ids, sizes = find.label_frames(pos, frames, sep)
    for f in (0, 2, 5, 6):      # scattered frames: singles and clusters of several sizes
        s = sizes[offset[f]:offset[f + 1]]
        assert (s == 1).any() and s.max() >= 4
    assert (sizes[offset[7]:offset[8]] == 300).all()          # the chain is one cluster ...
    chain = pos[offset[7]:offset[8]]
    d = np.sqrt((((chain[:, None] - chain[None]) / sep) ** 2).sum(-1))
    assert ((d <= 1).sum(1) <= 3).all()                         # ... each touching its neighbours only
    a, b = slice(offset[8], offset[9]), slice(offset[9], offset[10])
    assert_equal(pos[a], pos[b])
    assert_equal(sizes[a], sizes[b])
    assert ids[b].min() > ids[a].max()                          # frames never share a cluster
    assert_equal(A.canonical_ids([7, 3, 7, 3, 9]), [0, 1, 0, 1, 4])


@pytest.mark.parametrize('dtype', A.FM_DTYPES, ids=lambda d: np.dtype(d).name)
def test_frame_max_placements_are_where_they_say(dtype):
    v, chunk = A.fm_geometry(dtype)
    assert chunk * np.dtype(dtype).itemsize == 65536 and v * np.dtype(dtype).itemsize == 16
    assert set(A.fm_sizes(dtype)) == {1, v - 1, v, v + 1, chunk - 1, chunk, chunk + 1, 2 * chunk + v - 1} - {0}
    assert A.fm_offsets(dtype) == sorted({0, 1, v - 1})
    # an aligned frame of two chunks and a bit: no head; a frame one element off: a head of v - 1
    assert A.fm_placements(0, 2 * chunk + v - 1, dtype) == dict(
        first=0, last=2 * chunk + v - 2, chunk0_last=chunk - 1, chunk1_first=chunk, tail=2 * chunk)
    assert A.fm_placements(1, chunk + 1, dtype) == dict(
        first=0, last=chunk, head=v - 2, chunk0_last=chunk - 1, chunk1_first=chunk)
    tail = dict(tail=chunk - v + 1) if v > 2 else {}       # (two elements per vector: v - 2 are left)
    assert A.fm_placements(v - 1, chunk - 1, dtype) == dict(first=0, last=chunk - 2, head=0, **tail)
    seen = set()
    for case in A.fm_placement_cases(dtype):
        seen.add(case.name.split('-')[0])
        frames = A.fm_frames(case)
        top = frames.max(1)
        assert ((frames == top[:, None]).sum(1) == 1).all(), case.name      # a single maximum
        outside = np.r_[case.buf[:case.offset], case.buf[case.offset + frames.size:]]
        assert len(outside) >= v and (outside > top.max()).all(), case.name
    assert seen == {'first', 'last', 'head', 'chunk0_last', 'chunk1_first', 'tail'}
    names = [c.name for c in A.fm_value_cases(dtype)]
    assert len(set(names)) == len(names)
    if np.dtype(dtype) == np.uint16:
        tops = {c.name: A.fm_expected(c)[1] for c in A.fm_value_cases(dtype)}
        assert tops['max_32768-3x%d' % (v + 1)] == 32768. and tops['type_max-3x%d' % (chunk + 1)] == 65535.


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_frame_max_nan_cases_are_nan_for_numpy_whatever_the_sign(dtype):
    pos, neg = A.fm_nan_variants(dtype)
    assert np.isnan(pos) and np.isnan(neg) and not np.signbit(pos) and np.signbit(neg)
    with np.errstate(invalid='ignore'):
        made = np.array([0.], dtype=dtype) * np.array([np.inf], dtype=dtype)
    assert made.tobytes() in (pos.tobytes(), neg.tobytes())     # arithmetic yields one of the two
    kinds = set()
    v, chunk = A.fm_geometry(dtype)
    for case in A.fm_nan_cases(dtype):
        kinds.add(case.name.split('-')[1])
        frames, exp = A.fm_frames(case), A.fm_expected(case)
        t = case.n_frames // 2
        assert_equal(np.isnan(exp), np.arange(case.n_frames) == t, err_msg=case.name)
        nan_at = np.flatnonzero(np.isnan(frames[t]))
        assert np.signbit(frames[t, nan_at]).all() == case.name.startswith('neg')
        if '-same_lane-' in case.name:
            peak_at = int(np.nanargmax(frames[t]))
            assert frames[t, peak_at] == dtype(A.FLOAT_PEAK) and nan_at.tolist() == [peak_at + A.FM_THREADS * v]
            head = (-(case.offset + t * case.frame_elems)) % v
            assert peak_at >= head and (peak_at - head) // v < A.FM_THREADS and nan_at[0] < chunk - v
    assert kinds == {'first', 'last', 'head', 'chunk0_last', 'chunk1_first', 'tail', 'same_lane', 'all'}


def test_nan_twins_differ_in_one_sign_bit():
    a, b, f0, diameter = A.nan_twin_frames()
    assert a.shape == (64, 64) and a.dtype == np.float64 and len(f0) == 12
    diff = np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))
    assert len(diff) == 1
    assert a.view(np.uint64).ravel()[diff[0]] ^ b.view(np.uint64).ravel()[diff[0]] == 1 << 63
    y, x = np.unravel_index(diff[0], a.shape)
    assert np.isnan(a[y, x]) and np.isnan(b[y, x]) and np.isnan(a.max()) and np.isnan(b.max())
    assert (((f0[['y', 'x']].values - [y, x]) ** 2).sum(1) > (diameter // 2 + 2) ** 2).all()
