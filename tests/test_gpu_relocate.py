"""``ctr_relocate_device`` on the MI355X against the reference's recorded candidates
(tests/golden/relocate) and the NumPy restatement of tests/_relocate.py.

Measures.  Coordinates, order, ``n_found`` and ``status``: exact.  Integer frames: mass, signal and
size bit for bit (exact integer sums, then one division and one square root, both correctly
rounded on either side).  float64 frames: rtol 1e-12, what tests/test_characterize_rule.py uses
(signal exact).  float32 frames: the reference sums its float32 window in float32, the device in
float64, so mass and size agree to the bound of plain float32 summation of the window,
n_window * 2^-24 -- the bound tests/test_gpu_characterize.py derives for ``ctr_characterize_device``,
whose rule this stage applies (signal exact)."""
import numpy as np
import pytest

import _characterize
import _relocate
import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib, relocate
from clustertracking_amd.find import locate_arrays

pytestmark = pytest.mark.gpu

FIXTURES = _relocate.fixtures()
K = 6


def run(frames, thr, known, known_offset, queries, query_frame, kw, k=K, **more):
    sources = np.vstack(queries) if len(queries) else np.empty((0, frames.ndim - 1))
    soff = np.cumsum([0] + [len(s) for s in queries])
    return cta.relocate_arrays(frames, thr, known, known_offset, sources, soff, query_frame, max_candidates=k,
                               **dict(kw, **more))


def run_case(case, k=K):
    queries = [case.query(q) for q in range(case.n_queries)]
    return run(case.frame[None], [case.threshold], case.known, [0, len(case.known)], queries,
               np.zeros(case.n_queries, np.int64), case.kwargs(), k)


def assert_rows(out, q, expect, dtype, radius, k=K):
    """query q of a device result against (coords, mass, signal, size) or None"""
    n_found, pos, mass, signal, size, status = out
    assert status[q] == _abi.RELOCATE_OK
    n = 0 if expect is None else len(expect[0])
    assert n_found[q] == n
    m = min(n, k)
    assert (pos[q, m:] == -1).all() and np.isnan(mass[q, m:]).all() and np.isnan(signal[q, m:]).all() \
        and np.isnan(size[q, m:]).all()
    if n == 0:
        return
    np.testing.assert_array_equal(pos[q, :m], expect[0][:m])
    np.testing.assert_array_equal(signal[q, :m], expect[2][:m])
    dtype = np.dtype(dtype)
    if dtype.kind in 'ui':
        np.testing.assert_array_equal(mass[q, :m], expect[1][:m])
        np.testing.assert_array_equal(size[q, :m], expect[3][:m])
    else:
        rtol = 1e-12 if dtype == np.float64 else _characterize.float_rtol(dtype, radius)
        np.testing.assert_allclose(mass[q, :m], expect[1][:m], rtol=rtol, atol=0)
        np.testing.assert_allclose(size[q, :m], expect[3][:m], rtol=rtol, atol=0)


def restated(case_or_frame, thr, sources, known, kw):
    coords, extra = _relocate.compose(case_or_frame, thr, sources, known, **kw)
    if coords is None:
        return None
    ndim = case_or_frame.ndim
    dia = _relocate.as_tuple(kw['diameter'], ndim)
    return coords, extra['mass'], extra['signal'], _relocate.size_array(extra, ndim, all(d == dia[0] for d in dia))


def radius_of(kw, ndim):
    return tuple(int(d // 2) for d in _relocate.as_tuple(kw['diameter'], ndim))


@pytest.mark.parametrize('case', FIXTURES, ids=lambda c: c.name)
def test_device_equals_fixture_and_restatement(case):
    out = run_case(case)
    radius = radius_of(case.kwargs(), case.ndim)
    for q in range(case.n_queries):
        assert_rows(out, q, case.expect[q], case.frame.dtype, radius)
        # the restatement computes in NumPy's arithmetic: float32 sums as the reference's
        assert_rows(out, q, restated(case.frame, case.threshold, case.query(q), case.known, case.kwargs()),
                    case.frame.dtype, radius)


@pytest.mark.parametrize('tie', _relocate.tie_cases(), ids=lambda t: t[0])
def test_constructed_ties(tie):
    """every edge as tests/test_relocate_rule.py records it: the float64 rule, which equals
    cKDTree and the reference's masks on all of them"""
    name, frame, sources, known, kw = tie
    out = run(frame[None], [_relocate.TIE_THRESHOLD], known, [0, len(known)], [sources], [0], kw)
    assert_rows(out, 0, restated(frame, _relocate.TIE_THRESHOLD, sources, known, kw), frame.dtype, radius_of(kw, 2))


def _plan(case_shape, dtype, kw):
    return _relocate.plan(case_shape, dtype, kw['diameter'], kw['separation'], kw['search_range'])


def test_every_branch_of_the_launch_decision():
    """one slab (box below, at the tile), slabs (one row beyond; sources spread over the frame; a
    one-source box of float64 in 3D), each against the restatement; the plan is the restated one"""
    case = next(c for c in FIXTURES if c.name == '2d_multi_u8')
    kw = case.kwargs()
    d = relocate.descriptor(case.frame.shape, case.frame.dtype, 1, case.diameter, case.separation, case.search_range)
    tile, lds = _lib.relocate_plan(d)
    assert (tile, lds) == _plan(case.frame.shape, case.frame.dtype, kw) == (840, 848)
    rng = np.random.RandomState(5)
    queries = [np.array([[24.2, 28.1]]),                                   # 21 x 21: one slab
               np.array([[4., 10.], [4.2, 45.]]),                          # 15 x 56 = the tile: one slab
               np.array([[5., 10.], [5.2, 45.]]),                          # 16 x 56: slabs of one row
               np.array([[3., 4.], [44., 52.], [20., 30.], [40., 8.]]),    # the whole frame: 48 slabs
               rng.uniform(0, 48, (30, 2))]                                # 30 sources
    paths = []
    for s in queries:
        o, e = _relocate.box_of(s, case.frame.shape, (10, 10))
        paths.append(_relocate.path(tuple(e - o), tile, 15))
    assert paths == [('tile', 1), ('tile', 1), ('slabs', 16), ('slabs', 48), ('slabs', 48)]
    out = run(case.frame[None], [case.threshold], case.known, [0, len(case.known)], queries, np.zeros(5, np.int64), kw, 12)
    found = 0
    for q, s in enumerate(queries):
        expect = restated(case.frame, case.threshold, s, case.known, kw)
        found += 0 if expect is None else len(expect[0])
        assert_rows(out, q, expect, case.frame.dtype, (4, 4), 12)
    assert found >= len(queries)      # the branches are compared on candidates, not on empty results
    case = next(c for c in FIXTURES if c.name == '3d_aniso_float64')
    tile3, _ = _plan(case.frame.shape, case.frame.dtype, case.kwargs())
    o, e = _relocate.box_of(np.array([[8., 12., 12.]]), case.frame.shape, (6, 9, 8))
    assert _relocate.path(tuple(e - o), tile3, 6)[0] == 'slabs'
    queries = [np.array([[8., 12., 12.]]), np.array([[2., 3., 20.], [13., 20., 4.]])]
    out = run(case.frame[None], [case.threshold], case.known, [0, len(case.known)], queries, [0, 0], case.kwargs())
    for q, s in enumerate(queries):
        assert_rows(out, q, restated(case.frame, case.threshold, s, case.known, case.kwargs()), np.float64, (2, 3, 3))
    # 0 known features and Q = 0
    out = run(case.frame[None], [case.threshold], np.empty((0, 3)), [0, 0], queries[:1], [0], case.kwargs())
    assert_rows(out, 0, restated(case.frame, case.threshold, queries[0], np.empty((0, 3)), case.kwargs()), np.float64, (2, 3, 3))
    out = run(case.frame[None], [case.threshold], case.known, [0, len(case.known)], [], [], case.kwargs())
    assert [len(x) for x in out] == [0] * 6 and out[1].shape == (0, K, 3)


def test_fewer_rows_than_candidates():
    case = next(c for c in FIXTURES if c.name == '2d_multi_u8')
    q = next(q for q in range(case.n_queries) if len(case.expect[q][0]) == 3)
    for k in (1, 2, 3):
        out = run(case.frame[None], [case.threshold], case.known, [0, len(case.known)], [case.query(q)], [0], case.kwargs(), k)
        assert out[0][0] == 3 and out[1].shape == (1, k, 2)
        assert_rows(out, 0, case.expect[q], np.uint8, (4, 4), k)


def test_zeros_nan_threshold_and_bad_frame():
    kw = dict(diameter=9, separation=11, search_range=5)
    frames = np.zeros((2, 48, 56), np.uint16)
    frames[1, 20, 20] = 500
    out = run(frames, [np.nan, 100.], np.empty((0, 2)), [0, 0, 0], [np.array([[20., 20.]])] * 4, [0, 1, 2, -1], kw)
    assert out[5].tolist() == [0, 0, _abi.RELOCATE_BAD_FRAME, _abi.RELOCATE_BAD_FRAME]
    assert out[0].tolist() == [0, 1, 0, 0] and out[1][1, 0].tolist() == [20, 20] and out[2][1, 0] == 500
    assert (out[1][[0, 2, 3]] == -1).all() and np.isnan(out[2][[0, 2, 3]]).all()
    # the percentile pass of locate gives the NaN itself
    assert cta.relocate_candidates(frames[0], [[20., 20.]], None, 9, 11, 5) == (None, None)
    coords, extra = cta.relocate_candidates(frames[1], [[21., 19.]], None, 9, 11, 5, percentile=0)
    assert coords is None       # the only non-zero pixel IS the threshold: not above it


def test_capacity_is_data():
    """a saturated plateau (every visible pixel a maximum: 317 > 256) and 31 sources report
    CTR_RELOCATE_CAPACITY; their neighbours in the batch are exact"""
    case = next(c for c in FIXTURES if c.name == '2d_iso_uint8')
    kw = case.kwargs()
    plateau = np.full((48, 56), 200, np.uint8)
    assert _relocate.n_raw_maxima(plateau, 10., np.array([[24., 28.]]), np.empty((0, 2)), 9, 11, 5) == 317
    frames = np.stack([case.frame, plateau])
    many = np.random.RandomState(3).uniform(5, 40, (31, 2))
    queries = [case.query(0), np.array([[24., 28.]]), case.query(1), many, many[:30], case.query(2)]
    qf = [0, 1, 0, 0, 0, 0]
    out = run(frames, [case.threshold, 10.], case.known, [0, len(case.known), len(case.known)], queries, qf, kw)
    assert out[5].tolist() == [0, _abi.RELOCATE_CAPACITY, 0, _abi.RELOCATE_CAPACITY, 0, 0]
    assert out[0][[1, 3]].tolist() == [0, 0] and (out[1][[1, 3]] == -1).all() and np.isnan(out[2][[1, 3]]).all()
    for q, fq in ((0, 0), (2, 1), (5, 2)):
        assert_rows(out, q, case.expect[fq], np.uint8, (4, 4))
    assert_rows(out, 4, restated(case.frame, case.threshold, many[:30], case.known, kw), np.uint8, (4, 4))
    plateau[0, 0] = 1           # the percentile-0 threshold: everything else is above it
    with pytest.raises(_lib.EngineError):
        cta.relocate_candidates(plateau, [[24., 28.]], None, 9, 11, 5, percentile=0)


def test_same_bytes_alone_in_a_batch_and_on_a_stream():
    import torch
    a = next(c for c in FIXTURES if c.name == '2d_multi_u8')
    b = next(c for c in FIXTURES if c.name == '2d_scale2_u8')
    kw = a.kwargs()
    frames = np.stack([a.frame, b.frame])
    known = np.vstack([a.known, b.known])
    koff = [0, len(a.known), len(a.known) + len(b.known)]
    thr = [a.threshold, b.threshold]
    queries = [a.query(1), b.query(1), a.query(0), b.query(3), a.query(3)]
    qf = [0, 1, 0, 1, 0]
    batch = run(frames, thr, known, koff, queries, qf, kw)
    assert batch[0].max() >= 3
    for q in range(len(queries)):
        alone = run(frames, thr, known, koff, [queries[q]], [qf[q]], kw)
        for x, y in zip(alone, batch):
            assert x[0].tobytes() == y[q].tobytes()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        on_stream = run(frames, thr, known, koff, queries, qf, kw)
    for x, y in zip(on_stream, batch):
        assert x.tobytes() == y.tobytes()
    assert_rows(batch, 0, a.expect[1], np.uint8, (4, 4))


def test_chained_after_locate_on_the_device():
    """locate_arrays(_on_device=True) -> relocate_arrays: a located feature taken out of `known` and
    offered as a source is found again"""
    import torch
    a = next(c for c in FIXTURES if c.name == '2d_iso_uint16')
    b = next(c for c in FIXTURES if c.name == '2d_aniso_u16')
    frames = np.stack([a.frame, b.frame])
    kw = dict(diameter=9, separation=11, search_range=5)
    t, pix, pos, offset, thr = locate_arrays(frames, 11, 64, margin=0, dtype=np.uint16, _on_device=True)
    off = offset.cpu().numpy()
    pos_h = pos.cpu().numpy()
    # one feature per frame, away from the edge, that the restatement confirms
    lost = []
    for f in range(2):
        rows = [i for i in range(off[f], off[f + 1]) if 12 <= pos_h[i, 0] < 36 and 12 <= pos_h[i, 1] < 44]
        for i in rows:
            known_f = np.delete(pos_h[off[f]:off[f + 1]], i - off[f], axis=0).astype(np.float64)
            coords, _ = _relocate.compose(frames[f], float(thr[f]), pos_h[i:i + 1].astype(np.float64), known_f, **kw)
            if coords is not None and pos_h[i].tolist() in coords.tolist():
                lost.append(i)
                break
    assert len(lost) == 2
    keep = torch.ones(len(pos_h), dtype=torch.bool, device=pos.device)
    keep[lost] = False
    known = pos[keep]                                  # int32, on the device
    known_offset = offset.clone()
    known_offset[1:] -= 1
    known_offset[2:] -= 1
    out = cta.relocate_arrays(t, thr, known, known_offset, pos_h[lost].astype(np.float64), [0, 1, 2], [0, 1],
                              max_candidates=4, dtype=pix, **kw)
    assert out[5].tolist() == [0, 0]
    for q, i in enumerate(lost):
        assert pos_h[i].tolist() in out[1][q, :out[0][q]].tolist()
        f = q
        known_f = np.delete(pos_h[off[f]:off[f + 1]], i - off[f], axis=0).astype(np.float64)
        assert_rows(out, q, restated(frames[f], float(thr[f]), pos_h[i:i + 1].astype(np.float64), known_f, kw),
                    np.uint16, (4, 4), 4)


def test_relocate_candidates_returns_as_the_reference():
    case = next(c for c in FIXTURES if c.name == '2d_aniso_u16')
    for q in (0, 1):
        coords, extra = cta.relocate_candidates(case.frame, case.query(q), case.known, case.diameter, case.separation,
                                                case.search_range, case.minmass)
        e = case.expect[q]
        np.testing.assert_array_equal(coords, e[0])
        assert list(extra) == ['mass', 'signal', 'size_y', 'size_x']
        np.testing.assert_array_equal(extra['mass'], e[1])
        np.testing.assert_array_equal(np.stack([extra['size_y'], extra['size_x']], 1), e[3])
    edges = next(c for c in FIXTURES if c.name == '2d_edges_u8')
    assert cta.relocate_candidates(edges.frame, edges.query(2), edges.known, 9, 11, 5) == (None, None)


def _spotted(shape, seed, dtype, n=14, noise=6.):
    """a few Gaussian spots on uniform noise (no negative pixels)"""
    rng = np.random.RandomState(seed)
    im = rng.uniform(0, noise, shape)
    grid = np.indices(shape).astype(np.float64)
    centres = np.array([rng.uniform(2, s - 2, n) for s in shape]).T
    for c in centres:
        im += rng.uniform(60, 110) * np.exp(-sum((g - ci) ** 2 for g, ci in zip(grid, c)) / 1.8 ** 2)
    return (im if np.dtype(dtype).kind == 'f' else np.round(2 * im)).astype(dtype), centres


def _threshold(frame):
    return float(np.percentile(frame[np.nonzero(frame)], 64))


@pytest.mark.parametrize('shape,dtype,kw,box0', [
    ((40, 600), np.float64, dict(diameter=9, separation=11, search_range=5), 15),
    ((24, 128, 128), np.uint8, dict(diameter=(9, 17, 17), separation=(9, 17, 17), search_range=(4, 8, 8)), 10),
], ids=['wide_float64', 'cfg3_like_stack'])
def test_frames_whose_slab_exceeds_the_tile(shape, dtype, kw, box0):
    """a frame on which not one slab of a frame-wide box fits the tile (a wide float64 frame, a
    stack with the geometry of workloads.cfg3): a one-source box still takes the tile, a box of
    spread-out sources is read from global memory; each equals the restatement"""
    ndim = len(shape)
    frame, centres = _spotted(shape, 11, dtype)
    tile, _ = _plan(shape, dtype, kw)
    d = _relocate.derived(*(_relocate.as_tuple(kw[k], ndim) for k in ('diameter', 'separation', 'search_range')))
    assert min(box0, shape[0]) * int(np.prod(shape[1:])) > tile == _relocate.TILE_BYTES // np.dtype(dtype).itemsize
    order = np.argsort(centres[:, -1])
    left, right = centres[order[1]], centres[order[-2]]
    queries = [left[None] + 0.7, np.array([left, right]) - 0.4, right[None] + 0.3]
    want_paths = ['tile', 'direct', 'tile']
    if ndim == 2:
        queries.append(np.array([[20., 100.], [20.3, 330.]]))          # 21 x 251: slabs of 2 rows
        want_paths.append('slabs')
    thr = _threshold(frame)
    known = centres[order[2::3]].round()
    paths = []
    for s in queries:
        o, e = _relocate.box_of(s, shape, d['slice_radius'])
        paths.append(_relocate.path(tuple(e - o), tile, box0)[0])
        assert _relocate.n_raw_maxima(frame, thr, s, known, **kw) <= _relocate.MAX_MAXIMA
    assert paths == want_paths
    out = run(frame[None], [thr], known, [0, len(known)], queries, np.zeros(len(queries), np.int64), kw, 8)
    found = 0
    for q, s in enumerate(queries):
        expect = restated(frame, thr, s, known, kw)
        found += 0 if expect is None else len(expect[0])
        assert_rows(out, q, expect, dtype, radius_of(kw, ndim), 8)
    assert found >= 3


def test_background_capacity_is_data():
    """512 background features around one source are taken, 513 report CTR_RELOCATE_CAPACITY; the
    neighbour in the batch is exact"""
    case = next(c for c in FIXTURES if c.name == '2d_iso_uint8')
    kw = case.kwargs()
    src = np.array([[24., 28.]])
    g = np.arange(-14, 14.01, 0.5)
    grid = np.array(np.meshgrid(g, g, indexing='ij')).reshape(2, -1).T
    grid = grid[np.hypot(grid[:, 0], grid[:, 1]) < 14.5] + src + [30., 0.]     # around a source of frame 1
    assert len(grid) > 513
    frames = np.stack([case.frame, case.frame, case.frame])
    for n, want in ((512, _abi.RELOCATE_OK), (513, _abi.RELOCATE_CAPACITY)):
        dense = grid[:n]
        assert _relocate.background(dense, src + [30., 0.], case.search_range, 3.).all()
        known = np.vstack([case.known, dense, case.known])
        koff = [0, len(case.known), len(case.known) + n, len(known)]
        out = run(frames, [case.threshold] * 3, known, koff, [case.query(0), src + [30., 0.], case.query(1)], [0, 1, 2], kw)
        assert out[5].tolist() == [0, want, 0]
        assert_rows(out, 0, case.expect[0], np.uint8, (4, 4))
        assert_rows(out, 2, case.expect[1], np.uint8, (4, 4))
        if want == _abi.RELOCATE_OK:
            assert_rows(out, 1, restated(case.frame, case.threshold, src + [30., 0.], dense, kw), np.uint8, (4, 4))
        else:
            assert out[0][1] == 0 and (out[1][1] == -1).all() and np.isnan(out[2][1]).all()
