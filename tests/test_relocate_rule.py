"""The relocation rule without a GPU: the NumPy restatement of tests/_relocate.py
equals the reference's recorded candidates on every fixture and, where the reference exists, a
fresh run of it; on constructed ties every comparison of the float64 rule decides as cKDTree and
the reference's own NumPy functions do; the C-ABI of ``ctr_relocate_device`` is declared,
exported, mirrored and validated; the launch decision is the restated one at its edges."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

import _cases
import _characterize
import _relocate
import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib, find, relocate

sys.path.insert(0, os.path.join(_cases.ROOT, 'oracle'))
import refshim  # noqa: E402

FIXTURES = _relocate.fixtures()


def assert_query(case, q, coords, extra, exact_float=False):
    """(coords, extra) of query q against the fixture: coordinates and order exact; integer frames
    bit for bit; float frames to rtol 1e-12 (what tests/test_characterize_rule.py uses)."""
    expect = case.expect[q]
    if expect is None:
        assert coords is None
        return
    assert coords is not None
    np.testing.assert_array_equal(coords, expect[0])
    size = _relocate.size_array(extra, case.ndim, case.isotropic)
    got = (extra['mass'], extra['signal'], size)
    for g, e, key in zip(got, expect[1:], ('mass', 'signal', 'size')):
        assert g.shape == e.shape, key
        if case.frame.dtype.kind in 'ui':
            np.testing.assert_array_equal(g, e, err_msg=key)
        else:
            np.testing.assert_allclose(g, e, rtol=1e-12, atol=0, err_msg=key)


@pytest.mark.parametrize('case', FIXTURES, ids=lambda c: c.name)
def test_restatement_equals_fixture(case):
    for q in range(case.n_queries):
        coords, extra = _relocate.compose(case.frame, case.threshold, case.query(q), case.known, **case.kwargs())
        assert_query(case, q, coords, extra)


def test_fixtures_cover_the_rule():
    fx = FIXTURES
    counts = [[0 if e is None else len(e[0]) for e in c.expect] for c in fx]
    for c, n in zip(fx, counts):
        assert 2 * sum(k > 0 for k in n) >= len(n), c.name
        for e in c.expect:
            assert e is None or len(np.unique(e[1])) == len(e[1]), c.name      # no equal masses
    assert sum(k >= 2 for n in counts for k in n) >= 10
    for ndim in (2, 3):
        assert {np.dtype(d) for d in ('uint8', 'uint16', 'int16', 'int32', 'float32', 'float64')} \
            == {c.frame.dtype for c in fx if c.ndim == ndim}
    assert any(not c.isotropic and c.ndim == 2 for c in fx) and any(not c.isotropic and c.ndim == 3 for c in fx)
    assert any(c.scale_factor == 2 for c in fx) and any(c.minmass > 0 for c in fx)
    assert any(len(c.query(q)) == 3 for c in fx for q in range(c.n_queries))
    assert any(e is not None and len(e[0]) == 0 for c in fx for e in c.expect)      # all fell to minmass
    edges = next(c for c in fx if c.name == '2d_edges_u8')
    assert edges.query(0)[0, 0] == -3 and edges.expect[0] is not None                # 3 px beyond an edge
    assert _relocate.box_of(edges.query(2), edges.frame.shape, (10, 10)) is None and edges.expect[2] is None
    assert edges.expect[3] is None                                                   # hidden altogether
    d = _relocate.derived(edges.diameter, edges.separation, edges.search_range)
    m, _, _ = _relocate.masked_box(edges.frame, edges.query(3), edges.known, d, edges.separation, edges.search_range)
    assert not m.any() and _relocate.masked_box(edges.frame, edges.query(3), np.empty((0, 2)), d, edges.separation,
                                                edges.search_range)[0].any()
    bg = next(c for c in fx if c.name == '2d_bgedge_u16')
    hit = _relocate.background(bg.known, bg.query(0), bg.search_range, 3.)
    assert hit.tolist() == [True, False] and bg.separation[0] > bg.diameter[0] // 2 + 1
    assert [26, 32] in bg.expect[0][0].tolist() and [26, 32] not in bg.expect[1][0].tolist()


@pytest.mark.skipif(not refshim.available(), reason='the reference is not present')
def test_reference_reproduces_fixtures():
    sys.path.insert(0, os.path.join(_cases.ROOT, 'tests', 'golden'))
    import make_golden_relocate
    _, run = make_golden_relocate.reference_relocate()
    for name in ('2d_multi_u8', '3d_aniso_float32', '2d_bgedge_u16'):
        case = next(c for c in FIXTURES if c.name == name)
        args = dict(case.args)
        for q in range(case.n_queries):
            coords, extra, thr = run(case.frame, case.known, case.query(q), args)
            assert thr == case.threshold
            expect = case.expect[q]
            if expect is None:
                assert coords is None
                continue
            np.testing.assert_array_equal(coords, expect[0])
            np.testing.assert_array_equal(extra['mass'], expect[1])
            np.testing.assert_array_equal(extra['signal'], expect[2])
            np.testing.assert_array_equal(_relocate.size_array(extra, case.ndim, case.isotropic), expect[3])


# ---- constructed ties ----------------------------------------------------------------------------
TIES = _relocate.tie_cases()
# what the float64 rule gives on them (recorded here so that a change of the rule shows)
TIE_RESULT = {
    'visible_edge_axis': None, 'visible_edge_6_8': None, 'visible_outside': [[27, 31]],
    'background_edge_6_8': [[26, 31]], 'background_edge_axis': [[26, 31]], 'background_inside': None,
    'max_dist_on': None, 'max_dist_axis': None, 'max_dist_beyond': [[26, 32]],
    'reach_3_4': [[27, 32]], 'reach_axis': [[24, 33]], 'reach_offset_source': [[27, 32]], 'reach_beyond': None,
    'reach_aniso_axis': None, 'reach_aniso_axis0': [[28, 28]], 'reach_aniso_beyond': None,
    'plateau_sum': [[24, 30]], 'plateau_c_order': [[25, 28]], 'plateau_2x2': [[25, 29]], 'plateau_aniso': [[25, 27]],
}


def _reference_masks():
    if not refshim.available():
        return None
    refshim.load()
    return sys.modules['clustertracking.masks']


@pytest.mark.parametrize('tie', TIES, ids=lambda t: t[0])
def test_ties_decide_as_ckdtree_and_the_reference(tie):
    """Every comparison of the restated float64 rule against what the reference calls: cKDTree's
    query_ball_point (background, reach), query_pairs through the host drop_close, and -- where
    the reference exists -- its own binary_mask_multiple and query_point."""
    name, frame, sources, known, kw = tie
    ndim = frame.ndim
    dia, sep, sr = (_relocate.as_tuple(kw[k], ndim) for k in ('diameter', 'separation', 'search_range'))
    d = _relocate.derived(dia, sep, sr)
    sr_a = np.array(sr, dtype=np.float64)
    coords, _ = _relocate.compose(frame, _relocate.TIE_THRESHOLD, sources, known, **kw)
    assert (None if coords is None else coords.tolist()) == TIE_RESULT[name]
    origin, end = _relocate.box_of(sources, frame.shape, d['slice_radius'])
    ext, rel = tuple(end - origin), sources - origin
    # background: TreeFinder.query_points (find_link.py:224-233)
    if len(known):
        tree = cKDTree(known / sr_a[None, :], 15)
        found = {i for sl in tree.query_ball_point(sources / sr_a[None, :], d['max_dist']) for i in sl}
        hit = _relocate.background(known, sources, sr, d['max_dist'])
        assert set(np.flatnonzero(hit)) == found
    # reach: query_point (find_link.py:25-41) on every pixel of the box
    pix = np.argwhere(np.ones(ext, dtype=bool))
    if all(s == sr[0] for s in sr):
        found = cKDTree(pix, 30).query_ball_point(rel, sr[0])
    else:
        found = cKDTree(pix / sr_a[None, :], 30).query_ball_point(rel / sr_a[None, :], 1.)
    found = {i for sl in found for i in sl}
    assert set(np.flatnonzero(_relocate.within_reach(pix, rel, sr))) == found
    # drop close: find.drop_close = cKDTree.query_pairs(1 - 1e-7) and the reference's order
    bright = np.argwhere(frame[tuple(slice(o, e) for o, e in zip(origin, end))] > 0)
    values = frame[tuple((bright + origin).T)]
    kept = find.drop_close(bright, sep, values)
    np.testing.assert_array_equal(bright[~_relocate.close_losers(bright, sep, values)], kept)
    masks = _reference_masks()
    if masks is not None:
        vis = masks.binary_mask_multiple(rel, ext, d['slice_radius'], include_edge=True)
        np.testing.assert_array_equal(_relocate.visible(ext, rel, d['slice_radius']), vis)
        if len(known):
            hid = masks.binary_mask_multiple(known - origin, ext, sep, include_edge=False)
            np.testing.assert_array_equal(_relocate.hidden(ext, known - origin, sep), hid)
        mod = sys.modules['clustertracking.find_link']
        got = mod.query_point(rel, pix, sr_a)
        want = pix[_relocate.within_reach(pix, rel, sr)]
        assert sorted(map(tuple, [] if got is None else got.tolist())) == sorted(map(tuple, want.tolist()))


def test_the_ties_are_ties():
    """the constructed quantities sit on their bounds to the last bits"""
    ulp = 4 * np.finfo(np.float64).eps
    v = _relocate.ellipse_sums((48, 56), [[24., 28.]], [10., 10.])[0]
    assert abs(v[24, 38] - 1) <= ulp and abs(v[30, 36] - 1) <= ulp and v[31, 36] > 1.1
    h = _relocate.ellipse_sums((48, 56), [[20., 23.], [16., 31.]], [10., 10.])
    assert abs(h[0, 26, 31] - 1) <= ulp and abs(h[1, 26, 31] - 1) <= ulp
    for k, s in (([33., 40.], [24., 28.]), ([39.5, 28.], [24.5, 28.])):
        d2 = sum((a / 5. - b / 5.) ** 2 for a, b in zip(k, s))
        assert abs(d2 / 9. - 1) <= ulp
    assert 3 ** 2 + 4 ** 2 == 5 ** 2 and abs((17 / 6. - 11 / 6.) ** 2 - 1) <= ulp


# ---- C ABI ---------------------------------------------------------------------------------------
def test_header_declares_and_library_exports():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'\bint\s+ctr_relocate_device\s*\(\s*ctr_handle\s*\*', header)
    assert 'typedef struct ctr_relocate' in header
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    lib = _lib.load()
    assert lib.ctr_abi_version() == 8
    for name in ('ctr_relocate_device', 'ctr_relocate_plan'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for name, value in (('CTR_RELOCATE_MAX_MAXIMA', _abi.RELOCATE_MAX_MAXIMA), ('CTR_RELOCATE_MAX_BACKGROUND', _abi.RELOCATE_MAX_BACKGROUND),
                        ('CTR_RELOCATE_TILE_BYTES', _abi.RELOCATE_TILE_BYTES)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % name, header).group(1)) == value
    assert (_abi.RELOCATE_MAX_MAXIMA, _abi.RELOCATE_MAX_BACKGROUND, _abi.RELOCATE_TILE_BYTES, _abi.LINK_MAX_SOURCES) == \
        (_relocate.MAX_MAXIMA, _relocate.MAX_BACKGROUND, _relocate.TILE_BYTES, _relocate.MAX_SOURCES)
    assert re.search(r'CTR_RELOCATE_OK = 0, CTR_RELOCATE_CAPACITY = 1, CTR_RELOCATE_BAD_FRAME = 2', header)


def test_relocate_struct_layout_matches_header(tmp_path):
    """ctypes mirror of ctr_relocate vs the C compiler's view of include/ctrefine.h"""
    fields = [f[0] for f in _abi.Relocate._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_relocate));\n'
    for f in fields:
        src += 'printf("%%zu\\n", offsetof(ctr_relocate, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == ctypes.sizeof(_abi.Relocate)
    assert out[1:] == [getattr(_abi.Relocate, f).offset for f in fields]


def _descriptor(n_queries=0):
    d = relocate.descriptor((48, 56), np.uint8, 1, 9, 11, 5)
    d.n_queries = n_queries
    return d


def test_validation_needs_no_device():
    """A bad descriptor is refused before the handle is looked at; the text is the NULL handle's
    last error.  A good descriptor then fails on the NULL handle itself."""
    lib = _lib.load()

    def call(d):
        rc = lib.ctr_relocate_device(None, ctypes.byref(d), None)
        return rc, (lib.ctr_last_error(None) or b'').decode()

    rc, msg = call(_descriptor())
    assert rc == _abi.ERR_INVALID and 'null handle' in msg

    def bad(expect_rc=_abi.ERR_INVALID, word='', **fields):
        d = _descriptor()
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        rc, msg = call(d)
        assert rc == expect_rc and word in msg, (fields, rc, msg)

    bad(ndim=4, word='ndim')
    bad(ndim=1, word='ndim')
    bad(frame_dtype=6, expect_rc=_abi.ERR_UNSUPPORTED, word='dtype')
    bad(shape=(0, 0), word='shape')
    bad(radius=(1, -1), word='radius')
    bad(search_range=(0, 0.), word='search_range')
    bad(search_range=(1, -2.), word='search_range')
    bad(search_range=(1, float('nan')), word='search_range')
    bad(separation=(0, 0.), word='separation')
    bad(separation=(1, -1.), word='separation')
    bad(scale_factor=0., word='scale_factor')
    bad(scale_factor=float('nan'), word='scale_factor')
    bad(minmass=float('nan'), word='minmass')
    bad(max_candidates=0, word='max_candidates')
    bad(n_queries=-1, word='negative')
    bad(n_known=-1, word='negative')
    bad(n_queries=3, word='queries without')       # queries, but no frames / offsets / outputs
    d = _descriptor(3)
    d.frames = d.threshold = d.known_offset = d.source_offset = 8
    rc, msg = call(d)
    assert rc == _abi.ERR_INVALID and 'query_frame' in msg        # cannot be checked on the host: must be given
    d.query_frame = 8
    rc, msg = call(d)
    assert rc == _abi.ERR_INVALID and 'output' in msg
    # no frame is too wide or too deep: one whose thinnest slab exceeds the tile is a valid call
    for shape, dt in (((48, 40000), np.float64), ((64, 128, 128), np.uint8)):
        rc, msg = call(relocate.descriptor(shape, dt, 1, (9,) * len(shape), 11, 5))
        assert rc == _abi.ERR_INVALID and 'null handle' in msg


# ---- the launch decision -----------------------------------------------------------------------
PLAN_CASES = [
    ((48, 56), np.uint8, 9, 11, 5),
    ((48, 56), np.float64, 9, 11, 5),
    ((512, 512), np.uint8, 9, 11, 5),
    ((512, 512), np.float64, 9, 11, 5),             # slab 15 x 512 x 8 B = 60 KiB: beyond the tile, tile = cap
    ((1024, 1024), np.uint16, 9, 13, 5),
    ((64, 128, 128), np.uint8, (9, 17, 17), (9, 17, 17), (4, 8, 8)),     # the cfg-3 stack: slab 160 KiB
    ((512, 273), np.float64, 9, 11, 5),             # 15 x 273 = 4095 pixels: one below the cap
    ((512, 274), np.float64, 9, 11, 5),             # 4110: one row beyond it
    ((16, 24, 24), np.float64, (5, 7, 7), (6, 9, 9), (3, 5, 4)),
    ((16, 24, 24), np.uint8, (5, 7, 7), (6, 9, 9), (3, 5, 4)),
    ((8, 8), np.uint16, 9, 11, 5),                  # frame smaller than every box
    ((64, 64), np.float32, 21, 40, 30),             # a one-source box larger than the frame
    ((300, 300), np.int32, 9, 0.5, 5),              # dilation box 0 -> 1
]


@pytest.mark.parametrize('shape,dtype,diameter,separation,search_range', PLAN_CASES)
def test_plan_is_the_restated_one(shape, dtype, diameter, separation, search_range):
    want = _relocate.plan(shape, dtype, diameter, separation, search_range)
    d = relocate.descriptor(shape, dtype, 1, _relocate.as_tuple(diameter, len(shape)), separation, search_range)
    assert _lib.relocate_plan(d) == want
    assert want[1] <= _relocate.TILE_BYTES


def test_plan_edges():
    """the cap on both sides, and what the kernel does with boxes at the tile and one pixel beyond"""
    assert _relocate.plan((512, 273), np.float64, 9, 11, 5) == (4095, 4095 * 8 + 8)
    assert _relocate.plan((512, 274), np.float64, 9, 11, 5) == (4096, 32768)     # the cap: slabs no longer fit
    assert _relocate.path((21, 21), 4096, 15) == ('tile', 1)                     # ... a one-source box still does
    assert _relocate.path((21, 273), 4096, 15) == ('slabs', 21)
    assert _relocate.path((21, 274), 4096, 15) == ('direct', 1)                  # 4096 // 274 = 14 rows < 15
    tile_c3, _ = _relocate.plan((64, 128, 128), np.uint8, (9, 17, 17), (9, 17, 17), (4, 8, 8))
    assert tile_c3 == 32768 and _relocate.path((19, 35, 35), tile_c3, 10) == ('tile', 1)
    assert _relocate.path((40, 128, 128), tile_c3, 10) == ('direct', 1)
    tile, lds = _relocate.plan((48, 56), np.uint8, 9, 11, 5)
    assert (tile, lds) == (15 * 56, 848)          # the slab of a frame-wide box, above the 21 x 21 of one source
    assert _relocate.path((15, 56), tile, 15) == ('tile', 1)
    assert _relocate.path((16, 56), tile, 15) == ('slabs', 16)
    assert _relocate.path((48, 56), tile, 15) == ('slabs', 48)
    assert _relocate.path((21, 21), tile, 15) == ('tile', 1)
    tile3, _ = _relocate.plan((16, 24, 24), np.float64, (5, 7, 7), (6, 9, 9), (3, 5, 4))
    assert tile3 == 4096 and _relocate.path((13, 19, 17), tile3, 6)[0] == 'slabs'     # one source, float64, 3D
    # sources and known features do not enter the plan: 1 or 30 sources, 0 known, Q = 0 launch alike
    lib = _lib.load()
    d = _descriptor(0)
    assert lib.ctr_relocate_device(None, ctypes.byref(d), None) == _abi.ERR_INVALID
    assert 'null handle' in (lib.ctr_last_error(None) or b'').decode()      # Q = 0 is a valid call
    # the boxes of 1 and of 30 sources
    one = _relocate.box_of(np.array([[24., 28.]]), (48, 56), (10, 10))
    assert tuple(one[1] - one[0]) == (21, 21)
    many = _relocate.box_of(np.random.RandomState(0).uniform(0, 48, (30, 2)), (48, 56), (10, 10))
    assert _relocate.path(tuple(many[1] - many[0]), tile, 15)[0] == 'slabs'


# ---- Python plumbing -----------------------------------------------------------------------------
def _fake(monkeypatch, n, status=0, iso=True, ndim=2):
    calls = []

    def fake_locate(frames, separation, percentile=64, **kw):
        return np.empty((0, ndim), np.int32), np.zeros(2, np.int64), np.array([7.5])

    def fake_arrays(frames, threshold, known, known_offset, sources, source_offset, query_frame, diameter,
                    separation, search_range, minmass, isotropic, scale_factor, max_candidates, device):
        K = max_candidates
        calls.append(K)
        assert threshold[0] == 7.5 and isotropic == iso and list(known_offset) == [0, len(known)]
        pos = np.full((1, K, ndim), -1, np.int32)
        mass = np.full((1, K), np.nan)
        size = np.full((1, K) if iso else (1, K, ndim), np.nan)
        m = min(n, K)
        pos[0, :m] = np.arange(m)[:, None]
        mass[0, :m] = 100. - np.arange(m)
        size[0, :m] = (np.arange(m) + 1.) if iso else (np.arange(m)[:, None] + [1., 2.])
        return (np.array([n], np.int32), pos, mass, mass * 2, size, np.array([status], np.int32))

    monkeypatch.setattr(relocate, 'locate_arrays', fake_locate)
    monkeypatch.setattr(relocate, 'relocate_arrays', fake_arrays)
    return calls


def test_candidates_none_sizes_retry_and_status(monkeypatch):
    image = np.ones((20, 24), np.uint8)
    _fake(monkeypatch, 0)
    assert cta.relocate_candidates(image, [[5., 5.]], None, 9, 11, 5) == (None, None)
    calls = _fake(monkeypatch, 3, iso=False)
    coords, extra = cta.relocate_candidates(image, [[5., 5.]], [[1., 1.]], (7, 9), (9, 11), (4, 6))
    assert coords.dtype == np.int64 and coords.tolist() == [[0, 0], [1, 1], [2, 2]]
    assert sorted(extra) == ['mass', 'signal', 'size_x', 'size_y']
    assert extra['size_y'].tolist() == [1., 2., 3.] and extra['size_x'].tolist() == [2., 3., 4.]
    assert extra['signal'].tolist() == [200., 198., 196.] and calls == [16]
    calls = _fake(monkeypatch, 20)                      # more than the first K: asked again with room for all
    coords, extra = cta.relocate_candidates(image, [[5., 5.]], None, 9, 11, 5)
    assert calls == [16, 20] and len(coords) == 20 and list(extra) == ['mass', 'signal', 'size']
    _fake(monkeypatch, 0, status=_abi.RELOCATE_CAPACITY)
    with pytest.raises(_lib.EngineError):
        cta.relocate_candidates(image, [[5., 5.]], None, 9, 11, 5)


def test_derived_quantities():
    d = relocate.derived((9, 9), (11, 11), (5, 5))
    assert d == dict(radius=(4, 4), dilation_size=(15, 15), slice_radius=(10, 10), bg_radius=(15, 15), max_dist=3.)
    d = relocate.derived((5, 7, 7), (6, 9, 9), (3, 5, 4))
    assert d['slice_radius'] == (6, 9, 8) and d['dilation_size'] == (6, 10, 10) and d['max_dist'] == 3.
    r = relocate.descriptor((48, 56), np.uint16, 3, (7, 9), 11, (4, 6), minmass=5, max_candidates=4)
    assert (r.ndim, r.frame_dtype, r.n_frames, r.isotropic, r.max_candidates) == (2, 1, 3, 0, 4)
    assert list(r.radius)[:2] == [3, 4] and list(r.separation)[:2] == [11., 11.] and list(r.search_range)[:2] == [4., 6.]


def test_no_cpu_fallback():
    try:
        import torch
        if torch.cuda.is_available():
            return
    except Exception:
        pass
    with pytest.raises(_lib.EngineError):
        cta.relocate_candidates(np.ones((20, 20), np.uint8), [[5., 5.]], None, 9, 11, 5)
