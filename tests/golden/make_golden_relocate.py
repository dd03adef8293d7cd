"""Generate tests/golden/relocate/relocate_cases.npz: relocation candidates computed by the
REFERENCE's ``FindLinker.get_relocate_candidates`` (find_link.py:811-867, run through
oracle/refshim.py) -- what pins ``clustertracking_amd.relocate`` and ``ctr_relocate_device``
(DESIGN.md 7b).

    python tests/golden/make_golden_relocate.py     (build container only: needs the reference)

The reference's own ``FindLinker(diameter, separation, search_range, 0, minmass, percentile)`` is
driven: ``image`` is set to a ``Frame`` with ``frame_no``, ``hash`` to a ``TreeFinder`` over
``PointND``s of the known positions, and ``get_relocate_candidates`` is called on ``PointND``s of
the sources.  What NumPy 2 and the absent trackpy / pims need is supplied here, the reference's
arithmetic is untouched: the two weight tables and the ``np.pad`` view of
make_golden_characterize.py (PARITY UNPINNED for the two tables), ``masks.slice_image`` rebound on
``find_link``, and a ``pims.Frame`` subclass whose ``__getitem__`` turns a list of slices into the
tuple it meant.

Layout: ``names`` (JSON list); per case ``i``: ``frame_i``, ``known_i`` (float64 [M, ndim]),
``args_i`` (JSON: diameter, separation, search_range, minmass, percentile, scale_factor),
``threshold_i`` (NaN: none), ``sources_i`` (float64 [S, ndim]) with ``source_offset_i`` ([Q + 1]);
the answers of the Q queries one after the other: ``is_none_i`` ([Q]; a query whose candidates all
fall to ``minmass`` returns empty arrays instead), ``result_offset_i``
([Q + 1]), ``coords_i`` (int64 [R, ndim]), ``mass_i``, ``signal_i`` ([R]) and ``size_i`` ([R], or
[R, ndim] when the diameter is anisotropic), as the reference returns them.

The script asserts what the tests rely on: at least half of the queries of each case have a
candidate, at least 10 queries overall have two or more, no two candidates of a query have equal
mass, and no known feature and no maximum lies within 1e-9 (relative) of the background radius or
of the search range (the comparisons at those edges are fixed by definition, in
tests/test_relocate_rule.py, not by this fixture).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)
import refshim  # noqa: E402
import _relocate  # noqa: E402
import make_golden_characterize  # noqa: E402

DTYPES = ('uint8', 'uint16', 'int16', 'int32', 'float32', 'float64')
SCALE = {'uint8': 2., 'uint16': 300., 'int16': 200., 'int32': 1e6}


def reference_relocate():
    """run(frame, known, sources, args) -> (coords, extra, threshold) by the reference"""
    ref, _ = make_golden_characterize.reference_characterize()     # weight tables, np.pad view
    mod = sys.modules['clustertracking.find_link']
    mod.slice_image = sys.modules['clustertracking.masks'].slice_image
    pims = sys.modules['pims']

    class ListFrame(pims.Frame):
        def __getitem__(self, key):
            return np.ndarray.__getitem__(self, tuple(key) if isinstance(key, list) else key)

    def run(frame, known, sources, args):
        ndim = frame.ndim
        tup = lambda v: _relocate.as_tuple(v, ndim)   # noqa: E731
        linker = mod.FindLinker(tup(args['diameter']), tup(args['separation']), tup(args['search_range']), 0,
                                args['minmass'], args['percentile'])
        meta = {'scale_factor': args['scale_factor']} if args['scale_factor'] != 1. else {}
        linker.image = ListFrame(frame, frame_no=0, metadata=meta)
        mod.PointND.set_counter()
        linker.hash = mod.TreeFinder([mod.PointND(0, p) for p in known], linker.search_range)
        with np.errstate(divide='ignore', invalid='ignore'):
            coords, extra = linker.get_relocate_candidates([mod.PointND(0, s) for s in sources])
        thr = linker.threshold[1] if linker.threshold[0] == 0 else linker.percentile_threshold(args['percentile'])
        return coords, extra, (np.nan if thr is None else float(thr))
    return ref, run


def blobs(shape, n, size, seed, dtype, noise=12., peak=(60, 110)):
    """Gaussian blobs of one size, some centred beyond the edge, plus uniform noise, scaled into
    the pixel type (no negative pixels: what preprocess writes)."""
    rng = np.random.RandomState(seed)
    ndim = len(shape)
    size = _relocate.as_tuple(size, ndim)
    im = np.zeros(shape)
    grid = np.indices(shape).astype(np.float64)
    for _ in range(n):
        c = [rng.uniform(-3, s + 3) for s in shape]
        r2 = sum(((g - ci) / si) ** 2 for g, ci, si in zip(grid, c, size))
        im += rng.uniform(*peak) * np.exp(-r2 * ndim / 2)
    im += rng.uniform(0, noise, shape)
    im *= SCALE.get(dtype, 1.)
    if np.dtype(dtype).kind in 'ui':
        info = np.iinfo(dtype)
        im = np.clip(np.round(im), info.min, info.max)
    return im.astype(dtype)


def scenario(ref, frame, args, seed, n_queries, n_sources=(1,), lose=0.5, jitter=2.):
    """known features = what the reference's grey_dilation finds, less the lost ones; every query
    looks for lost ones near where they were"""
    rng = np.random.RandomState(seed)
    ndim = frame.ndim
    sep = _relocate.as_tuple(args['separation'], ndim)
    found = np.asarray(ref.find.grey_dilation(frame, sep, percentile=args['percentile'], margin=0, precise=True),
                       dtype=np.float64).reshape(-1, ndim)
    lost = rng.rand(len(found)) < lose
    if lost.sum() < 3:
        lost[:3] = True
    known, gone = found[~lost], found[lost]
    queries = []
    for q in range(n_queries):
        k = n_sources[q % len(n_sources)]
        pick = rng.choice(len(gone), size=min(k, len(gone)), replace=False)
        queries.append(gone[pick] + rng.uniform(-jitter, jitter, (len(pick), ndim)))
    return known, queries


def cases(ref):
    """[(name, frame, known, args, [sources of query 0, ...])]"""
    out = []
    base = dict(diameter=9, separation=11, search_range=5, minmass=0, percentile=64, scale_factor=1.)
    for k, dt in enumerate(DTYPES):
        frame = blobs((48, 56), 18, 1.8, 40 + k, dt)
        known, queries = scenario(ref, frame, base, 140 + k, 8)
        out.append(('2d_iso_%s' % dt, frame, known, base, queries))
    frame = blobs((48, 56), 18, 1.8, 50, 'uint8')
    known, queries = scenario(ref, frame, base, 150, 12, n_sources=(2, 3), lose=0.7)
    out.append(('2d_multi_u8', frame, known, base, queries))
    aniso = dict(base, diameter=(7, 9), separation=(9, 11), search_range=(4, 6))
    frame = blobs((48, 56), 18, (1.5, 1.9), 51, 'uint16')
    known, queries = scenario(ref, frame, aniso, 151, 8, n_sources=(1, 2, 2), lose=0.7)
    out.append(('2d_aniso_u16', frame, known, aniso, queries))
    aniso3 = dict(base, diameter=(5, 7, 7), separation=(6, 9, 9), search_range=(3, 5, 4))
    for k, dt in enumerate(DTYPES):
        frame = blobs((16, 24, 24), 18, (1.4, 1.8, 1.8), 60 + k, dt)
        known, queries = scenario(ref, frame, aniso3, 160 + k, 5, n_sources=(1, 1, 2), lose=0.6)
        out.append(('3d_aniso_%s' % dt, frame, known, aniso3, queries))
    # sources 3 pixels beyond an edge, one far outside (no box), one whose box is hidden altogether
    # by a grid of known features
    yy, xx = np.indices((48, 56))

    def drawn(seed, noise, spots):
        im = np.random.RandomState(seed).uniform(0, noise, (48, 56))
        for cy, cx, a in spots:
            im += a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 1.8 ** 2)
        return im

    frame = np.round(2 * drawn(52, 8, ((0.5, 21., 90.), (46.5, 12., 85.), (14., 10., 80.), (30., 14., 75.), (42., 20., 70.),
                                       (24., 44., 95.), (18., 38., 60.)))).astype(np.uint8)
    known = np.array(np.meshgrid(np.arange(8, 41, 8), np.arange(32, 57, 8), indexing='ij'), dtype=np.float64).reshape(2, -1).T
    queries = [np.array([[-3., 20.3]]), np.array([[50.4, 12.3]]), np.array([[-40., 200.]]), np.array([[24.3, 43.8]]),
               np.array([[-40., 200.], [14.5, 9.5]]), np.array([[30.2, 14.4]]), np.array([[41., 19.]])]
    out.append(('2d_edges_u8', frame, known, base, queries,
                dict(none={0: False, 1: False, 2: True, 3: True, 4: False, 5: False, 6: False})))
    # a known feature just inside max_dist (3 search ranges = 15 px) and one just outside, with
    # separation 11 > radius + 1: the outside one, 10.6 px from the blob at (26, 32), would hide it
    # if it counted; it does for the second query, whose other source is close to it
    u = np.array([2., 4.]) / np.sqrt(20.)
    src = np.array([24., 28.])
    frame = np.round(300 * drawn(53, 8, ((26., 32., 90.), (22., 24., 80.), (33., 20., 70.)))).astype(np.uint16)
    known = np.array([src - 14.9 * u, src + 15.1 * u])
    out.append(('2d_bgedge_u16', frame, known, base, [src[None], np.array([src, [30., 40.]])],
                dict(none={0: False}, has={0: (26, 32)}, has_not={0: (22, 24), 1: (26, 32)})))
    # minmass removes the candidate with the brightest peak: one hot pixel on the noise
    frame = drawn(54, 10, ((14., 14., 90.), (30., 40., 80.)))
    frame[20, 26] = frame[36, 14] = 115.
    frame = np.round(2 * frame).astype(np.uint8)
    mm = dict(base, minmass=1200)
    out.append(('2d_minmass_u8', frame, np.empty((0, 2)), mm,
                [np.array([[19., 25.]]), np.array([[14.5, 13.5], [21., 27.]]), np.array([[30., 41.], [35., 15.]]),
                 np.array([[13., 15.]])], dict(none={0: True, 1: False, 2: False, 3: False}, has_not={1: (20, 26), 2: (36, 14)})))
    frame = blobs((48, 56), 18, 1.8, 55, 'uint8')
    sc = dict(base, scale_factor=2., minmass=150)
    known, queries = scenario(ref, frame, sc, 155, 6, n_sources=(1, 2))
    out.append(('2d_scale2_u8', frame, known, sc, queries))
    return out


def check_edges(frame, known, sources, args, thr):
    """no known feature within 1e-9 of the background radius, no raw maximum within 1e-9 of the
    search range (relative, scaled distances)"""
    ndim = frame.ndim
    dia, sep, sr = (_relocate.as_tuple(args[k], ndim) for k in ('diameter', 'separation', 'search_range'))
    d = _relocate.derived(dia, sep, sr)
    for s in sources:
        if len(known):
            dist = np.sqrt(np.sum((known / sr - s / sr) ** 2, 1)) / d['max_dist']
            assert np.all(np.abs(dist - 1) > 1e-9), 'a known feature on the background radius'
    mb = _relocate.masked_box(frame, sources, known, d, sep, sr)
    if mb is None:
        return
    m, origin, rel = mb
    from scipy import ndimage
    if np.isnan(thr):
        return
    peak = np.argwhere((m == ndimage.grey_dilation(m, d['box'], mode='constant')) & (m > thr))
    for r in rel:
        dist = np.sqrt(np.sum((peak / sr - r / sr) ** 2, 1))
        assert np.all(np.abs(dist - 1) > 1e-9), 'a maximum on the search range'


def main():
    ref, run = reference_relocate()
    arrays, names = {}, []
    n_two = 0
    for i, case in enumerate(cases(ref)):
        name, frame, known, args, queries = case[:5]
        want = case[5] if len(case) > 5 else {}
        ndim = frame.ndim
        iso = len(set(_relocate.as_tuple(args['diameter'], ndim))) == 1
        known = np.asarray(known, dtype=np.float64).reshape(-1, ndim)
        is_none, roff = [], [0]
        rows = dict(coords=[], mass=[], signal=[], size=[])
        thr = np.nan
        n_empty = 0
        for sources in queries:
            coords, extra, thr = run(frame, known, sources, args)
            check_edges(frame, known, sources, args, thr)
            is_none.append(coords is None)
            q = len(is_none) - 1
            found = set() if coords is None else set(map(tuple, np.asarray(coords).tolist()))
            empty = coords is None or len(coords) == 0     # (all removed by minmass: empty arrays, not None)
            n_empty += empty
            assert want.get('none', {}).get(q, empty) == empty, (name, q, coords)
            assert q not in want.get('has', {}) or want['has'][q] in found, (name, q, coords)
            assert q not in want.get('has_not', {}) or want['has_not'][q] not in found, (name, q, coords)
            if coords is not None:
                assert len(np.unique(extra['mass'])) == len(coords), 'equal masses in %s' % name
                n_two += len(coords) >= 2
                rows['coords'].append(np.asarray(coords, dtype=np.int64))
                rows['mass'].append(extra['mass'])
                rows['signal'].append(extra['signal'])
                rows['size'].append(_relocate.size_array(extra, ndim, iso))
            roff.append(roff[-1] + (0 if coords is None else len(coords)))
        assert 2 * n_empty <= len(queries), 'fewer than half of the queries of %s have a candidate' % name
        names.append(name)
        arrays['frame_%d' % i] = frame
        arrays['known_%d' % i] = known
        arrays['args_%d' % i] = np.array(json.dumps(args))
        arrays['threshold_%d' % i] = np.array(thr)
        arrays['sources_%d' % i] = np.vstack(queries).astype(np.float64)
        arrays['source_offset_%d' % i] = np.cumsum([0] + [len(s) for s in queries]).astype(np.int64)
        arrays['is_none_%d' % i] = np.array(is_none)
        arrays['result_offset_%d' % i] = np.array(roff, dtype=np.int64)
        arrays['coords_%d' % i] = np.vstack(rows['coords']) if rows['coords'] else np.empty((0, ndim), np.int64)
        for k in ('mass', 'signal'):
            arrays['%s_%d' % (k, i)] = np.concatenate(rows[k]) if rows[k] else np.empty(0)
        arrays['size_%d' % i] = np.concatenate(rows['size']) if rows['size'] else np.empty(0 if iso else (0, ndim))
        print('%-18s %-8s %2d known, %2d queries: %s' % (name, frame.dtype, len(known), len(queries),
                                                       ' '.join('-' if n else str(b - a) for n, a, b in zip(is_none, roff, roff[1:]))))
    assert n_two >= 10, 'only %d queries with two or more candidates' % n_two
    arrays['names'] = np.array(json.dumps(names))
    os.makedirs(os.path.join(HERE, 'relocate'), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, 'relocate', 'relocate_cases.npz'), **arrays)
    print('%d queries with two or more candidates' % n_two)


if __name__ == '__main__':
    main()
