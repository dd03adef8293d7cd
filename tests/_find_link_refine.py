"""The yardstick of ``find_link(refine=True)``: the loop of tests/_find_link.py's
``link_relocate`` with the centre-of-mass refinement of tests/_refine_com.py after every level, as
the reference's ``after_link`` callback and ``linker.set_dataframe`` apply it (find_link.py:451-465,
651-654, 1001-1007): the rows of a level, the relocated ones included, are refined on the RAW frame
once the level is linked, and the refined positions are the sources of the next level (a remembered
row keeps what it had).  ``F.link_level`` is called unchanged."""
import json
import os

import numpy as np

import _characterize
import _find_link as F
import _locate
import _refine_com as RC
import _relocate


def link_relocate(frames, raw_frames, thresholds, levels, level_extras, diameter, separation, search_range, memory=0,
                  minmass=0, isotropic=None, scale_factor=1., max_queries=None, max_relocated=None, log=None,
                  max_iterations=RC.MAX_ITERATIONS, shift_thresh=RC.SHIFT_THRESH):
    """``F.link_relocate`` with the refinement.  frames: what the relocation looks at; raw_frames:
    what the refinement reads.  Returns its dict, ``pos`` and ``mass`` refined, plus per row
    ``start`` (the whole-pixel position), ``n_iter``, ``clipped`` and the list ``offs``."""
    frames, raw_frames = np.asarray(frames), np.asarray(raw_frames)
    ndim = frames.ndim - 1
    diameter, separation, search_range = (_relocate.as_tuple(v, ndim) for v in (diameter, separation, search_range))
    radius = tuple(int(x // 2) for x in diameter)
    if isotropic is None:
        isotropic = all(x == diameter[0] for x in diameter)
    keys = _characterize.size_keys(ndim, isotropic) + ['mass', 'signal']
    next_id = 0
    src_pos, src_id = np.zeros((0, ndim)), np.zeros(0, dtype=np.int64)
    mem_pos, mem_id, mem_age = np.zeros((0, ndim)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    out = dict(pos=[], start=[], frame=[], particle=[], relocated=[], coupled=[], n_iter=[], clipped=[])
    out.update({k: [] for k in keys})
    all_offs = []
    for t, pos in enumerate(levels):
        pos = np.asarray(pos, dtype=np.float64).reshape(-1, ndim)
        n = len(pos)
        extras = {k: np.asarray(level_extras[t][k], dtype=np.float64) for k in keys}
        coupled = False
        if t == 0:
            ids = np.arange(n, dtype=np.int64)
            next_id = n
            rows = pos
        else:
            all_src_pos = np.concatenate([src_pos, mem_pos])
            all_src_id = np.concatenate([src_id, mem_id])
            thr = thresholds[t]
            link, cpos, cextra, coupled = F.link_level(
                frames[t], None if thr is None or np.isnan(thr) else thr, pos, all_src_pos, diameter, separation,
                search_range, minmass, isotropic, scale_factor, t, max_queries, max_relocated, log)
            rows = np.concatenate([pos, cpos.astype(np.float64)])
            extras = {k: np.concatenate([extras[k], cextra[k]]) for k in keys}
            ids = np.full(len(rows), -1, dtype=np.int64)
            linked = link >= 0
            ids[linked] = all_src_id[link[linked]]
            new = np.flatnonzero(~linked)       # located rows only: a relocated row is always linked
            if len(new):
                order = np.lexsort(rows[new].T[::-1])       # births are numbered where they were located
                ids[new[order]] = next_id + np.arange(len(new))
                next_id += len(new)
            if memory > 0:
                used = np.zeros(len(all_src_pos), dtype=bool)
                used[link[linked]] = True
                lost_new = ~used[:len(src_pos)]
                keep_mem = ~used[len(src_pos):] & (mem_age + 1 < memory)
                mem_pos = np.concatenate([mem_pos[keep_mem], src_pos[lost_new]])
                mem_id = np.concatenate([mem_id[keep_mem], src_id[lost_new]])
                mem_age = np.concatenate([mem_age[keep_mem] + 1, np.zeros(int(lost_new.sum()), dtype=np.int64)])
        # ---- the refinement of the level (after_link, then set_dataframe)
        r = RC.compose(raw_frames[t][None], rows, [0, len(rows)], radius, max_iterations, shift_thresh)
        extras['mass'] = r['mass']
        out['start'].append(rows)
        out['pos'].append(r['pos'])
        out['n_iter'].append(r['n_iter'])
        out['clipped'].append(r['clipped'])
        all_offs.extend(r['offs'])
        out['frame'].append(np.full(len(rows), t, dtype=np.int64))
        out['particle'].append(ids)
        out['relocated'].append(np.arange(len(rows)) >= n)
        out['coupled'].append(coupled)
        for k in keys:
            out[k].append(extras[k])
        src_pos, src_id = r['pos'], ids
    counts = [len(p) for p in out['pos']]
    res = {k: (np.concatenate(v) if len(v) else np.zeros(0)) for k, v in out.items() if k != 'coupled'}
    res['pos'] = res['pos'].reshape(-1, ndim)
    res['start'] = res['start'].reshape(-1, ndim)
    res['coupled'] = np.array(out['coupled'], dtype=bool)
    res['frame_offset'] = np.r_[0, np.cumsum(counts)].astype(np.int64)
    res['n_tracks'] = next_id
    res['offs'] = all_offs
    return res


def find_link(frames, search_range, separation, diameter=None, memory=0, minmass=0, percentile=64,
              raw_frames=None, scale_factor=1., max_queries=None, max_relocated=None, log=None,
              max_iterations=RC.MAX_ITERATIONS, shift_thresh=RC.SHIFT_THRESH):
    """``F.find_link`` with the refinement after every level: maxima of ``frames``, mass, signal and
    size of the located rows from ``raw_frames`` (default: the same frames), ``mass >= minmass``,
    then :func:`link_relocate`, which refines on the raw frames."""
    frames = np.asarray(frames)
    raw = frames if raw_frames is None else np.asarray(raw_frames)
    ndim = frames.ndim - 1
    separation = _relocate.as_tuple(separation, ndim)
    isotropic = not hasattr(diameter, '__iter__') or all(x == diameter[0] for x in diameter)
    diameter = separation if diameter is None else _relocate.as_tuple(diameter, ndim)
    radius = tuple(int(x // 2) for x in diameter)
    margin = tuple(int(max(x // 2, s // 2 - 1)) for x, s in zip(diameter, separation))
    levels, extras, thresholds = [], [], []
    for t in range(len(frames)):
        pos = np.asarray(_locate.compose(frames[t], separation, percentile, margin, True), dtype=np.float64).reshape(-1, ndim)
        ex = _characterize.compose(pos, raw[t], radius, isotropic, scale_factor if raw_frames is None else 1.)
        with np.errstate(invalid='ignore'):
            keep = ex['mass'] >= minmass
        levels.append(pos[keep])
        extras.append({k: v[keep] for k, v in ex.items()})
        thresholds.append(_locate.percentile_threshold(frames[t], percentile))
    return link_relocate(frames, raw, thresholds, levels, extras, diameter, separation, search_range, memory, minmass,
                         isotropic, scale_factor, max_queries, max_relocated, log, max_iterations, shift_thresh)


# ---- the constructed pair: refinement decides whether a track continues --------------------------
# diameter 7 (radius 3), separation 7, search range 3.9.  Frame 0 holds one feature whose maximum is
# the pixel (12, 20) and whose centre of mass lies 164 / 364 = 0.4505 pixels from it along x (below
# the shift threshold of 0.6: the window stays); frame 1 holds one symmetric feature.  A destination
# is linked from where it was located, a source from where it was refined to.
PAIR_KW = dict(diameter=7, separation=7, search_range=3.9, minmass=100, memory=0)
PAIR_SHAPE = (24, 48)


def _leaning(y, x, toward):
    im = np.zeros(PAIR_SHAPE, dtype=np.uint8)
    im[y, x] = 200
    im[y, x + toward] = 164
    return im


def _round_spot(y, x):
    im = np.zeros(PAIR_SHAPE, dtype=np.uint8)
    im[y, x] = 200
    im[y - 1, x] = im[y + 1, x] = im[y, x - 1] = im[y, x + 1] = 60
    return im


def pair_cases():
    """{name: (frames, kwargs)}.
    'only_with': the source leans towards the destination at (12, 24): 4 whole pixels, beyond the
    search range; 3.55 from the centre of mass near x = 20.45, within.
    'only_without': the source leans away from the destination at (14, 23): sqrt(4 + 9) = 3.61 in
    whole pixels, within; sqrt(4 + 3.45^2) = 3.99 from the centre of mass near x = 19.55, beyond."""
    return {'only_with': (np.stack([_leaning(12, 20, +1), _round_spot(12, 24)]), dict(PAIR_KW)),
            'only_without': (np.stack([_leaning(12, 20, -1), _round_spot(14, 23)]), dict(PAIR_KW))}


# ---- fixtures ------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'find_link', 'find_link_refine_cases.npz')


def fixtures():
    """[(name, frames, kwargs, the reference's table as a dict sorted by (frame, refined position))]
    of tests/golden/find_link/find_link_refine_cases.npz (tests/golden/make_golden_find_link_refine.py)"""
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(json.loads(str(z['names']))):
        args = json.loads(str(z['args_%d' % i]))
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in args.items()}
        frames = z['frames_%d' % i]
        ndim = frames.ndim - 1
        want = {k: z['%s_%d' % (k, i)] for k in ('pos', 'frame', 'particle', 'mass', 'signal', 'relocated')}
        size = z['size_%d' % i].reshape(len(want['pos']), -1)
        for a, k in enumerate(_characterize.size_keys(ndim, F.is_isotropic(kw))):
            want[k] = size[:, a]
        out.append((name, frames, kw, want))
    return out


def assert_equals_fixture(got, want, ndim, isotropic, exact):
    """a result against the reference's table, both sorted by (frame, position): particle, frame
    and relocated identical; positions and mass bit for bit (``exact``: integer frames) or to
    1e-10 / rtol 1e-12 (float64 frames); signal and size bit for bit or to rtol 1e-12"""
    o = F.sorted_rows(got, ndim)
    assert len(o) == len(want['pos'])
    assert np.array_equal(np.asarray(got['frame'])[o], want['frame'])
    assert np.array_equal(np.asarray(got['particle'])[o], want['particle'])
    assert np.array_equal(np.asarray(got['relocated'])[o], want['relocated'])
    assert not np.asarray(got['coupled']).any()
    pos = got['pos'].reshape(-1, ndim)[o]
    if exact:
        assert np.array_equal(pos, want['pos'])
    else:
        np.testing.assert_allclose(pos, want['pos'], rtol=0, atol=1e-10)
    for k in _characterize.size_keys(ndim, isotropic) + ['mass', 'signal']:
        x, y = np.asarray(got[k])[o], want[k]
        if exact:
            assert np.array_equal(x, y), k
        else:
            np.testing.assert_allclose(x, y, rtol=1e-12, atol=0, err_msg=k)


def assert_same(got, want, ndim, isotropic, exact):
    """two results (dicts as :func:`link_relocate` returns) on the levels that neither flags
    coupled, rows sorted by (frame, position), and ``coupled`` itself: particle, frame and relocated
    identical; positions and mass bit for bit (``exact``) or to 1e-10 / rtol 1e-12; signal and size
    bit for bit or to rtol 1e-12.  Without a coupled level also ``frame_offset`` and ``n_tracks``."""
    coupled = np.asarray(want['coupled'], dtype=bool)
    assert np.array_equal(np.asarray(got['coupled'], dtype=bool), coupled)
    if not coupled.any():
        assert np.array_equal(got['frame_offset'], want['frame_offset']) and int(got['n_tracks']) == int(want['n_tracks'])
    a, b = F.sorted_rows(got, ndim), F.sorted_rows(want, ndim)
    a = a[~coupled[np.asarray(got['frame'])[a]]]
    b = b[~coupled[np.asarray(want['frame'])[b]]]
    assert len(a) == len(b)
    for k in ('frame', 'particle', 'relocated'):
        assert np.array_equal(np.asarray(got[k])[a], np.asarray(want[k])[b]), k
    x, y = got['pos'].reshape(-1, ndim)[a], want['pos'].reshape(-1, ndim)[b]
    if exact:
        assert np.array_equal(x, y)
    else:
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-10)
    for k in _characterize.size_keys(ndim, isotropic) + ['mass', 'signal']:
        x, y = np.asarray(got[k])[a], np.asarray(want[k])[b]
        if exact:
            assert np.array_equal(x, y, equal_nan=True), k
        else:
            np.testing.assert_allclose(x, y, rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
