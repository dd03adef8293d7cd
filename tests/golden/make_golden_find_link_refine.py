"""Generate tests/golden/find_link/find_link_refine_cases.npz: small videos linked by the REFERENCE's
``_find_link_iter`` (find_link.py:914-1008) with an ``after_link`` callback that refines every
level by centre of mass, as ``find_link(refine=True)`` installs one (find_link.py:451-465) -- what
pins the loop of ``ctr_find_link_refine_device`` and ``find_link(refine=True)``.

    python tests/golden/make_golden_find_link_refine.py     (build container only: needs the reference)

The reference's callback calls ``trackpy.refine``, and trackpy is not installed: the callback here
applies tests/_refine_com.py, the restated rule, to the raw ``image`` and sets the position columns
and ``mass``.  So the fixtures pin the reference's LOOP around the refinement (what is refined when,
``linker.set_dataframe``, which positions the next level and the relocation measure from), not
trackpy's arithmetic.  The reference is driven exactly as make_golden_find_link.py drives it (its
``reference_find_link``), with ``_find_link_iter`` given the callback.

Layout: as find_link_cases.npz -- ``names``; per case ``frames_i``, ``args_i``, and the reference's
table sorted by (frame, refined position): ``pos_i`` (refined), ``frame_i``, ``particle_i``,
``mass_i`` (the refinement's), ``signal_i``, ``size_i``, ``relocated_i`` -- plus ``start_i`` (the
whole-pixel position the row had when it was linked), ``n_iter_i`` and ``clipped_i``.

The script asserts, for the reference alone: every case has at least 3 claimed relocations; over
all cases at least 2 relocated rows are sources of a later link, at least 10 rows have
``n_iter >= 2`` and at least 1 row's start is clipped; no coupled level; no distance within 1e-9
(relative) of 1, 2 or max_dist, computed from the refined sources; on the float64 case no
``abs(off)`` within 1e-9 of ``shift_thresh`` at any evaluated window.
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
import refshim  # noqa: E402,F401
import _find_link as F  # noqa: E402
import _refine_com as RC  # noqa: E402
import _relocate  # noqa: E402
import make_golden_find_link as G  # noqa: E402

CASES = ('2d_iso_u8_m0', '2d_iso_u16_m1', '2d_iso_f64_m2', '3d_aniso_u8_m0')


def reference_find_link_refine():
    """run(frames, args) -> (rows, log of the relocate calls, offs of every window) by the reference"""
    run_plain = G.reference_find_link()
    mod = sys.modules['clustertracking.find_link']

    def run(frames, args):
        ndim = frames.ndim - 1
        cols = ['z', 'y', 'x'][3 - ndim:]
        radius = tuple(int(d // 2) for d in _relocate.as_tuple(args['diameter'], ndim))
        all_offs = []

        def after_link(features, image, **kwargs):
            coords = features[cols].values.astype(np.float64)
            r = RC.compose(np.asarray(image)[None], coords, [0, len(coords)], radius)
            for a, c in enumerate(cols):
                features['start_' + c] = coords[:, a]
            features[cols] = r['pos']
            features['mass'] = r['mass']
            features['n_iter'] = r['n_iter']
            features['clipped'] = r['clipped']
            all_offs.extend(r['offs'])
            return features
        original = mod._find_link_iter
        mod._find_link_iter = lambda *a, **k: original(*a, after_link=after_link, **k)
        try:
            rows, log = run_plain(frames, args)
        finally:
            mod._find_link_iter = original
        return rows, log, all_offs
    return run


def cases():
    wanted = {name: (frames, args) for name, frames, args in G.cases()}
    return [(name,) + wanted[name] for name in CASES]


def check_case(name, frames, args, rows, log, offs):
    """(arrays of the case, counts) -- asserts the per-case conditions"""
    import pandas as pd
    ndim = frames.ndim - 1
    iso = F.is_isotropic(args)
    cols = ['z', 'y', 'x'][3 - ndim:]
    table = pd.concat(rows, ignore_index=True)
    pos = table[cols].values.astype(np.float64)
    order = np.lexsort(tuple(pos.T[::-1]) + (table['frame'].values,))
    table = table.iloc[order].reset_index(drop=True)
    pos = pos[order]
    start = table[['start_' + c for c in cols]].values.astype(np.float64)
    fr = table['frame'].values.astype(np.int64)
    present = {(int(f),) + tuple(p) for f, p in zip(fr, start.tolist())}
    taken = {(q['level'],) + tuple(p) for q in log for p in q['taken'].tolist()}
    reloc = np.array([(int(f),) + tuple(p) in taken for f, p in zip(fr, start.tolist())], dtype=bool)
    assert int(reloc.sum()) >= 3, 'fewer than 3 claimed relocations in %s' % name
    d = _relocate.derived(*(_relocate.as_tuple(args[k], ndim) for k in ('diameter', 'separation', 'search_range')))
    sr = np.array(_relocate.as_tuple(args['search_range'], ndim), dtype=np.float64)
    for q in log:       # q['sources']: the points' positions when the query was issued -- refined
        claimed_here = [p for p in q['taken'].tolist() if (q['level'],) + tuple(p) in present]
        for other in log:
            if other is q or other['level'] != q['level']:
                continue
            for p in claimed_here:
                dist = F._scaled_dist(np.asarray(p, dtype=np.float64), other['sources'], sr)
                assert np.all(dist > d['max_dist']), 'a coupled level in %s' % name
                assert np.all(np.abs(dist / d['max_dist'] - 1) > 1e-9)
        for p in q['taken'].tolist():
            dist = F._scaled_dist(np.asarray(p, dtype=np.float64), q['sources'], sr)
            assert np.all(np.abs(dist - 1) > 1e-9), 'a candidate on the search range in %s' % name
        for s in q['sources']:      # the background: known features within max_dist of a source
            known = start[(fr == q['level']) & ~reloc]
            if len(known):
                dist = F._scaled_dist(s, known, sr)
                assert np.all(np.abs(dist / d['max_dist'] - 1) > 1e-9), 'a known feature on max_dist in %s' % name
    # a destination is linked from where it was located, a source from where it was refined to
    for t in range(1, len(frames)):
        a, b = pos[fr == t - 1], start[fr == t]
        for p in b:
            if len(a):
                dist = F._scaled_dist(p, a, sr)
                assert np.all(np.abs(dist - 1) > 1e-9) and np.all(np.abs(dist / 2 - 1) > 1e-9), 'a distance on 1 or 2'
        for p in a:
            dist = F._scaled_dist(p, a, sr)
            assert np.all(np.abs(dist / 2 - 1) > 1e-9), 'two sources at 2 search ranges in %s' % name
    if frames.dtype.kind == 'f':
        assert RC.min_gap(offs) > 1e-9, 'an offset on the shift threshold in %s' % name
    part = table['particle'].values.astype(np.int64)
    counts = dict(reused=0, walked=int((table['n_iter'].values >= 2).sum()), clipped=int(table['clipped'].values.sum()))
    for k in np.flatnonzero(reloc):     # relocated rows that are sources of a later link
        counts['reused'] += bool(np.any((part == part[k]) & (fr == fr[k] + 1)))
    keys = ['size'] if iso else ['size_z', 'size_y', 'size_x'][3 - ndim:]
    arrays = dict(frames=frames, args=np.array(json.dumps(args)), pos=pos, start=start, frame=fr, particle=part,
                  mass=table['mass'].values.astype(np.float64), signal=table['signal'].values.astype(np.float64),
                  size=table[keys[0]].values if iso else table[keys].values, relocated=reloc,
                  n_iter=table['n_iter'].values.astype(np.int32), clipped=table['clipped'].values.astype(bool))
    return arrays, counts


def main():
    run = reference_find_link_refine()
    arrays, names = {}, []
    totals = dict(reused=0, walked=0, clipped=0)
    for i, (name, frames, args) in enumerate(cases()):
        rows, log, offs = run(frames, args)
        case, counts = check_case(name, frames, args, rows, log, offs)
        print('%-18s %d rows, %d relocate calls, %d claimed %s' % (name, len(case['pos']), len(log),
                                                                  int(case['relocated'].sum()), counts))
        for k, v in counts.items():
            totals[k] += int(v)
        names.append(name)
        for k, v in case.items():
            arrays['%s_%d' % (k, i)] = v
    print(totals)
    assert totals['reused'] >= 2, 'fewer than 2 relocated rows that are sources of a later link'
    assert totals['walked'] >= 10, 'fewer than 10 rows with n_iter >= 2'
    assert totals['clipped'] >= 1, 'no row whose start is clipped'
    arrays['names'] = np.array(json.dumps(names))
    os.makedirs(os.path.join(HERE, 'find_link'), exist_ok=True)
    path = os.path.join(HERE, 'find_link', 'find_link_refine_cases.npz')
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 512 * 1024, 'the fixture file is too large'
    print('%d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
