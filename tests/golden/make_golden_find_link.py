"""Generate tests/golden/find_link/find_link_cases.npz: small videos linked by the REFERENCE's
``_find_link_iter`` (find_link.py:914-1008, run through oracle/refshim.py with ``proc_func=None``)
-- what pins ``clustertracking_amd.find_link`` and ``ctr_find_link_device``.

    python tests/golden/make_golden_find_link.py     (build container only: needs the reference)

The reference's own loop is driven; what NumPy 2 and the absent trackpy / pims need is supplied as
in make_golden_relocate.py (the two weight tables, ``find_link.slice_image`` rebound, a
``pims.Frame`` subclass that takes a list of slices, a plain list of such frames as the reader).
``FindLinker.relocate`` is hooked to record sources, shortage and candidates of every call.

Layout: ``names`` (JSON list); per case ``i``: ``frames_i``, ``args_i`` (JSON: diameter, separation,
search_range, memory, minmass, percentile, scale_factor), and the reference's table sorted by
(frame, position): ``pos_i`` float64 [N, ndim], ``frame_i``, ``particle_i`` int64 [N], ``mass_i``,
``signal_i`` [N], ``size_i`` [N] or [N, ndim], ``relocated_i`` bool [N] (the row was a relocation
candidate).

The script asserts what the tests rely on: every case has at least 3 claimed relocations; over all
cases at least 3 claimed in a query of two or more sources, at least 2 queries with more candidates
than shortage, at least 2 relocated rows that are sources of a later link, at least 1 remembered
source that is relocated later; no coupled level; no two candidates of equal mass; no sub-network
above 8 sources; no distance within 1e-9 (relative) of 1, of 2 or of max_dist; in the minmass case,
a query that ``minmass`` takes a candidate from.
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
import _relocate  # noqa: E402
import make_golden_relocate  # noqa: E402


def reference_find_link():
    """run(frames, args) -> (table dict, log of the relocate calls) by the reference"""
    make_golden_relocate.reference_relocate()      # the patches
    mod = sys.modules['clustertracking.find_link']
    pims = sys.modules['pims']

    class ListFrame(pims.Frame):
        def __getitem__(self, key):
            return np.ndarray.__getitem__(self, tuple(key) if isinstance(key, list) else key)

    def run(frames, args):
        ndim = frames.ndim - 1
        tup = lambda v: _relocate.as_tuple(v, ndim)   # noqa: E731
        meta = {'scale_factor': args['scale_factor']} if args['scale_factor'] != 1. else {}
        reader = [ListFrame(f, frame_no=t, metadata=meta) for t, f in enumerate(frames)]
        log = []
        original = mod.FindLinker.relocate

        def relocate(self, source_points, n=1):
            sources = np.array([p.pos for p in source_points], dtype=np.float64)
            with np.errstate(divide='ignore', invalid='ignore'):
                coords, extra = self.get_relocate_candidates(source_points)
                minmass, self.minmass = self.minmass, 0
                everything = self.get_relocate_candidates(source_points)[0]
                self.minmass = minmass
                points = original(self, source_points, n)
            remembered = [p.t < self.image.frame_no - 1 for p in source_points]
            log.append(dict(level=int(self.image.frame_no), sources=sources, shortage=int(n),
                            n_found=0 if coords is None else len(coords),
                            n_before_minmass=0 if everything is None else len(everything),
                            mass=np.zeros(0) if coords is None else np.asarray(extra['mass']),
                            taken=np.array([p.pos for p in points], dtype=np.float64).reshape(-1, ndim),
                            remembered=remembered))
            return points
        mod.FindLinker.relocate = relocate
        try:
            mod.PointND.set_counter() if hasattr(mod.PointND, 'set_counter') else None
            rows = []
            dia = args['diameter']
            with np.errstate(divide='ignore', invalid='ignore'):
                for frame_no, features in mod._find_link_iter(
                        reader, tup(args['search_range']), tup(args['separation']),
                        diameter=tuple(dia) if hasattr(dia, '__iter__') else dia, memory=args['memory'],
                        percentile=args['percentile'], minmass=args['minmass'], proc_func=None):
                    if features is not None and len(features):
                        rows.append(features)
        finally:
            mod.FindLinker.relocate = original
        return rows, log
    return run


def cases():
    """[(name, frames, args)]; the seeds are those at which the reference alone meets the
    conditions that main() asserts"""
    s8, s16 = 2., 300.
    iso = dict(F.ISO2, percentile=64, scale_factor=1.)
    an = dict(F.ANISO2, percentile=64)
    an3 = dict(F.ANISO3, percentile=64)
    out = [
        ('2d_iso_u8_m0', F.video((48, 56), 8, 6, 101, 'uint8'), dict(iso, memory=0, minmass=300 * s8)),
        ('2d_iso_u16_m1', F.video((48, 56), 8, 6, 115, 'uint16'), dict(iso, memory=1, minmass=300 * s16, scale_factor=2.)),
        ('2d_iso_f64_m2', F.video((48, 56), 8, 6, 115, 'float64'), dict(iso, memory=2, minmass=300., scale_factor=0.5)),
        # twins 11.6 pixels apart along x: two lost sources within two search ranges of each other
        ('2d_aniso_u8_m1', F.video((48, 56), 10, 6, 139, 'uint8', size=(1.5, 1.9), twin_offset=(0., 11.6), walkers=0.4,
                                   noise=10.), dict(an, memory=1, minmass=220 * s8, scale_factor=2.)),
        ('3d_aniso_u8_m0', F.video((16, 24, 24), 6, 4, 112, 'uint8', size=(1.3, 1.7, 1.7), drift=1., margin=(2, 3, 3)),
         dict(an3, memory=0, minmass=300 * s8, scale_factor=2.)),
        # a minmass above the mass of a feature that the edge of the frame cuts
        ('2d_minmass_u8_m0', F.video((48, 56), 8, 6, 101, 'uint8'), dict(iso, memory=0, minmass=900 * s8)),
        ('2d_scale1_u16_m2', F.video((48, 56), 10, 7, 101, 'uint16'), dict(iso, memory=2, minmass=300 * s16)),
    ]
    # a separation below two search ranges: a second, dimmer maximum in the margin within reach of
    # the lost source -- more candidates than the sub-network is short of
    walk = [(3, 20), (1, 22), (3, 23), (1, 25), (3, 26), (1, 28), (3, 29)]
    spots = [[(y, x, 200), (30, 30 + 0.5 * t, 180)] + ([(1, x - 5, 150)] if y == 1 else [])
             for t, (y, x) in enumerate(walk)]
    out.append(('2d_spare_u8_m0', F.spot_frames((48, 56), spots, width=1.0),
                dict(diameter=5, separation=5, search_range=4, memory=0, minmass=100, percentile=64, scale_factor=1.)))
    return out


def check_case(name, frames, args, rows, log):
    """(arrays of the case, counts) -- asserts the per-case conditions"""
    import pandas as pd
    ndim = frames.ndim - 1
    iso = F.is_isotropic(args)
    counts = dict(multi=0, spare=0, reused=0, remembered=0)
    if 'minmass' in name:
        assert any(q['n_before_minmass'] > q['n_found'] for q in log), 'minmass removes no candidate in %s' % name
    cols = ['z', 'y', 'x'][3 - ndim:]
    table = pd.concat(rows, ignore_index=True)
    pos = table[cols].values.astype(np.float64)
    order = np.lexsort(tuple(pos.T[::-1]) + (table['frame'].values,))
    table = table.iloc[order].reset_index(drop=True)
    pos = pos[order]
    fr = table['frame'].values.astype(np.int64)
    present = {(int(f),) + tuple(p) for f, p in zip(fr, pos.tolist())}
    taken = {(q['level'],) + tuple(p) for q in log for p in q['taken'].tolist()}
    reloc = np.array([(int(f),) + tuple(p) in taken for f, p in zip(fr, pos.tolist())], dtype=bool)
    assert int(reloc.sum()) >= 3, 'fewer than 3 claimed relocations in %s' % name
    d = _relocate.derived(*(_relocate.as_tuple(args[k], ndim) for k in ('diameter', 'separation', 'search_range')))
    sr = np.array(_relocate.as_tuple(args['search_range'], ndim), dtype=np.float64)
    for q in log:
        assert len(q['sources']) <= 8, 'a sub-network above 8 sources in %s' % name
        assert len(np.unique(q['mass'])) == len(q['mass']), 'equal masses in %s' % name
        claimed_here = [p for p in q['taken'].tolist() if (q['level'],) + tuple(p) in present]
        counts['multi'] += len(claimed_here) if len(q['sources']) >= 2 else 0
        counts['spare'] += q['n_found'] > q['shortage']
        counts['remembered'] += bool(claimed_here) and any(q['remembered'])
        # coupled: a claimed candidate within max_dist of a source of another query of the level
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
    # distances between the rows of consecutive frames: none on 1 or 2
    for t in range(1, len(frames)):
        a, b = pos[fr == t - 1], pos[fr == t]
        for p in b:
            if len(a):
                dist = F._scaled_dist(p, a, sr)
                assert np.all(np.abs(dist - 1) > 1e-9) and np.all(np.abs(dist / 2 - 1) > 1e-9), 'a distance on 1 or 2'
        for p in a:
            dist = F._scaled_dist(p, a, sr)
            assert np.all(np.abs(dist / 2 - 1) > 1e-9), 'two sources at 2 search ranges in %s' % name
    part = table['particle'].values.astype(np.int64)
    for k in np.flatnonzero(reloc):     # relocated rows that are sources of a later link
        counts['reused'] += bool(np.any((part == part[k]) & (fr == fr[k] + 1)))
    keys = ['size'] if iso else ['size_z', 'size_y', 'size_x'][3 - ndim:]
    arrays = dict(frames=frames, args=np.array(json.dumps(args)), pos=pos, frame=fr, particle=part,
                  mass=table['mass'].values.astype(np.float64), signal=table['signal'].values.astype(np.float64),
                  size=table[keys[0]].values if iso else table[keys].values, relocated=reloc)
    return arrays, counts


def main():
    run = reference_find_link()
    arrays, names = {}, []
    totals = dict(multi=0, spare=0, reused=0, remembered=0)
    for i, (name, frames, args) in enumerate(cases()):
        rows, log = run(frames, args)
        case, counts = check_case(name, frames, args, rows, log)
        print('%-18s %d rows, %d relocate calls, %d claimed %s' % (name, len(case['pos']), len(log),
                                                                  int(case['relocated'].sum()), counts))
        for k, v in counts.items():
            totals[k] += int(v)
        names.append(name)
        for k, v in case.items():
            arrays['%s_%d' % (k, i)] = v
    print(totals)
    assert totals['multi'] >= 3, 'fewer than 3 claimed in a query of two or more sources'
    assert totals['spare'] >= 2, 'fewer than 2 queries with more candidates than shortage'
    assert totals['reused'] >= 2, 'fewer than 2 relocated rows that are sources of a later link'
    assert totals['remembered'] >= 1, 'no remembered source that is relocated later'
    arrays['names'] = np.array(json.dumps(names))
    os.makedirs(os.path.join(HERE, 'find_link'), exist_ok=True)
    path = os.path.join(HERE, 'find_link', 'find_link_cases.npz')
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 512 * 1024, 'the fixture file is too large'
    print('%d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
