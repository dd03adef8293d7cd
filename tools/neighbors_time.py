"""Time the neighbours stage on the MI355X (ctr_neighbors_device) against
``scipy.spatial.cKDTree.query`` on the host, one tree per frame, which is what a user of trackpy does today.

    python tools/neighbors_time.py [--reps 20] [--frames 1250] [--rows 20000] [--out profiles/neighbors_time.json]

Two tables.  ``cfg2``: the positions that ``find_link_arrays`` returns for `--frames` cfg-2 frames (512 x
512 uint8, 200 Gaussians each, diameter 13, separation 13, search range 5) with ``minmass = 0``, so the
noise maxima are rows too (where the linker refuses the table, ``locate_arrays`` of the same frames
gives it; the file says which): the table of ``tools/pair_correlation_time.py``.  ``one_frame``: `--rows`
uniform points in a 2048 x 2048 box, one frame.  ``k = 1`` and ``k = 16``, ``lag = 0``, no ``max_dist``, the table
on the device and the results left there; HIP events on a stream of its own around one call after a
warm-up call, median / minimum / maximum of `reps`.  Next to it, wall clock on one core in the same
process, one run: a ``cKDTree`` per frame built and queried for ``k + 1`` (the row itself comes first).
The device's ``dist2``, ``index`` and ``count`` must equal the rule restated in NumPy
(``tests/_neighbors.py``); against cKDTree the share of equal indices (ties may fall the other way there)
and the largest relative difference of the distances are recorded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

DIAMETER, SEPARATION, SEARCH_RANGE = 13, 13, 5
KS = (1, 16)


def spread(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--rows', type=int, default=20000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    from scipy.spatial import cKDTree
    import _neighbors as yard
    import clustertracking_amd as ct
    from clustertracking_amd import _abi, _lib, workloads
    from clustertracking_amd.find import locate_arrays
    from clustertracking_amd.link import SubnetOversizeException

    _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    own = torch.cuda.Stream(dev)

    def timed(fn):
        with torch.cuda.stream(own):
            out = fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(own)
                fn()
                b.record(own)
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
        return out, spread(ms)

    def host_trees(pos, off, k):
        """(dist [N, k], index [N, k]) of one cKDTree per frame, the row itself dropped; inf and N where a
        frame has fewer rows"""
        dist = np.full((len(pos), k), np.inf)
        index = np.full((len(pos), k), -1, dtype=np.int64)
        for t in range(len(off) - 1):
            r0, r1 = int(off[t]), int(off[t + 1])
            if r1 - r0 < 2:
                continue
            d, j = cKDTree(pos[r0:r1]).query(pos[r0:r1], k=min(k + 1, r1 - r0))
            m = d.shape[1] - 1
            dist[r0:r1, :m] = d[:, 1:]
            index[r0:r1, :m] = j[:, 1:] + r0
        return dist, index

    def measure(name, t_pos, t_off):
        pos, off = t_pos.cpu().numpy(), t_off.cpu().numpy()
        res, ok = {}, True
        most = yard.neighbors(pos, off, k=max(KS))      # the first k of the most are the k nearest
        print(name, 'restated', flush=True)
        for k in KS:
            got, r = timed(lambda: ct.neighbors_arrays(t_pos, t_off, k=k))
            ok = ok and int(got.status) == _abi.NBR_OK
            dist, dist2, index, count = (x.cpu().numpy() for x in got[:4])
            want = yard.Result(None, np.ascontiguousarray(most.dist2[:, :k]), most.index[:, :k], most.count, None, None)
            none = np.isnan(want.dist2)
            same = bool((index == want.index).all() and (count == want.count).all() and np.array_equal(np.isnan(dist2), none)
                        and np.where(none, 0., dist2).tobytes() == np.where(none, 0., want.dist2).tobytes())
            t0 = time.perf_counter()
            h_dist, h_index = host_trees(pos, off, k)
            host_ms = (time.perf_counter() - t0) * 1e3
            found = index >= 0
            with np.errstate(invalid='ignore', divide='ignore'):
                rel = np.abs(dist[found] - h_dist[found]) / h_dist[found]
            r.update(host_ckdtree_ms=host_ms, equals_the_restatement=same,
                     sqrt_ulp_from_numpy=yard.ulps(dist, np.sqrt(want.dist2)),
                     share_of_indices_equal_to_ckdtree=float((index == h_index).mean()) if index.size else 1.,
                     largest_relative_difference_to_ckdtree=float(np.nanmax(rel)) if rel.size else 0.,
                     median_nearest_distance=float(np.nanmedian(dist[:, 0])) if dist.size else 0.)
            res['k%d' % k] = r
            ok = ok and same
            print(name, 'k', k, r, flush=True)
        shape = dict(frames=int(len(off) - 1), rows=int(len(pos)), rows_per_frame=float(len(pos)) / max(len(off) - 1, 1),
                     distance_evaluations=int((np.diff(off) ** 2).sum()))
        return shape, res, ok

    frames = workloads.cfg2(n_frames=args.frames)[0]
    print('drawn', flush=True)
    d_frames = torch.from_numpy(frames).to(dev)
    try:
        r = ct.find_link_arrays(d_frames, search_range=SEARCH_RANGE, separation=SEPARATION, diameter=DIAMETER, minmass=0,
                                max_queries=1024, max_relocated=1024, _on_device=True)
        t_pos, t_off, source = r.pos, r.frame_offset, 'find_link_arrays'
    except (_lib.EngineError, SubnetOversizeException) as e:
        print('find_link_arrays refused the table (%s): locate_arrays instead' % e, flush=True)
        _, _, pos_i, t_off, _ = locate_arrays(d_frames, SEPARATION, 64, (DIAMETER // 2,) * 2, _on_device=True)
        t_pos, source = pos_i.to(torch.float64), 'locate_arrays (find_link_arrays refused: %s)' % e
    del d_frames
    print('located', int(t_pos.shape[0]), 'rows', flush=True)
    shape_a, res_a, ok_a = measure('cfg2', t_pos, t_off)
    shape_a.update(generator='workloads.cfg2(n_frames=%d), minmass 0' % args.frames, table=source, diameter=DIAMETER,
                   separation=SEPARATION, search_range=SEARCH_RANGE)

    rng = np.random.RandomState(7)
    one = torch.from_numpy(rng.uniform(0., 2048., (args.rows, 2))).to(dev)
    shape_b, res_b, ok_b = measure('one_frame', one, torch.tensor([0, args.rows], dtype=torch.int64, device=dev))
    shape_b.update(generator='uniform points in a 2048 x 2048 box, one frame')

    out = dict(
        method=dict(reps=args.reps, warmup_calls=1, k=list(KS), lag=0, max_dist=None,
                    clock='HIP events on a stream of its own around one call; median, minimum and maximum of reps',
                    inputs='the table on the device, results left there',
                    host='wall clock, one core, one run, the same process: scipy.spatial.cKDTree per frame, built and '
                         'queried for k + 1; not trackpy',
                    max_k=_abi.NBR_MAX_K),
        cfg2=dict(workload=shape_a, device=res_a), one_frame=dict(workload=shape_b, device=res_b))
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not (ok_a and ok_b):
        sys.exit('the device and the rule restated in NumPy disagree')


if __name__ == '__main__':
    main()
