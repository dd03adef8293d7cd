"""Time the van Hove stage on the MI355X (ctr_vanhove_device) against the host's
pivot-and-histogram of the same table in NumPy.

    python tools/vanhove_time.py [--reps 5] [--frames 1250] [--out profiles/vanhove_time.json]

Three tables, generated from a seed.  ``stubs``: 262 144 tracks of three consecutive frames each, starting
anywhere in `--frames` frames (786 432 rows, 1024 chunks of ids): the shape of a linked table of
accidental links.  ``stubs_at_rest``: the same tracks without a step, every pair in the central bin: the
most that the LDS counters can be contended.  ``walks``: 200 random walks present in every one of
`--frames` frames (one chunk, so one workgroup per lag: the table that the launch cannot spread).  The
moving ones with a step of 0.7 px per axis, mpp 0.16, so the displacements of lag 1 spread over some 60
bins of 0.01 around the centre.  Timed on
each, the table on the device and the results left there, ``n_particles`` given (no host copy inside),
torch's stable sort of the ids included: HIP events on a stream of its own around one call after a
warm-up call, median / minimum / maximum of `reps`, and per call for 50 calls queued back to back.
Next to each, wall clock on one core in the same process, one run: the rows sorted by (particle,
frame), a ``searchsorted`` per lag for the pairs, ``searchsorted`` against the same edges and
``bincount`` for the histograms.  The device's counts and tails must equal the host's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MPP, WIDTH = 0.16, 0.01
LAGS = [1, 2, 5, 10, 20, 50, 100]


def host_vanhove(pos, off, particle, lags, edges, edge2, mpp):
    """(n, count, below, above, count_r, above_r) by the rule, vectorised; the sort is part of it"""
    T = len(off) - 1
    half = len(edge2) - 1
    frame = np.repeat(np.arange(T), np.diff(off))
    keep = particle >= 0
    key, first = np.unique(particle[keep] * T + frame[keep], return_index=True)
    spos, sframe = pos[keep][first], key % T
    nd = pos.shape[1]
    K = len(lags)
    n, count = np.zeros(K, dtype=np.int64), np.zeros((K, nd, 2 * half), dtype=np.int64)
    below, above = np.zeros((K, nd), dtype=np.int64), np.zeros((K, nd), dtype=np.int64)
    count_r, above_r = np.zeros((K, half), dtype=np.int64), np.zeros(K, dtype=np.int64)
    for q, k in enumerate(lags):
        at = np.searchsorted(key, key + k)
        ok = (sframe + k < T) & (at < len(key))
        ok[ok] = key[at[ok]] == key[ok] + k
        d = (spos[at[ok]] - spos[ok]) * mpp
        n[q] = len(d)
        for a in range(nd):
            b = np.bincount(np.searchsorted(edges, d[:, a], side='right'), minlength=2 * half + 2)
            below[q, a], count[q, a], above[q, a] = b[0], b[1:2 * half + 1], b[2 * half + 1]
        d2 = d[:, 0] * d[:, 0]
        for a in range(1, nd):
            d2 = d2 + d[:, a] * d[:, a]
        b = np.bincount(np.searchsorted(edge2, d2, side='right'), minlength=half + 2)
        count_r[q], above_r[q] = b[1:half + 1], b[half + 1]
    return n, count, below, above, count_r, above_r


def spread(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--tracks', type=int, default=262144)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import clustertracking_amd as ct
    from clustertracking_amd import _abi, _lib
    vh = sys.modules['clustertracking_amd.vanhove']

    _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    F = args.frames
    own = torch.cuda.Stream(dev)
    rng = np.random.RandomState(7)

    # stubs: tracks of three frames; rows sorted by frame, the rows of a frame in track order
    P = args.tracks
    start = rng.randint(0, F - 2, P)
    frame = (start[:, None] + np.arange(3)).reshape(-1)
    par = np.repeat(np.arange(P), 3)
    origin = rng.uniform(0., 512., (P, 1, 2))
    pos = (origin + np.cumsum(rng.normal(0., 0.7, (P, 3, 2)), axis=1)).reshape(-1, 2)
    order = np.argsort(frame, kind='stable')
    stubs = (pos[order], np.searchsorted(frame[order], np.arange(F + 1)).astype(np.int64), par[order].astype(np.int64), P)
    # at rest: the same tracks without a step, so every pair lands in the central counters
    at_rest = (np.repeat(origin, 3, axis=1).reshape(-1, 2)[order],) + stubs[1:]
    # walks: 200 ids in every frame, every frame in an order of its own
    walks = 256. + np.cumsum(rng.normal(0., 0.7, (F, 200, 2)), axis=0)
    shuffle = np.argsort(rng.uniform(size=(F, 200)), axis=1)
    walks = (np.take_along_axis(walks, shuffle[..., None], axis=1).reshape(-1, 2), np.arange(F + 1, dtype=np.int64) * 200,
             shuffle.reshape(-1).astype(np.int64), 200)

    def measure(table, reach):
        pos, off, par, P = table
        t_pos, t_off, t_par = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pos, off, par))
        call = lambda: ct.vanhove_arrays(t_pos, t_off, t_par, LAGS, WIDTH, reach, MPP, n_particles=P)
        with torch.cuda.stream(own):
            res = call()
            torch.cuda.synchronize()
            single = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(own)
                call()
                b.record(own)
                torch.cuda.synchronize()
                single.append(a.elapsed_time(b))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(own)
            for _ in range(50):
                call()
            b.record(own)
            torch.cuda.synchronize()
            queued = a.elapsed_time(b) / 50.
        half, edges, _, edge2 = vh.bins(WIDTH, reach)
        t0 = time.perf_counter()
        want = host_vanhove(pos, off, par, LAGS, edges, edge2, MPP)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = [getattr(res, name).cpu().numpy() for name in ('n', 'count', 'below', 'above', 'count_r', 'above_r')]
        same = all(np.array_equal(g, w) for g, w in zip(got, want)) and int(res.status) == _abi.VANHOVE_OK
        out = spread(single)
        out.update(per_call_of_50_queued_ms=queued, host_numpy_ms=host_ms, counts_equal_the_host=bool(same), half_bins=half,
                   pairs=[int(x) for x in want[0]], largest_cell=int(want[1].max()),
                   in_the_tails=int(want[2].sum() + want[3].sum()))
        return out, same

    out, ok = {}, True
    for name, table in (('stubs', stubs), ('stubs_at_rest', at_rest), ('walks', walks)):
        res = {}
        for reach in (1., 10.24):
            res['max_disp_%g' % reach], same = measure(table, reach)
            ok = ok and same
        out[name] = dict(workload=dict(frames=F, rows=int(len(table[2])), particles=int(table[3])), device=res)
        print(name, 'done', flush=True)
    out['method'] = dict(reps=args.reps, warmup_calls=1, lags=LAGS, bin_width=WIDTH, mpp=MPP,
                         clock="HIP events on a stream of its own around one call, torch's stable sort of the ids included; "
                               "median, minimum and maximum of reps; and 50 calls queued back to back, per call",
                         inputs='the table on the device, n_particles given, results left there',
                         host='wall clock, one core, one run, the same process: sort, pairs per lag by searchsorted, '
                              'histograms by searchsorted against the same edges and bincount')
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not ok:
        sys.exit('the device and the host rule disagree')


if __name__ == '__main__':
    main()
