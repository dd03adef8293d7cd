"""Time the two-point stage on the MI355X (ctr_twopoint_device) against the all-pairs walk
of g(r) on the same table and against the rule restated in NumPy on the host.

    python tools/twopoint_time.py [--reps 5] [--frames 1250] [--out profiles/twopoint_time.json]

Two tables.  ``cfg2``: what ``find_link_arrays`` returns for `--frames` cfg-2 frames (512 x 512 uint8, 200
Gaussians each, diameter 13, separation 13, search range 5) with ``minmass = 0``, so the noise maxima are
rows too: the table of ``tools/pair_correlation_time.py`` and ``tools/neighbors_time.py``, here with its
particle ids.  ``walks``: 200 random walkers (step 0.7 per axis and frame) in every one of `--frames` frames,
every frame in a row order of its own.  ``cutoff = 40``, ``dr = 0.5``, lags ``(1, 10, 100)``, ``max_disp = 20``;
the table on the device, ``n_particles`` given, the results left there.  HIP events on a stream of its own
around one call after a warm-up call, median / minimum / maximum of `reps`; alternating with it, in the
same process, ``pair_correlation_arrays(edge='none')`` at the same cutoff and bin width: the yardstick of an
all-pairs walk over the same frames (it walks every frame once, the two-point stage once per lag, and
only over the rows that have moved).  Next to them, wall clock on one core, one run: the rule restated in
NumPy (``tests/_twopoint.py``), whose integers the device's must equal (the c sum within ``n``).
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
CUTOFF, DR, LAGS, MAX_DISP = 40., 0.5, [1, 10, 100], 20.


def spread(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import _twopoint as yard
    import clustertracking_amd as ct
    from clustertracking_amd import _abi, _lib, workloads

    _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    own = torch.cuda.Stream(dev)

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(own)
        fn()
        b.record(own)
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def measure(name, t_pos, t_off, t_par, P):
        two = lambda: ct.twopoint_arrays(t_pos, t_off, t_par, LAGS, CUTOFF, DR, MAX_DISP, n_particles=P)
        gr = lambda: ct.pair_correlation_arrays(t_pos, t_off, CUTOFF, DR, edge='none')
        with torch.cuda.stream(own):
            res, g = two(), gr()                     # the warm-up calls
            torch.cuda.synchronize()
            ms_two, ms_gr = [], []
            for _ in range(args.reps):               # alternating
                ms_two.append(once(two))
                ms_gr.append(once(gr))
        pos, off, par = t_pos.cpu().numpy(), t_off.cpu().numpy(), t_par.cpu().numpy()
        t0 = time.perf_counter()
        want = yard.twopoint(pos, off, par, LAGS, CUTOFF, DR, MAX_DISP)
        host_ms = (time.perf_counter() - t0) * 1e3
        n, sums = res.n.cpu().numpy(), yard.integers(res.sums.cpu().numpy())
        c_off = max(abs(sums[k][b][2] - want.sums[k][b][2]) for k in range(len(LAGS)) for b in range(n.shape[1]))
        same = bool(int(res.status) == _abi.TP_OK and (n == want.n).all() and (res.n_moved.cpu().numpy() == want.n_moved).all()
                    and (res.beyond.cpu().numpy() == want.beyond).all()
                    and all(sums[k][b][:2] == want.sums[k][b][:2] and abs(sums[k][b][2] - want.sums[k][b][2]) <= want.n[k, b]
                            for k in range(len(LAGS)) for b in range(n.shape[1])))
        rows = np.diff(off)
        out = dict(workload=dict(frames=int(len(off) - 1), rows=int(len(pos)), particles=int(P),
                                 distance_evaluations_of_g_r=int((rows ** 2).sum())),
                   twopoint=spread(ms_two), pair_correlation_edge_none=spread(ms_gr), host_numpy_ms=host_ms,
                   integers_equal_the_restatement=same, largest_c_sum_difference=int(c_off),
                   pairs=[int(x) for x in want.n.sum(1)], moved=[int(x) for x in want.n_moved], beyond=[int(x) for x in want.beyond],
                   dot_in_the_last_bin=[None if n[k, -1] == 0 else float(res.dot[k, -1]) for k in range(len(LAGS))])
        print(name, out, flush=True)
        return out, same

    frames = workloads.cfg2(n_frames=args.frames)[0]
    print('drawn', flush=True)
    d_frames = torch.from_numpy(frames).to(dev)
    r = ct.find_link_arrays(d_frames, search_range=SEARCH_RANGE, separation=SEPARATION, diameter=DIAMETER, minmass=0,
                            max_queries=1024, max_relocated=1024, _on_device=True)
    del d_frames
    P = int(r.n_tracks.item()) if hasattr(r.n_tracks, 'item') else int(r.n_tracks)
    print('linked', int(r.pos.shape[0]), 'rows', P, 'tracks', flush=True)
    res_a, ok_a = measure('cfg2', r.pos, r.frame_offset, r.particle, P)
    res_a['workload'].update(generator='workloads.cfg2(n_frames=%d), minmass 0' % args.frames, table='find_link_arrays',
                             diameter=DIAMETER, separation=SEPARATION, search_range=SEARCH_RANGE)

    F = args.frames
    rng = np.random.RandomState(7)
    walks = 256. + np.cumsum(rng.normal(0., 0.7, (F, 200, 2)), axis=0)
    shuffle = np.argsort(rng.uniform(size=(F, 200)), axis=1)
    t_pos = torch.from_numpy(np.take_along_axis(walks, shuffle[..., None], axis=1).reshape(-1, 2)).to(dev)
    t_off = torch.arange(F + 1, dtype=torch.int64, device=dev) * 200
    t_par = torch.from_numpy(shuffle.reshape(-1).astype(np.int64)).to(dev)
    res_b, ok_b = measure('walks', t_pos, t_off, t_par, 200)
    res_b['workload'].update(generator='200 random walkers from one point, step 0.7 per axis and frame, shuffled rows')

    out = dict(
        method=dict(reps=args.reps, warmup_calls=1, cutoff=CUTOFF, dr=DR, lags=LAGS, max_disp=MAX_DISP,
                    clock='HIP events on a stream of its own around one call; median, minimum and maximum of reps; the two '
                          'calls alternate in one process',
                    inputs='the table on the device, n_particles given, results left there',
                    host='wall clock, one core, one run, the same process: tests/_twopoint.py',
                    max_bins=_abi.TP_MAX_BINS, max_lags=_abi.TP_MAX_LAGS),
        cfg2=res_a, walks=res_b)
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not (ok_a and ok_b):
        sys.exit('the device and the rule restated in NumPy disagree')


if __name__ == '__main__':
    main()
