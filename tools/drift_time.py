"""Time the drift stage on the MI355X (ctr_drift_device, ctr_drift_subtract_device,
ctr_filter_stubs_device) against the same rule on the host.

    python tools/drift_time.py [--reps 5] [--frames 1250] [--train 100] [--out profiles/drift_time.json]

Table: what ``find_link_arrays`` returns for `--frames` cfg-2 frames (512 x 512 uint8, 200 Gaussians
each, diameter 13, separation 13, search range 5) with ``minmass = 0``, so the noise maxima are rows
of the table too.  cfg 2 draws every frame from a seed of its own: the links are accidental and
nearly every track is a stub, which is the table that the stub filter is for.  Where the linker
refuses that table (a level beyond its limits), locate + ``link_arrays`` of the same frames gives it
instead; the file says which.
Timed, the table on the device and the results left there, HIP events on a stream of its own around
one call after a warm-up call, median / minimum / maximum of `reps`: ``compute_drift_arrays``
(smoothing 0 and 10), ``subtract_drift_arrays`` and ``filter_stubs_arrays`` with ``n_particles`` given
(no host copy inside); and, since such a window is tens of microseconds, `--train` calls queued back
to back between one pair of events, per call.  Next to each, wall clock on one core in the same process: the rule as plain
loops (the text of tests/_drift.py, copied) and in vectorised pandas / NumPy; the device's result is
compared with the loops': n_pairs, counts and ids exactly, the drift within 2^-50 n_max (t + 1) D.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIAMETER, SEPARATION, SEARCH_RANGE = 13, 13, 5
THRESHOLD = 5


# ---- the rule on the host: plain loops (tests/_drift.py) ----
def _mean(values, ndim):
    if not values:
        return None
    return np.array([math.fsum(v[d] for v in values) / len(values) for d in range(ndim)])


def loops_compute_drift(pos, off, particle, smoothing=0):
    T, ndim = len(off) - 1, pos.shape[1]
    n_pairs = np.zeros(T, dtype=np.int32)
    dx = np.zeros((T, ndim))
    largest = 0.
    for t in range(1, T):
        lowest = {}
        for j in range(off[t - 1], off[t]):
            if particle[j] >= 0:
                lowest.setdefault(int(particle[j]), j)
        steps = []
        for i in range(off[t], off[t + 1]):
            j = lowest.get(int(particle[i])) if particle[i] >= 0 else None
            if j is not None:
                steps.append(pos[i] - pos[j])
        n_pairs[t] = len(steps)
        if steps:
            dx[t] = _mean(steps, ndim)
            largest = max(largest, float(np.abs(steps).max()))
    sm = np.zeros((T, ndim))
    for t in range(1, T):
        window = [t] if smoothing <= 1 else range(max(1, t - smoothing + 1), t + 1)
        m = _mean([dx[u] for u in window if n_pairs[u] > 0], ndim)
        if m is not None:
            sm[t] = m
    drift = np.zeros((T, ndim))
    for t in range(1, T):
        drift[t] = drift[t - 1] + sm[t]
    return drift, n_pairs, largest


def loops_filter_stubs(particle, threshold, P):
    count = np.zeros(P, dtype=np.int32)
    for p in particle:
        if p >= 0:
            count[p] += 1
    return np.array([p if p >= 0 and count[p] >= threshold else -1 for p in particle], dtype=np.int64), count


# ---- ... and vectorised ----
def vectorised_compute_drift(pos, off, particle, smoothing=0):
    import pandas as pd
    T, ndim = len(off) - 1, pos.shape[1]
    axes = ['x%d' % d for d in range(ndim)]
    f = pd.DataFrame(pos, columns=axes)
    f['frame'] = np.repeat(np.arange(T), np.diff(off))
    f['particle'] = particle
    f = f[f['particle'] >= 0]
    before = f.drop_duplicates(['frame', 'particle'], keep='first').copy()     # the lowest row of an id
    before['frame'] += 1
    pairs = f.merge(before, on=['frame', 'particle'], suffixes=('', 'b'))
    step = pd.DataFrame({a: pairs[a] - pairs[a + 'b'] for a in axes})
    by = step.groupby(pairs['frame'].values)
    n_pairs = by.size().reindex(np.arange(T), fill_value=0).values.astype(np.int32)
    dx = by.mean().reindex(np.arange(T))
    sm = (dx if smoothing <= 1 else dx[1:].rolling(smoothing, min_periods=1).mean().reindex(np.arange(T))).fillna(0.)
    return np.cumsum(sm.values, axis=0), n_pairs


def vectorised_subtract(pos, off, drift):
    return pos - drift[np.repeat(np.arange(len(off) - 1), np.diff(off))]


def vectorised_filter_stubs(particle, threshold, P):
    count = np.bincount(particle[particle >= 0], minlength=P).astype(np.int32)
    return np.where((particle >= 0) & (count[np.maximum(particle, 0)] >= threshold), particle, -1), count


def spread(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)))


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--train', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import clustertracking_amd as ct
    from clustertracking_amd import _lib, workloads
    from clustertracking_amd.find import locate_arrays
    from clustertracking_amd.link import SubnetOversizeException

    _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    F = args.frames
    frames = workloads.cfg2(n_frames=F)[0]
    print('drawn', flush=True)
    d_frames = torch.from_numpy(frames).to(dev)
    try:
        r = ct.find_link_arrays(d_frames, search_range=SEARCH_RANGE, separation=SEPARATION, diameter=DIAMETER, minmass=0,
                                max_queries=1024, max_relocated=1024, _on_device=True)
        t_pos, t_off, t_par, P, source = r.pos, r.frame_offset, r.particle, int(r.n_tracks.item()), 'find_link_arrays'
    except (_lib.EngineError, SubnetOversizeException) as e:
        print('find_link_arrays refused the table (%s): locate + link_arrays instead' % e, flush=True)
        _, _, pos_i, t_off, _ = locate_arrays(d_frames, SEPARATION, 64, (DIAMETER // 2,) * 2, _on_device=True)
        t_pos = pos_i.to(torch.float64)
        t_par = ct.link_arrays(t_pos, t_off, SEARCH_RANGE, 0, _on_device=True)
        P, source = int(t_par.max().item()) + 1, 'locate_arrays + link_arrays (find_link_arrays refused: %s)' % e
    del d_frames
    pos, off, par = (x.cpu().numpy() for x in (t_pos, t_off, t_par))
    print('linked', len(par), 'rows', P, 'particles', flush=True)
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
            # a window of tens of microseconds measures the clock as much as the call: also
            # `--train` calls queued back to back between one pair of events, per call
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(own)
            for _ in range(args.train):
                fn()
            b.record(own)
            torch.cuda.synchronize()
        return out, dict(spread(ms), back_to_back_ms_per_call=a.elapsed_time(b) / args.train)

    device, host, ok = {}, {}, True
    for s in (0, 10):
        got, device['compute_drift_arrays_smoothing_%d' % s] = timed(
            lambda: ct.compute_drift_arrays(t_pos, t_off, t_par, smoothing=s, n_particles=P))
        (want, want_n, D), loops_ms = wall(lambda: loops_compute_drift(pos, off, par, s))
        (vec, vec_n), vec_ms = wall(lambda: vectorised_compute_drift(pos, off, par, s))
        drift, n_pairs = got.drift.cpu().numpy(), got.n_pairs.cpu().numpy()
        bound = 2. ** -50 * int(want_n.max()) * (np.arange(len(want_n)) + 1.)[:, None] * D
        same = bool(int(got.status) == 0 and np.array_equal(n_pairs, want_n) and (np.abs(drift - want) <= bound).all())
        ok = ok and same
        host['compute_drift_smoothing_%d' % s] = dict(
            loops_ms=loops_ms, vectorised_ms=vec_ms, device_within_bound_of_loops=same,
            max_abs_device_minus_loops=float(np.abs(drift - want).max()), bound_at_last_frame=float(bound[-1, 0]),
            max_abs_vectorised_minus_loops=float(np.abs(vec - want).max()), vectorised_n_pairs_equal=bool(np.array_equal(vec_n, want_n)))
    shifted, device['subtract_drift_arrays'] = timed(lambda: ct.subtract_drift_arrays(t_pos, t_off, got.drift))
    want_shift, vec_ms = wall(lambda: vectorised_subtract(pos, off, drift))
    same = shifted.cpu().numpy().tobytes() == want_shift.tobytes()
    ok = ok and same
    host['subtract_drift'] = dict(vectorised_ms=vec_ms, device_equals_bytes=bool(same))
    stubs, device['filter_stubs_arrays'] = timed(lambda: ct.filter_stubs_arrays(t_par, THRESHOLD, n_particles=P))
    (want_par, want_count), loops_ms = wall(lambda: loops_filter_stubs(par, THRESHOLD, P))
    (vec_par, vec_count), vec_ms = wall(lambda: vectorised_filter_stubs(par, THRESHOLD, P))
    same = np.array_equal(stubs.particle.cpu().numpy(), want_par) and np.array_equal(stubs.count.cpu().numpy(), want_count)
    ok = ok and same
    host['filter_stubs'] = dict(loops_ms=loops_ms, vectorised_ms=vec_ms, device_equals_loops=bool(same),
                                vectorised_equals_loops=bool(np.array_equal(vec_par, want_par) and np.array_equal(vec_count, want_count)))
    n_pairs = got.n_pairs.cpu().numpy()
    out = dict(
        workload=dict(generator='workloads.cfg2(n_frames=%d), minmass 0' % F, table=source, frames=F, rows=int(len(par)),
                      rows_per_frame=len(par) / F, largest_frame=int(np.diff(off).max()), particles=P,
                      linked_rows=int((par >= 0).sum()), pairs=int(n_pairs.sum()), frames_without_pairs=int((n_pairs[1:] == 0).sum()),
                      stub_threshold=THRESHOLD, rows_kept=int((want_par >= 0).sum()), diameter=DIAMETER, separation=SEPARATION,
                      search_range=SEARCH_RANGE),
        method=dict(reps=args.reps, warmup_calls=1, back_to_back_calls=args.train,
                    clock='HIP events on a stream of its own around one call; median, minimum and maximum of reps',
                    inputs='the table on the device, n_particles given, results left there',
                    host='wall clock, one core, one run, the same process'),
        device=device, host=host)
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not ok:
        sys.exit('the device and the host rule disagree')


if __name__ == '__main__':
    main()
