"""Time the MSD stage on the MI355X (ctr_msd_device, ctr_emsd_device) against the same
rule vectorised in NumPy on the host.

    python tools/msd_time.py [--reps 5] [--frames 1250] [--lags 100] [--threshold 100] [--out profiles/msd_time.json]

Two tables.  ``cfg2``: what ``find_link_arrays`` returns for `--frames` cfg-2 frames (512 x 512 uint8,
200 Gaussians each, diameter 13, separation 13, search range 5) with ``minmass = 0``, so the noise
maxima are rows too; cfg 2 draws every frame from a seed of its own, so the links are accidental and
nearly every track is a stub (where the linker refuses the table, locate + ``link_arrays`` of the same
frames gives it; the file says which).  ``walks``: 200 random walks present in every one of `--frames`
frames.  Timed on each, the table on the device and the results left there, HIP events on a stream
of its own around one call after a warm-up call, median / minimum / maximum of `reps`:
``emsd_arrays``, and ``msd_arrays`` for the ids that ``filter_stubs_arrays(threshold)`` keeps (and, on
cfg2, where few tracks are that long, also for a threshold of 5), ``n_particles`` given (no host copy
inside).  Each call includes torch's stable sort of the ids.  Next to each, wall clock on one core in
the same process, one run: the rule in vectorised NumPy (a ``searchsorted`` per lag on the rows
sorted by particle and frame).  The device's counts must equal the host's and its means lie within
(2 n + 4) X 2^-53 of them (n terms of size at most X summed in two different orders, tests/_msd.py).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIAMETER, SEPARATION, SEARCH_RANGE = 13, 13, 5
MPP, FPS = 0.16, 30.


class HostTable:
    """the rows that exist, sorted by (particle, frame): clause 1 and the sort, timed with the rule"""

    def __init__(self, pos, off, particle):
        T = len(off) - 1
        frame = np.repeat(np.arange(T), np.diff(off))
        keep = particle >= 0
        key = particle[keep] * T + frame[keep]
        key, first = np.unique(key, return_index=True)           # sorted; the lowest row of an id in a frame
        self.T, self.key, self.pos = T, key, pos[keep][first] * 1.
        self.particle, self.frame = key // T, key % T

    def lag(self, k):
        """(rows i, rows j) of the pairs at lag k"""
        at = np.searchsorted(self.key, self.key + k)
        ok = (self.frame + k < self.T) & (at < len(self.key))
        ok[ok] = self.key[at[ok]] == self.key[ok] + k
        return np.nonzero(ok)[0], at[ok]


def host_emsd(table, L, mpp):
    nd = table.pos.shape[1]
    n, mean_d, mean_d2, largest = np.zeros(L, dtype=np.int64), np.full((L, nd), np.nan), np.full((L, nd), np.nan), np.zeros((L, nd))
    for k in range(1, L + 1):
        i, j = table.lag(k)
        n[k - 1] = len(i)
        if len(i):
            d = (table.pos[j] - table.pos[i]) * mpp
            mean_d[k - 1], mean_d2[k - 1], largest[k - 1] = d.mean(0), (d * d).mean(0), np.abs(d).max(0)
    return n, mean_d, mean_d2, largest


def host_msd(table, L, mpp, ids, P):
    nd = table.pos.shape[1]
    n = np.zeros((len(ids), L), dtype=np.int64)
    mean_d, mean_d2 = np.full((len(ids), L, nd), np.nan), np.full((len(ids), L, nd), np.nan)
    largest = np.zeros((L, nd))
    for k in range(1, L + 1):
        i, j = table.lag(k)
        if not len(i):
            continue
        p = table.particle[i]
        d = (table.pos[j] - table.pos[i]) * mpp
        count = np.bincount(p, minlength=P)[ids]
        n[:, k - 1] = count
        with np.errstate(invalid='ignore', divide='ignore'):
            for a in range(nd):
                mean_d[:, k - 1, a] = np.bincount(p, weights=d[:, a], minlength=P)[ids] / count
                mean_d2[:, k - 1, a] = np.bincount(p, weights=d[:, a] * d[:, a], minlength=P)[ids] / count
        largest[k - 1] = np.abs(d).max(0)
    return n, mean_d, mean_d2, largest


def agree(got_n, got_d, got_d2, want):
    """counts equal, NaN in the same cells, means within (2 n + 4) X u; returns (ok, largest error / bound)"""
    n, mean_d, mean_d2, largest = want
    if not np.array_equal(got_n, n):
        return False, float('inf')
    worst = 0.
    for got, ref, X in ((got_d, mean_d, largest), (got_d2, mean_d2, largest ** 2)):
        if not np.array_equal(np.isnan(got), np.isnan(ref)):
            return False, float('inf')
        bound = (2. * n[..., None] + 4.) * X * 2. ** -53
        err = np.nan_to_num(np.abs(got - ref))
        if (err > bound).any():
            return False, float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.)
    return True, worst


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
    ap.add_argument('--lags', type=int, default=100)
    ap.add_argument('--threshold', type=int, default=100)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import clustertracking_amd as ct
    from clustertracking_amd import _abi, _lib, workloads
    from clustertracking_amd.find import locate_arrays
    from clustertracking_amd.link import SubnetOversizeException

    _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    F, L = args.frames, args.lags
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

    def measure(t_pos, t_off, t_par, P, thresholds):
        pos, off, par = (x.cpu().numpy() for x in (t_pos, t_off, t_par))
        res, ok = {}, True
        table, sort_ms = wall(lambda: HostTable(pos, off, par))
        ens, res['emsd_arrays'] = timed(lambda: ct.emsd_arrays(t_pos, t_off, t_par, L, MPP, FPS, n_particles=P))
        want, host_ms = wall(lambda: host_emsd(table, L, MPP))
        same, ratio = agree(ens.n.cpu().numpy(), ens.mean_d.cpu().numpy(), ens.mean_d2.cpu().numpy(), want)
        ok = ok and same and int(ens.status) == _abi.MSD_OK
        res['emsd_arrays'].update(host_sort_ms=sort_ms, host_vectorised_ms=host_ms, device_within_bound_of_host=same,
                                  largest_error_over_bound=ratio, pairs_at_lag_1=int(want[0][0]), pairs_at_last_lag=int(want[0][-1]))
        for th in thresholds:
            stubs = ct.filter_stubs_arrays(t_par, th, n_particles=P)
            ids = torch.nonzero(stubs.count >= th).flatten()
            per, t = timed(lambda: ct.msd_arrays(t_pos, t_off, t_par, L, MPP, FPS, particles=ids, n_particles=P))
            host_ids = ids.cpu().numpy()
            want, host_ms = wall(lambda: host_msd(table, L, MPP, host_ids, P))
            same, ratio = agree(per.n.cpu().numpy(), per.mean_d.cpu().numpy(), per.mean_d2.cpu().numpy(), want)
            ok = ok and same and int(per.status) == _abi.MSD_OK
            t.update(threshold=th, particles_reported=int(len(host_ids)), rows_of_them=int(stubs.count[ids].sum().item()),
                     host_vectorised_ms=host_ms, device_within_bound_of_host=same, largest_error_over_bound=ratio)
            res['msd_arrays_threshold_%d' % th] = t
        shape = dict(frames=int(len(off) - 1), rows=int(len(par)), particles=int(P), linked_rows=int((par >= 0).sum()),
                     longest_track_rows=int(np.bincount(par[par >= 0]).max()) if (par >= 0).any() else 0)
        return shape, res, ok

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
    print('linked', int(t_par.shape[0]), 'rows', P, 'particles', flush=True)
    shape_a, res_a, ok_a = measure(t_pos, t_off, t_par, P, sorted({5, args.threshold}))
    shape_a.update(generator='workloads.cfg2(n_frames=%d), minmass 0' % F, table=source, diameter=DIAMETER,
                   separation=SEPARATION, search_range=SEARCH_RANGE)
    print('cfg2 done', flush=True)

    rng = np.random.RandomState(7)
    walks = 256. + np.cumsum(rng.normal(0., 0.7, (F, 200, 2)), axis=0)
    order = np.argsort(rng.uniform(size=(F, 200)), axis=1)               # every frame in an order of its own
    w_pos = torch.from_numpy(np.take_along_axis(walks, order[..., None], axis=1).reshape(-1, 2)).to(dev)
    w_par = torch.from_numpy(order.reshape(-1).astype(np.int64)).to(dev)
    w_off = torch.arange(F + 1, dtype=torch.int64, device=dev) * 200
    shape_b, res_b, ok_b = measure(w_pos, w_off, w_par, 200, [args.threshold])
    shape_b.update(generator='200 Gaussian random walks (step 0.7 px per axis), every one in every frame, rows of a frame shuffled')

    out = dict(
        method=dict(reps=args.reps, warmup_calls=1, max_lagtime=L, mpp=MPP, fps=FPS,
                    clock='HIP events on a stream of its own around one call, torch\'s stable sort of the ids included; '
                          'median, minimum and maximum of reps',
                    inputs='the table on the device, n_particles given, results left there',
                    host='wall clock, one core, one run, the same process; host_sort_ms (the rows that exist, sorted) '
                         'is shared by the host calls of a table and not part of host_vectorised_ms',
                    tile=_abi.MSD_TILE, chunk=_abi.MSD_CHUNK),
        cfg2=dict(workload=shape_a, device=res_a), walks=dict(workload=shape_b, device=res_b))
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not (ok_a and ok_b):
        sys.exit('the device and the host rule disagree')


if __name__ == '__main__':
    main()
