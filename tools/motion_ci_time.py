"""Time the bootstrap interval of the diffusion tensor on the MI355X (ctr_diffusion_ci_device;
DESIGN.md 7b) against the NumPy restatement.

    python tools/motion_ci_time.py [--reps 3] [--samples 10000] [--out profiles/motion_ci_time.json]

Inputs are random positions and bases (the arithmetic does not care whether a basis is orthonormal),
2 % of the frames missing.  Cases: a 2D dimer over 1250 frames (3 x 3, two permutations: 2500 rows,
LDS-resident); a 3D tetramer over 1250 frames (6 x 6, twelve permutations: 15 000 rows, gathered
from global memory); a 3D tetramer over 110 frames (1320 rows, LDS-resident); pooled tracks of both
kinds.  Each as one (track, lag) and as a sweep of lags.  Device time: HIP events on a stream of
the script's around `reps` calls after warm-up, inputs on the device, outputs preallocated.
Host time: wall clock of tests/_motion_ci.py on the rows of ONE pair, with the closed form of the
acceleration in place of the jackknife that deletes rows, and `--host-samples` resamples (the time
is linear in them; the full count takes minutes for the tetramer).
Next to each device time: the gathers per second it implies (resamples x rows, an upper bound: the
rows that exist are 2 % fewer than n_max), the bytes per second those are (8 D per gather), and the
rate of the guide they are to be held against -- LDS: 150 TB/s of conflict-free ds_read_b64/b128
over the chip; L2: 17-19 TB/s of rows that every workgroup shares.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/motion_ci_time.py`.
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

LDS_PEAK, L2_RATE = 150e12, 18e12      # bytes/s, MI355X: LDS reads chip-wide; rows shared by all workgroups from L2

# name, ndim, n_perm, tracks, frames, lags of the sweep, pooled
CASES = [('dimer_2d', 2, 2, 1, 1250, 20, False),
         ('tetramer_3d_global', 3, 12, 1, 1250, 10, False),
         ('tetramer_3d_lds', 3, 12, 1, 110, 10, False),
         ('dimer_2d_pooled_8_tracks', 2, 2, 8, 150, 10, True),
         ('tetramer_3d_pooled_4_tracks', 3, 12, 4, 1250, 4, True)]


def tracks(seed, T, F, P):
    rng = np.random.RandomState(seed)
    positions = rng.normal(0., 1., (T, F, 3)).cumsum(1)
    bases = rng.normal(0., 1., (T, P, F, 3, 3))
    positions[rng.rand(T, F) < 0.02] = np.nan
    return positions, bases


def timed(fn, stream, reps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--samples', type=int, default=10000)
    ap.add_argument('--host-samples', type=int, default=500)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    from statistics import NormalDist
    import _motion_ci as C
    from clustertracking_amd import _abi, _lib
    eng = _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    own = torch.cuda.Stream(dev)
    B, results = args.samples, []
    for name, ndim, P, T, F, n_lags, pool in CASES:
        D = 3 if ndim == 2 else 6
        positions, bases = tracks(len(name), T, F, P)
        lags = np.arange(1, n_lags + 1, dtype=np.int64)
        pos_d, bases_d, lag_d = (torch.from_numpy(a).to(dev) for a in (positions, bases, lags))
        n_pairs = n_lags if pool else T * n_lags
        interval = torch.empty((n_pairs, 2, D, D), dtype=torch.float64, device=dev)
        ranks = torch.empty((n_pairs, 2, D, D), dtype=torch.int64, device=dev)
        tensor, z0, accel = (torch.empty((n_pairs, D, D), dtype=torch.float64, device=dev) for _ in range(3))
        counts = torch.empty((n_pairs,), dtype=torch.int64, device=dev)
        d = _abi.DiffusionCI()
        d.ndim, d.n_perm, d.n_tracks, d.n_frames, d.n_lags, d.fps = ndim, P, T, F, n_lags, 30.
        d.lags, d.positions, d.bases = lag_d.data_ptr(), pos_d.data_ptr(), bases_d.data_ptr()
        d.n_samples, d.seed, d.method, d.n_alpha, d.pool_tracks = B, 1, _abi.CI_BCA, 2, int(pool)
        for q, a in enumerate((0.025, 0.975)):
            d.alphas[q], d.z_alpha[q] = a, NormalDist().inv_cdf(a)
        d.interval, d.tensor, d.n_rows = interval.data_ptr(), tensor.data_ptr(), counts.data_ptr()
        d.z0, d.accel, d.ranks = z0.data_ptr(), accel.data_ptr(), ranks.data_ptr()
        in_lds, lds_bytes, scratch_bytes, chunk = _lib.diffusion_ci_plan(d)
        torch.cuda.synchronize(dev)
        sweep_ms = timed(lambda: eng.diffusion_ci_device(d, own.cuda_stream), own, args.reps)
        got = dict(interval=interval[0].cpu().numpy(), ranks=ranks[0].cpu().numpy(), counts=int(counts[0]))
        rows_sweep = int(counts.sum())
        d.n_lags = 1
        if not pool:
            d.n_tracks = 1
        one_ms = timed(lambda: eng.diffusion_ci_device(d, own.cuda_stream), own, args.reps)

        x = C.pooled_rows(positions, bases, 1, ndim) if pool else C.rows(positions[0], bases[0], 1, ndim)
        Bh = min(B, args.host_samples)
        t0 = time.perf_counter()
        C.ci(x, 1, 30., 0.05, Bh, 'bca', 1, accel=C.closed_form_accel)
        host_s = time.perf_counter() - t0
        agree = None
        if Bh == B:                                 # the whole interval on the host: hold the device against it
            want = C.ci(x, 1, 30., 0.05, B, 'bca', 1, accel=C.closed_form_accel)
            agree = dict(ranks_equal=bool((want['ranks'] == got['ranks']).all()),
                         interval_max_rel=float(np.abs(want['interval'] - got['interval']).max() / np.abs(want['interval']).max()))
        n = len(x)
        assert got['counts'] == n, (name, got['counts'], n)
        rate_one, rate_sweep = B * n / (one_ms * 1e-3), B * rows_sweep / (sweep_ms * 1e-3)
        results.append(dict(
            case=name, ndim=ndim, n_perm=P, tracks=T, frames=F, pooled=pool, n_samples=B, rows_of_the_pair=n,
            plan=dict(rows_in_lds=in_lds, lds_bytes=lds_bytes, scratch_bytes=scratch_bytes, pairs_per_chunk=chunk),
            device=dict(one_pair_ms=one_ms, sweep_ms=sweep_ms, sweep_pairs=n_pairs, sweep_ms_per_pair=sweep_ms / n_pairs,
                        gathers_per_s_one_pair=rate_one, gathers_per_s_sweep=rate_sweep,
                        gathered_bytes_per_s_sweep=rate_sweep * 8 * D,
                        compare_with=dict(what='LDS ds_read_b64/b128 chip-wide' if in_lds else "rows shared by all workgroups from the XCD's L2",
                                          bytes_per_s=LDS_PEAK if in_lds else L2_RATE),
                        fraction_of_that_rate_sweep=rate_sweep * 8 * D / (LDS_PEAK if in_lds else L2_RATE)),
            host_restatement=dict(n_samples=Bh, one_pair_ms=host_s * 1e3, ms_per_resample=host_s * 1e3 / Bh,
                                  one_pair_ms_at_n_samples=host_s * 1e3 / Bh * B, jackknife='closed form'),
            speedup_per_pair=host_s * 1e3 / Bh * B / (sweep_ms / n_pairs), agreement=agree))
    line = json.dumps(dict(n_samples=B, reps=args.reps, cases=results))
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
