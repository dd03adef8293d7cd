"""Time the standard errors of a fitted table on the MI355X (ctr_fit_error_device) beside
what the fit pays for its own Gaussian errors, and the NumPy restatement.

    python tools/fit_error_time.py [--frames 256] [--reps 5] [--out profiles/fit_error_time.json]

Input: the cfg-2 batch (workloads.cfg2: 256 frames of 512 x 512 uint8 and 51 200 rows, diameter 13) with
the parameters and clusters that refine_arrays returns for it, as tensors on the device, the number of
clusters given (no host read).  Device time: every call of the public functions between two HIP events on
a stream of the tool's, after a warm-up; median, minimum and maximum of `reps` calls.  In the same
process and alternating, call by call: fit_error_arrays with gauss, fit_error_arrays with ring (the same
table read as rings of thickness 0.45: not a fit, the same work per pixel), refine_arrays with
compute_error and refine_arrays without.  The yardstick is the difference of the last two: what the fit
pays for its own Gaussian errors.  Host time: wall clock of tests/_fit_error.py (NumPy, one core) on the
first frame, and the agreement of the device with it there.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/fit_error_time.py`.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=ms[0], max_ms=ms[-1], calls=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import _fit_error as rule
    import clustertracking_amd as ct
    from clustertracking_amd import _lib, workloads
    frames, f0, _, opts = workloads.cfg2(n_frames=args.frames)
    diameter = opts['diameter']
    T, n = len(frames), len(f0)
    offs = np.searchsorted(f0['frame'].values, np.arange(T + 1)).astype(np.int64)

    _lib.default_engine(0)            # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    frames_d = torch.from_numpy(frames).to(dev)
    pos_d = torch.from_numpy(np.ascontiguousarray(f0[['y', 'x']].values, dtype=np.float64)).to(dev)
    off_d = torch.from_numpy(offs).to(dev)
    fit = lambda **k: ct.refine_arrays(frames_d, pos_d, off_d, diameter, signal=float(f0['signal'].iloc[0]),
                                       size=float(f0['size'].iloc[0]), background=float(f0['background'].iloc[0]), **k)
    res = fit(compute_error=True)
    params_d, cluster_d = res.params, res.cluster
    n_clusters = int(res.status.shape[0])
    ring_d = torch.cat([params_d, torch.full((n, 1), 0.45, dtype=torch.float64, device=dev)], dim=1)
    calls = dict(
        fit_error_gauss=lambda: ct.fit_error_arrays(frames_d, params_d, off_d, cluster_d, diameter, n_clusters=n_clusters),
        fit_error_ring=lambda: ct.fit_error_arrays(frames_d, ring_d, off_d, cluster_d, diameter, 'ring', n_clusters=n_clusters),
        refine_with_errors=lambda: fit(compute_error=True),
        refine_without_errors=lambda: fit(compute_error=False))
    own = torch.cuda.Stream(dev)
    own.wait_stream(torch.cuda.current_stream(dev))
    ms = {name: [] for name in calls}
    with torch.cuda.stream(own):
        for _ in range(2):            # warm-up: the scratch of the handle, torch's allocator
            for fn in calls.values():
                fn()
        torch.cuda.synchronize(dev)
        for _ in range(args.reps):    # alternating, call by call
            for name, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(own)
                fn()
                b.record(own)
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
        got = calls['fit_error_gauss']()
        torch.cuda.synchronize(dev)

    device = {name: stats(v) for name, v in ms.items()}
    yardstick = device['refine_with_errors']['median_ms'] - device['refine_without_errors']['median_ms']
    params, cluster = params_d.cpu().numpy(), cluster_d.cpu().numpy()
    k = int(offs[1])
    t0 = time.perf_counter()
    want = rule.fit_error_np(frames[:1], params[:k], offs[:2], cluster[:k], diameter)
    host_ms = (time.perf_counter() - t0) * 1e3
    std, status = got.params_std[:k].cpu().numpy(), got.status[:k].cpu().numpy()
    ok = ~np.isnan(want.params_std)
    sizes = np.bincount(np.unique(cluster, return_counts=True)[1])
    plan = _lib.fit_error_plan(importlib.import_module('clustertracking_amd.fit_error').descriptor(
        frames.shape[1:], frames.dtype, T, n, n_clusters, diameter))
    out = dict(
        frames=T, shape=list(frames.shape[1:]), rows=n, clusters=n_clusters, diameter=diameter, pixel_type=str(frames.dtype),
        clusters_by_rows={str(s): int(c) for s, c in enumerate(sizes) if c},
        device=device, errors_of_the_fit_ms=yardstick,
        fit_error_gauss_of_errors_of_the_fit=device['fit_error_gauss']['median_ms'] / yardstick if yardstick > 0 else None,
        plan=dict(max_vars=list(plan.max_vars), chunk=list(plan.chunk), lds_bytes=list(plan.lds_bytes), grid=plan.grid,
                  scratch_bytes=plan.scratch_bytes),
        host_restatement=dict(frames=1, rows=k, ms=host_ms),
        agreement=dict(status_equal=bool((status == want.status).all()),
                       n_pix_equal=bool((got.n_pix[:k].cpu().numpy() == want.n_pix).all()),
                       std_max_rel_to_restatement=float((np.abs(std[ok] - want.params_std[ok]) / want.params_std[ok]).max())))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
