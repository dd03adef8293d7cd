"""Time the model and residual frames of a fitted table on the MI355X (ctr_residual_device; DESIGN.md
7b) beside the fit they follow and the NumPy restatement.

    python tools/residual_time.py [--frames 256] [--reps 5] [--out profiles/residual_time.json]

Input: the cfg-2 batch (workloads.cfg2: 256 frames of 512 x 512 uint8 and 51 200 rows, diameter 13) with
the parameters, clusters and offsets that refine_arrays returns for it, as tensors on the device.  Device
time: every call of the public functions between two HIP events on a stream of the tool's, after a
warm-up; median, minimum and maximum of `reps` calls.  In the same process and alternating, call by
call: residual_arrays with the frames written (residual, coverage, owner), with the model too, statistics
only (want_frames=False), and refine_arrays on the same batch as the yardstick.  Bytes moved: the frames
read and the outputs written, over the median time, next to the 6.29 TB/s a float4 copy reaches on this
GPU.  Host time: wall clock of tests/_residual.py (NumPy, one core) on the first frame, and the
agreement of the device with it there.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/residual_time.py`.
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

HBM_COPY_TBS = 6.29


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
    import _residual as R
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
    fit = lambda: ct.refine_arrays(frames_d, pos_d, off_d, diameter, signal=float(f0['signal'].iloc[0]),
                                   size=float(f0['size'].iloc[0]), background=float(f0['background'].iloc[0]))
    res = fit()
    params_d, cluster_d = res.params, res.cluster
    calls = dict(
        residual_frames=lambda: ct.residual_arrays(frames_d, params_d, off_d, diameter, cluster=cluster_d),
        residual_frames_and_model=lambda: ct.residual_arrays(frames_d, params_d, off_d, diameter, cluster=cluster_d, want_model=True),
        residual_statistics_only=lambda: ct.residual_arrays(frames_d, params_d, off_d, diameter, cluster=cluster_d, want_frames=False),
        refine_arrays=fit)
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
        got = calls['residual_frames_and_model']()
        torch.cuda.synchronize(dev)

    pixels = int(np.prod(frames.shape))
    rows_out = n * (3 * 8 + 5 * 8 + 3 * 8)
    moved = dict(residual_frames=pixels * (1 + 8 + 4 + 4) + rows_out,
                 residual_frames_and_model=pixels * (1 + 8 + 4 + 4 + 8) + rows_out,
                 residual_statistics_only=pixels * (1 + 8 + 4) + rows_out)      # residual and owner go to scratch
    device = {name: stats(v) for name, v in ms.items()}
    for name, b in moved.items():
        device[name]['bytes_moved'] = int(b)
        device[name]['tb_per_s'] = b / (device[name]['median_ms'] * 1e-3) / 1e12
        device[name]['of_float4_copy'] = device[name]['tb_per_s'] / HBM_COPY_TBS
        device[name]['of_refine_arrays'] = device[name]['median_ms'] / device['refine_arrays']['median_ms']

    params, cluster = params_d.cpu().numpy(), cluster_d.cpu().numpy()
    k = int(offs[1])
    t0 = time.perf_counter()
    want = R.residual_np(frames[:1], params[:k], offs[:2], diameter, 'gauss', cluster=cluster[:k])
    host_ms = (time.perf_counter() - t0) * 1e3
    r, w = got.residual[0].cpu().numpy(), want.residual[0]
    cost = got.cost[:k].cpu().numpy()
    fit_cost = res.cost[:k].cpu().numpy()
    both = ~np.isnan(fit_cost)
    scaled = want.scale[0] > 0                      # (a pixel of value 0 outside every mask has no scale, and no difference)
    plan = _lib.residual_plan(importlib.import_module('clustertracking_amd.residual').descriptor(frames.shape[1:], frames.dtype, T, n, diameter, has_cluster=True))
    out = dict(
        frames=T, shape=list(frames.shape[1:]), rows=n, diameter=diameter, pixel_type=str(frames.dtype),
        device=device,
        plan=dict(tile=list(plan.tile), chunk=plan.chunk, n_tiles=plan.n_tiles, grids=list(plan.grids), lds_bytes=plan.lds_bytes,
                  scratch_bytes_with_frames=plan.scratch_bytes),
        host_restatement=dict(frames=1, rows=k, ms=host_ms),
        agreement=dict(coverage_equal=bool((got.coverage[0].cpu().numpy() == want.coverage[0]).all()),
                       owner_equal=bool((got.owner[0].cpu().numpy() == want.owner[0]).all()),
                       n_pix_equal=bool((got.n_pix[:k].cpu().numpy() == want.n_pix).all()),
                       residual_max_in_eps_scale=float((np.abs(r - w)[scaled] / (R.EPS * want.scale[0][scaled])).max()),
                       cost_max_rel_to_restatement=float((np.abs(cost - want.cost) / want.cost).max()),
                       cost_median_rel_to_refine=float(np.median(np.abs(cost - fit_cost)[both] / fit_cost[both]))))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
