"""Time the orientation and the diffusion tensor of tracked clusters on the MI355X
(ctr_orientation_device, ctr_diffusion_device) against the NumPy restatement.

    python tools/motion_time.py [--reps 5] [--out profiles/motion_time.json]

Input (random rigid tetramers, no oracle, no reference): 200 tracks x 1250 frames in 3D, the shape of
the cfg-4 shard, lags 1 .. 100.  Device time: HIP events around `reps` calls after warm-up, inputs
on the device, outputs preallocated; the orientation call, the diffusion call with the whole sweep,
and the diffusion call with lag 1 alone.  Host time: wall clock of tests/_motion.py (vectorised
NumPy, one core) on the same arrays, orientation and ONE lag.
Bytes of the diffusion call, computed from the shapes: what the partial kernel stages (every tile
with its halo, bases and positions), the partials it writes and the final kernel reads back, the
lags and the outputs; `hbm_fraction` is those bytes over the call time over HBM_PEAK.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/motion_time.py`.
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

HBM_PEAK = 8.0e12      # bytes/s, the MI355X's specified peak
TRACKS, FRAMES, LAGS = 200, 1250, 100


def tetramers(seed, n_tracks, n_frames):
    """pos [T, F, 4, 3] (z, y, x) of rigid tetramers that diffuse and rotate; 2 % of the frames missing"""
    rng = np.random.RandomState(seed)
    shape = np.array([[3., 3., 3.], [3., -3., -3.], [-3., 3., -3.], [-3., -3., 3.]])
    w = rng.normal(0., 0.05, (n_tracks, n_frames, 3))
    K = np.zeros((n_tracks, n_frames, 3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -w[..., 2], w[..., 1], -w[..., 0]
    K = K - K.transpose(0, 1, 3, 2)
    step = np.eye(3) + K + 0.5 * K @ K                      # a small rotation, orthonormal to second order
    R = np.empty_like(step)
    cur = np.broadcast_to(np.eye(3), (n_tracks, 3, 3))
    for f in range(n_frames):
        cur = step[:, f] @ cur
        u, _, vt = np.linalg.svd(cur)                       # keep it a rotation
        cur = u @ vt
        R[:, f] = cur
    centre = 100. + rng.normal(0., 0.3, (n_tracks, n_frames, 1, 3)).cumsum(1)
    pos = np.einsum('kj,tfij->tfki', shape, R) + centre + rng.normal(0., 0.02, (n_tracks, n_frames, 4, 3))
    pos[rng.rand(n_tracks, n_frames) < 0.02] = np.nan
    return pos


def diffusion_bytes(n_tracks, n_perm, n_frames, n_lags, ndim):
    import _motion as M
    staged = M.MOT_TILE + M.mot_halo(n_frames)
    n_tiles = -(-n_frames // M.MOT_TILE)
    frames_staged = sum(min(staged, n_frames - b0) for b0 in range(0, n_frames, M.MOT_TILE))
    read_tiles = n_tracks * n_perm * frames_staged * M.MOT_ROW * 8
    partials = n_tracks * n_lags * n_perm * n_tiles * M.MOT_NSUM * 8
    D = 3 if ndim == 2 else 6
    outputs = n_tracks * n_lags * (D * D + 1) * 8
    return dict(staged_read=read_tiles, partials_written_and_read=2 * partials, outputs=outputs,
                total=read_tiles + 2 * partials + outputs + n_lags * 8,
                inputs_once=n_tracks * n_frames * (n_perm * 9 + 3) * 8)


def timed(fn, stream, reps, warmup=2):
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--tracks', type=int, default=TRACKS)
    ap.add_argument('--frames', type=int, default=FRAMES)
    ap.add_argument('--lags', type=int, default=LAGS)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import _motion as M
    from clustertracking_amd import _abi, _lib
    T, F, P = args.tracks, args.frames, 12
    sizes = np.array([1.0, 1.2, 0.9, 1.1])
    pos = tetramers(4, T, F)
    lags = np.arange(1, args.lags + 1, dtype=np.int64)

    t0 = time.perf_counter()
    want_com, want_bases = M.orientation(pos, 4, 3, 0.3, sizes)
    host_ori_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    want, want_n = M.diffusion_tensor(want_com, want_bases, lags[:1], 30., 3)
    host_dif_s = time.perf_counter() - t0

    eng = _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    pos_d = torch.from_numpy(pos).to(dev)
    lag_d = torch.from_numpy(lags).to(dev)
    com = torch.empty((T, F, 3), dtype=torch.float64, device=dev)
    bases = torch.empty((T, P, F, 3, 3), dtype=torch.float64, device=dev)
    tensor = torch.empty((T, len(lags), 6, 6), dtype=torch.float64, device=dev)
    counts = torch.empty((T, len(lags)), dtype=torch.int64, device=dev)
    o = _abi.Orientation()
    o.ndim, o.cluster_size, o.n_tracks, o.n_frames, o.mpp = 3, 4, T, F, 0.3
    for k in range(4):
        o.weights[k] = float(sizes[k] ** 3)
    o.pos, o.com, o.bases = pos_d.data_ptr(), com.data_ptr(), bases.data_ptr()
    d = _abi.Diffusion()
    d.ndim, d.n_perm, d.n_tracks, d.n_frames, d.n_lags, d.fps = 3, P, T, F, len(lags), 30.
    d.lags, d.positions, d.bases = lag_d.data_ptr(), com.data_ptr(), bases.data_ptr()
    d.tensor, d.n_samples = tensor.data_ptr(), counts.data_ptr()
    torch.cuda.synchronize(dev)
    own = torch.cuda.Stream(dev)     # see tools/characterize_time.py
    ori_ms = timed(lambda: eng.orientation_device(o, own.cuda_stream), own, args.reps)
    sweep_ms = timed(lambda: eng.diffusion_device(d, own.cuda_stream), own, args.reps)
    got, got_n = tensor.cpu().numpy(), counts.cpu().numpy()
    got_com, got_bases = com.cpu().numpy(), bases.cpu().numpy()
    d.n_lags = 1
    one_ms = timed(lambda: eng.diffusion_device(d, own.cuda_stream), own, args.reps)

    ok = np.isfinite(want_bases)
    top = np.abs(want[:, 0]).max((1, 2))
    by = diffusion_bytes(T, P, F, len(lags), 3)
    by1 = diffusion_bytes(T, P, F, 1, 3)
    out = dict(
        tracks=T, frames=F, n_perm=P, lags=int(len(lags)),
        device=dict(orientation_ms=ori_ms, diffusion_sweep_ms=sweep_ms, diffusion_ms_per_lag=sweep_ms / len(lags),
                    diffusion_one_lag_ms=one_ms),
        host_restatement=dict(orientation_ms=host_ori_s * 1e3, diffusion_one_lag_ms=host_dif_s * 1e3),
        speedup=dict(orientation=host_ori_s * 1e3 / ori_ms, diffusion_per_lag=host_dif_s * 1e3 / (sweep_ms / len(lags))),
        agreement=dict(bases_max_abs=float(np.abs(got_bases[ok] - want_bases[ok]).max()),
                       nan_pattern_equal=bool((np.isnan(got_bases) == np.isnan(want_bases)).all()
                                              and (np.isnan(got_com) == np.isnan(want_com)).all()),
                       tensor_lag1_max_rel=float((np.abs(got[:, 0] - want[:, 0]).max((1, 2)) / top).max()),
                       counts_equal=bool((got_n[:, 0] == want_n[:, 0]).all())),
        diffusion_bytes=dict(sweep=by, one_lag=by1, halo=M.mot_halo(F), lds_bytes=M.mot_lds_bytes(M.mot_halo(F)),
                             hbm_peak=HBM_PEAK,
                             hbm_fraction_sweep=by['total'] / (sweep_ms * 1e-3) / HBM_PEAK,
                             hbm_fraction_one_lag=by1['total'] / (one_ms * 1e-3) / HBM_PEAK,
                             # what a sweep without reuse would stage: every lag its own pass over the tiles
                             staged_read_without_reuse=by1['staged_read'] * int(len(lags))))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
