"""Time feature location (ctr_locate_maxima_device) on the MI355X.

    python tools/locate_time.py [--cfg2-frames 256] [--cfg3-stacks 16] [--reps 20] [--out FILE]

Frames are cfg 2 (512x512 uint8, separation 13) and cfg 3 stacks (64x128x128 uint8, separation
(9, 17, 17)) from workloads.py.  Device time: HIP events around `reps` calls after warm-up,
on preallocated buffers (no host copy inside the window).  Achieved bandwidth counts one read
of the frames per call, against 6.3 TB/s achievable HBM.  The host path (NumPy percentile +
scipy.ndimage.grey_dilation + drop_close, one core) is timed on a few frames for comparison.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/locate_time.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12


def host_locate(frame, separation, percentile=64):
    """The rule on the host: what a user of the reference runs per frame."""
    from scipy import ndimage
    from clustertracking_amd.find import drop_close, percentile_threshold
    from clustertracking_amd.utils import validate_tuple
    ndim = frame.ndim
    sep = validate_tuple(separation, ndim)
    margin = tuple(int(s / 2) for s in sep)
    thr = percentile_threshold(frame, percentile)
    box = [int(2 * s / np.sqrt(ndim)) for s in sep]
    peak = (frame == ndimage.grey_dilation(frame, box, mode='constant')) & (frame > thr)
    pos = np.argwhere(peak)
    val = frame[peak]
    inside = ~np.any((pos < margin) | (pos > np.array(frame.shape) - margin - 1), 1)
    return drop_close(pos[inside], sep, val[inside])


def time_device(frames, separation, reps, warmup=3):
    import torch
    from clustertracking_amd import _abi, _lib
    eng = _lib.default_engine(0)
    dev = torch.device('cuda', 0)
    t = torch.from_numpy(frames).to(dev)
    n_frames, ndim = frames.shape[0], frames.ndim - 1
    cap = 1024 * n_frames
    off = torch.empty(n_frames + 1, dtype=torch.int64, device=dev)
    tot = torch.empty(1, dtype=torch.int64, device=dev)
    pos = torch.empty((cap, ndim), dtype=torch.int32, device=dev)
    loc = _abi.Locate()
    loc.ndim, loc.frame_dtype, loc.n_frames = ndim, _abi.DTYPE_CODES[frames.dtype], n_frames
    sep = separation if hasattr(separation, '__len__') else (separation,) * ndim
    for a in range(ndim):
        loc.shape[a] = frames.shape[1 + a]
        loc.separation[a] = float(sep[a])
        loc.margin[a] = int(sep[a] / 2)
    loc.percentile, loc.precise, loc.capacity = 64., 1, cap
    loc.frames, loc.frame_offset, loc.pos_out, loc.total = t.data_ptr(), off.data_ptr(), pos.data_ptr(), tot.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(warmup):
        eng.locate_maxima_device(loc, stream)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        eng.locate_maxima_device(loc, stream)
    b.record()
    torch.cuda.synchronize(dev)
    sec = a.elapsed_time(b) / 1e3 / reps
    total = int(tot.item())
    return dict(n_frames=int(n_frames), frame_shape=list(frames.shape[1:]), dtype=frames.dtype.name,
                separation=list(sep), maxima=total, call_ms=sec * 1e3, frames_per_s=n_frames / sec,
                gb_per_s=frames.nbytes / sec / 1e9, hbm_share=frames.nbytes / sec / HBM_BYTES_PER_S,
                hbm_bound_us=frames.nbytes / HBM_BYTES_PER_S * 1e6)


def time_host(frames, separation, n=4):
    t0 = time.perf_counter()
    for i in range(n):
        host_locate(frames[i], separation)
    sec = (time.perf_counter() - t0) / n
    return dict(frames=n, frame_ms=sec * 1e3, frames_per_s=1. / sec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg2-frames', type=int, default=256)
    ap.add_argument('--cfg3-stacks', type=int, default=16)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-frames', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from clustertracking_amd import workloads
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    out = {}
    f2, _, _, o2 = workloads.cfg2(n_frames=args.cfg2_frames)
    out['cfg2'] = dict(device=time_device(f2, o2['diameter'], args.reps),
                       host_one_core=time_host(f2, o2['diameter'], args.host_frames))
    f3, _, _, o3 = workloads.cfg3(n_stacks=args.cfg3_stacks)
    out['cfg3'] = dict(device=time_device(f3, tuple(o3['diameter']), args.reps),
                       host_one_core=time_host(f3, tuple(o3['diameter']), min(args.host_frames, 2)))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
