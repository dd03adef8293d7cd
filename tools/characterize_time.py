"""Time feature characterisation (ctr_characterize_device) on the MI355X.

    python tools/characterize_time.py [--cfg2-frames 256] [--cfg3-stacks 16] [--reps 20] [--out FILE]

Frames are cfg 2 (512x512 uint8, diameter 13: radius 6) and cfg 3 stacks (64x128x128 uint8,
diameter (9, 17, 17): radius (4, 8, 8), sizes per axis) from workloads.py; the features are the
maxima `locate` finds in them (positions int32, left on the device).  Device time: HIP events
around `reps` calls after warm-up, on preallocated buffers (no host copy inside the window).
Achieved bandwidth counts one read of the frames per call, against 6.3 TB/s achievable HBM; the
share of locate's time is against the cfg-2 call of tools/locate_time.py.  The
host path (the NumPy composition of the rule, tests/_characterize.py, one core) is timed on a
few frames for comparison.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/characterize_time.py`.
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

HBM_BYTES_PER_S = 6.3e12
LOCATE_CFG2_CALL_MS = 0.95   # DESIGN.md 7b, profiles/r05_locate_time.json


def time_device(frames, diameter, reps, warmup=3):
    import torch
    from clustertracking_amd import _abi, _lib, find
    eng = _lib.default_engine(0)
    dev = torch.device('cuda', 0)
    n_frames, ndim = frames.shape[0], frames.ndim - 1
    diameter = diameter if hasattr(diameter, '__len__') else (diameter,) * ndim
    radius = tuple(int(d // 2) for d in diameter)
    isotropic = len(set(diameter)) == 1
    t, pix, pos, off, _ = find.locate_arrays(frames, diameter, margin=radius, _on_device=True)
    n = int(pos.shape[0])
    mass = torch.empty(n, dtype=torch.float64, device=dev)
    signal = torch.empty(n, dtype=torch.float64, device=dev)
    size = torch.empty((n, 1 if isotropic else ndim), dtype=torch.float64, device=dev)
    ch = _abi.Characterize()
    ch.ndim, ch.frame_dtype, ch.n_frames = ndim, _abi.DTYPE_CODES[np.dtype(pix)], n_frames
    for a in range(ndim):
        ch.shape[a] = frames.shape[1 + a]
        ch.radius[a] = radius[a]
    ch.isotropic, ch.scale_factor, ch.n_features = int(isotropic), 1., n
    ch.frames, ch.frame_offset, ch.pos_i32 = t.data_ptr(), off.data_ptr(), pos.data_ptr()
    ch.mass, ch.signal, ch.size = mass.data_ptr(), signal.data_ptr(), size.data_ptr()
    # a stream of its own: on the legacy default stream the engine would launch on the handle's
    # stream (stream 0 means that in the C-ABI) and the events would not bracket the kernels
    torch.cuda.synchronize(dev)
    own = torch.cuda.Stream(dev)
    stream = own.cuda_stream
    for _ in range(warmup):
        eng.characterize_device(ch, stream)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(own)
    for _ in range(reps):
        eng.characterize_device(ch, stream)
    b.record(own)
    torch.cuda.synchronize(dev)
    sec = a.elapsed_time(b) / 1e3 / reps
    window = int(np.prod([2 * r + 1 for r in radius]))
    return dict(n_frames=int(n_frames), frame_shape=list(frames.shape[1:]), dtype=frames.dtype.name,
                radius=list(radius), isotropic=isotropic, features=n, window_pixels=window,
                call_ms=sec * 1e3, features_per_s=n / sec, window_pixels_per_s=n * window / sec,
                gb_per_s=frames.nbytes / sec / 1e9, hbm_share=frames.nbytes / sec / HBM_BYTES_PER_S,
                hbm_bound_us=frames.nbytes / HBM_BYTES_PER_S * 1e6,
                mass_checksum=float(mass.sum().item()))


def time_host(frames, diameter, n=4):
    import _characterize
    import _locate
    ndim = frames.ndim - 1
    diameter = diameter if hasattr(diameter, '__len__') else (diameter,) * ndim
    radius = tuple(int(d // 2) for d in diameter)
    pos = [_locate.compose(frames[i], diameter, margin=radius) for i in range(n)]
    t0 = time.perf_counter()
    for i in range(n):
        _characterize.compose(pos[i], frames[i], radius, len(set(diameter)) == 1)
    sec = (time.perf_counter() - t0) / n
    n_feat = sum(len(p) for p in pos)
    return dict(frames=n, features=n_feat, frame_ms=sec * 1e3, features_per_s=n_feat / n / sec)


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
    out['cfg2']['device']['share_of_locate_call'] = out['cfg2']['device']['call_ms'] / LOCATE_CFG2_CALL_MS
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
