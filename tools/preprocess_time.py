"""Time the preprocessing (ctr_preprocess_device) on the MI355X.

    python tools/preprocess_time.py [--cfg2-frames 256] [--cfg3-stacks 16] [--reps 20] [--out FILE]

cfg 2: 512x512 uint8 frames, noise_size 1, smoothing_size 13; cfg 3: 64x128x128 uint8 stacks,
noise_size 1, smoothing_size (9, 17, 17) (workloads.py; `--distinct` frames are generated and
repeated to fill the block: the kernels do the same work on every frame).  Device time: HIP
events on a stream of its own around `reps` calls after warm-up, on preallocated frames and
outputs (the call's own workspace is a stream-ordered allocation inside every call), for
both ways of finding the per-frame maximum before the rescaling (CTR_PRE_BAND_PLANE: a float64
band plane through HBM; CTR_PRE_TWICE: the stencil run twice).  `floor_share` is the time of
one read of the raw frames plus one write of the output at 6.3 TB/s achievable HBM, over the
time measured.  `locate_ratio` is locate(..., noise_size=1) over locate(...) in this run (wall
clock of the Python call, positions left on the device); `vs_locate_call` the preprocessing call
over the 0.95 ms of the cfg-2 locate call of the parent commit.  The host path
is the SciPy yardstick (tests/_preprocess.py) on one core.
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


def time_device(frames, noise, smooth, strategy, reps, warmup=3):
    import torch
    from clustertracking_amd import _abi, _lib, preprocessing
    eng = _lib.default_engine(0)
    dev = torch.device('cuda', 0)
    ndim = frames.ndim - 1
    lshort, taps = preprocessing._taps(noise, ndim)
    box = preprocessing._box(lshort, smooth, ndim)
    t = torch.from_numpy(frames).to(dev)
    out = torch.empty_like(t)
    scale = torch.empty(len(frames), dtype=torch.float64, device=dev)
    d = _abi.Preprocess()
    d.ndim, d.frame_dtype, d.n_frames = ndim, _abi.DTYPE_CODES[frames.dtype], len(frames)
    d.mode, d.strategy, d.threshold = _abi.PRE_PREPROCESS, strategy, 1.
    held = [torch.from_numpy(w).to(dev) for w in taps]
    for a in range(ndim):
        d.shape[a], d.box[a] = frames.shape[1 + a], box[a]
        d.n_taps[a], d.taps[a] = held[a].numel(), held[a].data_ptr()
    d.frames, d.out, d.scale_factor = t.data_ptr(), out.data_ptr(), scale.data_ptr()
    torch.cuda.synchronize(dev)
    own = torch.cuda.Stream(dev)
    for _ in range(warmup):
        eng.preprocess_device(d, own.cuda_stream)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(own)
    for _ in range(reps):
        eng.preprocess_device(d, own.cuda_stream)
    b.record(own)
    torch.cuda.synchronize(dev)
    sec = a.elapsed_time(b) / 1e3 / reps
    floor = (frames.nbytes + out.numel() * out.element_size()) / HBM_BYTES_PER_S
    return dict(call_ms=sec * 1e3, pixels_per_s=frames.size / sec, floor_us=floor * 1e6, floor_share=floor / sec,
                checksum=int(out.sum(dtype=torch.int64).item()), scale0=float(scale[0].item()))


def time_locate(frames, sep, reps=5):
    import torch
    from clustertracking_amd import find
    t = torch.from_numpy(frames).cuda()
    res = {}
    for label, noise in (('raw', None), ('preprocessed', 1)):
        find.locate_arrays(t, sep, _on_device=True, noise_size=noise)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            find.locate_arrays(t, sep, _on_device=True, noise_size=noise)
        torch.cuda.synchronize()
        res[label + '_ms'] = (time.perf_counter() - t0) / reps * 1e3
    res['locate_ratio'] = res['preprocessed_ms'] / res['raw_ms']
    return res


def time_host(frames, noise, smooth, n):
    import _preprocess
    t0 = time.perf_counter()
    for i in range(n):
        _preprocess.preprocess(frames[i], noise, smooth)
    return dict(frames=n, frame_ms=(time.perf_counter() - t0) / n * 1e3)


def block(make, n, distinct):
    frames = make(min(n, distinct))[0]
    return np.concatenate([frames] * (-(-n // len(frames))))[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg2-frames', type=int, default=256)
    ap.add_argument('--cfg3-stacks', type=int, default=16)
    ap.add_argument('--distinct', type=int, default=8)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-frames', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from clustertracking_amd import _abi, workloads
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    out = {}
    for name, frames, noise, smooth in (
            ('cfg2', block(lambda n: workloads.cfg2(n_frames=n), args.cfg2_frames, args.distinct), 1, 13),
            ('cfg3', block(lambda n: workloads.cfg3(n_stacks=n), args.cfg3_stacks, min(args.distinct, 2)), 1, (9, 17, 17))):
        res = dict(n_frames=len(frames), frame_shape=list(frames.shape[1:]), dtype=frames.dtype.name,
                   noise_size=noise, smoothing_size=smooth,
                   band_plane=time_device(frames, noise, smooth, _abi.PRE_BAND_PLANE, args.reps),
                   twice=time_device(frames, noise, smooth, _abi.PRE_TWICE, args.reps),
                   locate=time_locate(frames, smooth),
                   host_one_core=time_host(frames, noise, smooth, min(args.host_frames, len(frames))))
        assert res['band_plane']['checksum'] == res['twice']['checksum']
        out[name] = res
    out['cfg2']['twice']['vs_locate_call'] = out['cfg2']['twice']['call_ms'] / LOCATE_CFG2_CALL_MS
    out['cfg2']['band_plane']['vs_locate_call'] = out['cfg2']['band_plane']['call_ms'] / LOCATE_CFG2_CALL_MS
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
