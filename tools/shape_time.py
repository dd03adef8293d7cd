"""Time the shape coordinates of tracked clusters on the MI355X (ctr_shape_device,
ctr_shape_dynamics_device, ctr_shape_histogram_device) beside the diffusion tensor of the
same block and the NumPy restatement.

    python tools/shape_time.py [--reps 5] [--out profiles/shape_time.json]

Input: the block of tools/motion_time.py, 200 tetramer tracks x 1250 frames in 3D, as a tensor on the
device.  Device time: every call of the public functions between two HIP events on a stream of the
tool's, after a warm-up; median, minimum and maximum of `reps` calls.  In the same process and
alternating, call by call: shape_arrays, shape_dynamics_arrays over lags 1 .. 100,
shape_histogram_arrays at B = 200 and A = 180, and motion.diffusion_tensor over the same lags on the com
and bases of the same block (motion.orientation_arrays, computed once, outside the timing).  Host time:
wall clock of tests/_shape.py (NumPy, one core) on the first `--host-tracks` tracks, reported with that
number; the agreement of the device with it on those tracks is reported too.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/shape_time.py`.
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

TRACKS, FRAMES, LAGS = 200, 1250, 100
BOND_BINS, ANGLE_BINS, BOND_DR = 200, 180, 0.0625


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=ms[0], max_ms=ms[-1], calls=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--tracks', type=int, default=TRACKS)
    ap.add_argument('--frames', type=int, default=FRAMES)
    ap.add_argument('--lags', type=int, default=LAGS)
    ap.add_argument('--host-tracks', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import _shape as S
    from motion_time import tetramers
    from clustertracking_amd import _lib, motion, shape
    T, F = args.tracks, args.frames
    pos = tetramers(4, T, F)
    lags = np.arange(1, args.lags + 1, dtype=np.int64)
    mpp, fps = 0.3, 30.
    bond_max = BOND_BINS * BOND_DR

    _lib.default_engine(0)            # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    pos_d = torch.from_numpy(pos).to(dev)
    com_d, bases_d = motion.orientation_arrays(pos_d, 4, 3, mpp)
    calls = dict(
        shape_arrays=lambda: shape.shape_arrays(pos_d, 4, 3, mpp),
        shape_dynamics_arrays=lambda: shape.shape_dynamics_arrays(pos_d, 4, 3, lags, mpp, fps),
        shape_histogram_arrays=lambda: shape.shape_histogram_arrays(pos_d, 4, 3, bond_max, BOND_DR, ANGLE_BINS, mpp),
        diffusion_tensor=lambda: motion.diffusion_tensor(com_d, bases_d, lags, fps, 3))
    own = torch.cuda.Stream(dev)
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
        got_q = calls['shape_arrays']().coords
        got_dyn = calls['shape_dynamics_arrays']()
        got_hist = calls['shape_histogram_arrays']()
        torch.cuda.synchronize(dev)

    H = min(args.host_tracks, T)
    host = {}
    t0 = time.perf_counter()
    want_q = S.coords(pos[:H], 4, 3, mpp)
    host['coords_ms'] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want_dyn = S.dynamics(want_q, lags, fps)
    host['dynamics_ms'] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    S.histogram(want_q, 4, bond_max, BOND_DR, ANGLE_BINS)
    host['histogram_ms'] = (time.perf_counter() - t0) * 1e3
    host['tracks'] = H

    q = got_q[:H].cpu().numpy()
    ok = np.isfinite(want_q)
    m2, w2 = got_dyn.mean_d2[:H].cpu().numpy(), want_dyn['mean_d2']
    fin = np.isfinite(w2)
    C = S.n_coords(4)
    halo = S.shp_halo(F, C)
    dyn, dif = stats(ms['shape_dynamics_arrays']), stats(ms['diffusion_tensor'])
    out = dict(
        tracks=T, frames=F, lags=int(len(lags)), coordinates=C, bond_bins=BOND_BINS, angle_bins=ANGLE_BINS,
        device={name: stats(v) for name, v in ms.items()},
        dynamics_over_diffusion_median=dyn['median_ms'] / dif['median_ms'],
        dynamics_plan=dict(tile=S.TILE, halo=halo, lds_bytes=S.shp_lds_bytes(halo, C),
                           lags_from_global=int(sum(S.shp_reads_global(F, C, int(k)) for k in lags))),
        host_restatement=host,
        agreement=dict(nan_pattern_equal=bool((np.isnan(q) == np.isnan(want_q)).all()),
                       bonds_rg_equal=bool(np.array_equal(q[..., :6], want_q[..., :6], equal_nan=True)
                                           and np.array_equal(q[..., 18], want_q[..., 18], equal_nan=True)),
                       angles_max_abs=float(np.abs(q[ok] - want_q[ok]).max()),
                       counts_equal=bool((got_dyn.n[:H].cpu().numpy() == want_dyn['n']).all()),
                       mean_d2_max_rel=float((np.abs(m2[fin] - w2[fin]) / np.abs(w2[fin])).max()),
                       histogram_sum_identity=bool(((got_hist.count_bond.sum(-1) + got_hist.above) == got_hist.n).all().item())))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
