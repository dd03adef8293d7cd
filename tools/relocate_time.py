"""Time the relocation candidates on the MI355X (ctr_relocate_device) against the
NumPy restatement.

    python tools/relocate_time.py [--reps 5] [--frames 1250] [--out profiles/relocate_time.json]

Workload: `--frames` frames of 512 x 512 uint8 drawn by ``workloads.cfg2(n_frames=...)`` with 200
Gaussians each (the feature count of the cfg-4 shard, for which workloads.py has no generator),
diameter 13, separation 13, search_range 5.  The frames are located on the device, which finds
about 540 maxima per frame (the noise maxima above the threshold included: no minmass cut); per
frame 10 of these located maxima are taken out of the known ones and offered, shifted by up to 2 px,
as one-source queries: 10 queries per frame.
Timed two ways, inputs on the device, outputs preallocated, descriptors prebuilt: one call per
frame (10 queries each, as a relocation loop would issue them) and all frames in one call.  Device
time: HIP events on a stream of its own around one pass over all frames, after a warm-up pass;
the median of `reps` passes.  Host time: wall clock of tests/_relocate.py (NumPy, one core) on the
queries of the first `--host-frames` frames, whose candidates are also compared with the device's.
Bytes, computed from the shapes: per query its box of the frame, the known rows of its frame (the
kernel scans them all), its sources and its K output rows.
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/relocate_time.py`.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PER_FRAME, K = 10, 4
DIAMETER, SEPARATION, SEARCH_RANGE = 13, 13, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--host-frames', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import _relocate as R
    from clustertracking_amd import _lib, relocate, workloads
    from clustertracking_amd.find import locate_arrays

    eng = _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    F = args.frames
    frames = workloads.cfg2(n_frames=F)[0]
    t, pix, pos, offset, thr = locate_arrays(frames, SEPARATION, 64, _on_device=True)
    pos_h, off_h, thr_h = pos.cpu().numpy(), offset.cpu().numpy(), thr.cpu().numpy()
    rng = np.random.RandomState(0)
    lost = np.concatenate([off_h[f] + rng.choice(off_h[f + 1] - off_h[f], PER_FRAME, replace=False) for f in range(F)])
    keep = np.ones(len(pos_h), dtype=bool)
    keep[lost] = False
    known = pos_h[keep].astype(np.float64)
    known_off = off_h - PER_FRAME * np.arange(F + 1)
    sources = pos_h[lost] + rng.uniform(-2, 2, (len(lost), 2))
    Q = len(lost)
    qframe = np.repeat(np.arange(F, dtype=np.int64), PER_FRAME)

    d_known, d_koff = torch.from_numpy(known).to(dev), torch.from_numpy(known_off).to(dev)
    d_src = torch.from_numpy(sources).to(dev)
    d_soff = torch.arange(Q + 1, dtype=torch.int64, device=dev)
    d_qf = torch.from_numpy(qframe).to(dev)
    n_found = torch.zeros(Q, dtype=torch.int32, device=dev)
    status = torch.zeros(Q, dtype=torch.int32, device=dev)
    cand = torch.empty((Q, K, 2), dtype=torch.int32, device=dev)
    mass, signal, size = (torch.empty((Q, K), dtype=torch.float64, device=dev) for _ in range(3))

    def descriptor(q0, q1):
        r = relocate.descriptor(frames.shape[1:], pix, F, DIAMETER, SEPARATION, SEARCH_RANGE, max_candidates=K)
        r.frames, r.threshold = t.data_ptr(), thr.data_ptr()
        r.n_known, r.known_pos, r.known_offset = len(known), d_known.data_ptr(), d_koff.data_ptr()
        r.n_queries = q1 - q0
        r.query_frame, r.source_offset, r.source_pos = d_qf.data_ptr() + 8 * q0, d_soff.data_ptr() + 8 * q0, d_src.data_ptr()
        r.n_found, r.status = n_found.data_ptr() + 4 * q0, status.data_ptr() + 4 * q0
        r.cand_pos = cand.data_ptr() + 4 * 2 * K * q0
        r.mass, r.signal, r.size = (x.data_ptr() + 8 * K * q0 for x in (mass, signal, size))
        return r

    whole = descriptor(0, Q)
    per_frame = [descriptor(f * PER_FRAME, (f + 1) * PER_FRAME) for f in range(F)]
    own = torch.cuda.Stream(dev)     # see tools/characterize_time.py

    def one_call():
        eng.relocate_device(whole, own.cuda_stream)

    def call_per_frame():
        for r in per_frame:
            eng.relocate_device(r, own.cuda_stream)

    def timed(fn):
        fn()                                      # warm-up: the same shapes as the timed passes
        torch.cuda.synchronize()
        ms, wall = [], []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record(own)
            fn()
            b.record(own)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(a.elapsed_time(b))
        return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)),
                    host_wall_median_ms=float(np.median(wall)))

    torch.cuda.synchronize(dev)
    t_one = timed(one_call)
    got = [x.cpu().numpy().copy() for x in (n_found, cand, mass, status)]
    t_loop = timed(call_per_frame)
    same = all(np.array_equal(a, x.cpu().numpy(), equal_nan=True) for a, x in zip(got, (n_found, cand, mass, status)))

    HF = min(args.host_frames, F)
    agree, t0 = True, time.perf_counter()
    host_found = 0
    for q in range(HF * PER_FRAME):
        f = qframe[q]
        coords, extra = R.compose(frames[f], thr_h[f], sources[q:q + 1], known[known_off[f]:known_off[f + 1]],
                                  DIAMETER, SEPARATION, SEARCH_RANGE)
        n = 0 if coords is None else len(coords)
        host_found += n
        m = min(n, K)
        agree = agree and got[0][q] == n and (n == 0 or (np.array_equal(got[1][q, :m], coords[:m])
                                                         and np.array_equal(got[2][q, :m], extra['mass'][:m])))
    host_ms = (time.perf_counter() - t0) * 1e3

    d = R.derived((DIAMETER,) * 2, (SEPARATION,) * 2, (SEARCH_RANGE,) * 2)
    box = 0
    for s in sources:
        o, e = R.box_of(s[None], frames.shape[1:], d['slice_radius'])
        box += int(np.prod(e - o))
    known_rows = int(np.sum(np.diff(known_off)[qframe]))
    by = dict(box_pixels=box * frames.dtype.itemsize, known_rows_scanned=known_rows * 16, sources=Q * 16,
              outputs=Q * (K * (8 + 3 * 8) + 8))
    by['total'] = sum(by.values())
    tile, lds = _lib.relocate_plan(whole)
    out = dict(
        workload=dict(generator='workloads.cfg2(n_frames=%d)' % F, frames=F, shape=list(frames.shape[1:]), dtype=str(frames.dtype),
                      features_per_frame=float(len(pos_h)) / F, queries=Q, queries_per_frame=PER_FRAME, sources_per_query=1,
                      diameter=DIAMETER, separation=SEPARATION, search_range=SEARCH_RANGE, max_candidates=K),
        method=dict(reps=args.reps, warmup_passes=1, clock='HIP events on a stream of its own around one pass over all frames; '
                    'median of reps', inputs='on the device, descriptors prebuilt, outputs preallocated'),
        plan=dict(tile_pixels=tile, lds_bytes=lds),
        device=dict(one_call=t_one, call_per_frame=t_loop,
                    one_call_us_per_query=t_one['median_ms'] * 1e3 / Q,
                    call_per_frame_us_per_call=t_loop['median_ms'] * 1e3 / F,
                    candidates_found=int(got[0].sum()), queries_with_candidates=int((got[0] > 0).sum()),
                    status_nonzero=int((got[3] != 0).sum()), loop_equals_one_call=bool(same)),
        host_restatement=dict(queries=HF * PER_FRAME, ms=host_ms, ms_per_query=host_ms / (HF * PER_FRAME),
                              candidates_found=host_found, equals_device=bool(agree)),
        speedup=dict(one_call_per_query=(host_ms / (HF * PER_FRAME)) / (t_one['median_ms'] / Q),
                     call_per_frame_per_query=(host_ms / (HF * PER_FRAME)) / (t_loop['median_ms'] / Q)),
        bytes=by,
    )
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not (agree and same):
        sys.exit('the device and the restatement disagree')


if __name__ == '__main__':
    main()
