"""Time linking on the MI355X (ctr_link_device) against the host linker.

    python tools/link_time.py [--reps 5] [--out FILE]

Inputs (random walkers, no oracle): the cfg-4 shard (1250 levels x 200 walkers in 512^2, steps
0.5 px, search_range 3), a dense video (40 levels x 150 walkers in 100^2, steps 1.5 px,
search_range 5: sub-networks of 10 x 10 and more) and a 3D one (200 levels x 500 walkers in
128^3, steps 1 px, search_range (3, 5, 5)); memory 0 and 2.  Device time: HIP events around
`reps` calls after warm-up, positions and offsets already on the device, outputs preallocated.
Host time: wall clock of `link.link_levels` on the same arrays in the same run (one core).
Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/link_time.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REFINE_CFG4_SHARD_S = 0.064   # DESIGN.md round 1, cfg 4: the shard refined end to end


def walkers(seed, n, n_levels, ndim, box, step):
    rng = np.random.RandomState(seed)
    pos = rng.uniform(0, box, (n, ndim))
    levels = []
    for _ in range(n_levels):
        pos = pos + rng.normal(0, step, pos.shape)
        levels.append(pos[rng.permutation(n)].copy())
    return levels


def time_device(levels, search_range, memory, reps, warmup=2):
    import torch
    from clustertracking_amd import _abi, _lib
    from clustertracking_amd.utils import validate_tuple
    eng = _lib.default_engine(0)
    dev = torch.device('cuda', 0)
    ndim = levels[0].shape[1]
    offs = np.r_[0, np.cumsum([len(l) for l in levels])].astype(np.int64)
    pos = torch.from_numpy(np.concatenate(levels)).to(dev)
    off = torch.from_numpy(offs).to(dev)
    n = int(pos.shape[0])
    particle = torch.empty(n, dtype=torch.int64, device=dev)
    n_tracks = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    d = _abi.Link()
    d.ndim, d.memory, d.n_levels, d.n_features = ndim, memory, len(levels), n
    for a, s in enumerate(validate_tuple(search_range, ndim)):
        d.search_range[a] = float(s)
    d.pos, d.frame_offset = pos.data_ptr(), off.data_ptr()
    d.particle, d.n_tracks, d.status = particle.data_ptr(), n_tracks.data_ptr(), status.data_ptr()
    torch.cuda.synchronize(dev)
    own = torch.cuda.Stream(dev)     # see tools/characterize_time.py
    for _ in range(warmup):
        eng.link_device(d, own.cuda_stream)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record(own)
    for _ in range(reps):
        eng.link_device(d, own.cuda_stream)
    b.record(own)
    queued = time.perf_counter() - t0
    torch.cuda.synchronize(dev)
    assert int(status[0].item()) == 0, status.tolist()
    return dict(call_ms=a.elapsed_time(b) / reps, host_queue_ms=queued * 1e3 / reps,
                n_tracks=int(n_tracks.item())), particle.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    from clustertracking_amd import link as lk
    inputs = {
        'cfg4_shard': (walkers(4, 200, 1250, 2, 512., 0.5), 3.),
        'dense2d': (walkers(5, 150, 40, 2, 100., 1.5), 5.),
        'walk3d': (walkers(6, 500, 200, 3, 128., 1.0), (3., 5., 5.)),
    }
    out = {}
    for name, (levels, sr) in inputs.items():
        for memory in (0, 2):
            t0 = time.perf_counter()
            want = np.concatenate(lk.link_levels(levels, sr, memory))
            host_s = time.perf_counter() - t0
            dev, ids = time_device(levels, sr, memory, args.reps)
            row = dict(levels=len(levels), features=int(len(want)), memory=memory, device=dev,
                       host_ms=host_s * 1e3, speedup=host_s * 1e3 / dev['call_ms'],
                       ids_equal_host=bool(np.array_equal(ids, want)))
            if name == 'cfg4_shard':
                row['share_of_refine'] = dev['call_ms'] / 1e3 / REFINE_CFG4_SHARD_S
            out['%s_m%d' % (name, memory)] = row
            print(name, memory, json.dumps(row), file=sys.stderr)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
