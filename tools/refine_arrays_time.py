"""Time ``ct.refine_arrays`` on the MI355X against the DataFrame path it stands beside.

    python tools/refine_arrays_time.py [--frames 256] [--reps 5] [--out profiles/refine_arrays_time.json]

Workload: the cfg-2 batch of bench.py's ``drop_in_end_to_end`` (``workloads.cfg2``: 512 x 512 uint8
frames of 200 Gaussians each, default modes), generated from seeds.
Timed in one process, one call of each after the other, ``reps`` times after one warm-up round
(median, minimum, maximum and every value; a host clock around work that ends in a device
synchronise):
  prepare_stage: ``refine.prepare_arrays`` -- ctr_refine_prepare_device on tensors that are on the
    device, with its copy of three words to the host;
  refine_arrays: ``ct.refine_arrays`` end to end, frames, positions and offsets on the device, the
    results left there (the one synchronisation and the plan included);
  refine_leastsq: ``ct.refine_leastsq(cluster_labels='device')`` from a DataFrame and host frames to
    a DataFrame, and its three stages apart as bench.py times them (prepare_batch, ctr_refine_batch
    with its PCIe copies, write_back): the yardstick, measured again in this run.
Before any timing the two paths' results are compared byte for byte.  No threshold: the numbers are
the result."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), all_ms=[float(x) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import clustertracking_amd as ct
    from clustertracking_amd import _lib, refine, workloads
    from clustertracking_amd.fitfunc import FitFunctions

    eng = _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    frames, f0, _, opts = workloads.cfg2(n_frames=args.frames)
    diameter = opts['diameter']
    reader = ct.ArrayReader(frames)
    n = len(f0)
    off = np.searchsorted(f0['frame'].values, np.arange(args.frames + 1)).astype(np.int64)
    dev = torch.device('cuda', 0)
    t_frames = torch.from_numpy(frames).to(dev)
    t_pos = torch.from_numpy(np.ascontiguousarray(f0[['y', 'x']].values)).to(dev)
    t_off = torch.from_numpy(off).to(dev)
    signal, size, background = (float(f0[c].iloc[0]) for c in ('signal', 'size', 'background'))
    ff = FitFunctions('gauss', 2, True)
    t_params0 = torch.from_numpy(np.ascontiguousarray(f0[ff.params].values)).to(dev)
    radius = (diameter // 2,) * 2

    def sync():
        torch.cuda.synchronize(dev)

    def prepare_stage():
        return refine.prepare_arrays(t_pos, t_off, t_params0, diameter, ff, None, radius)

    def arrays():
        return ct.refine_arrays(t_frames, t_pos, t_off, diameter, signal=signal, size=size, background=background)

    def tables():
        return ct.refine_leastsq(f0, reader, diameter, cluster_labels='device')

    stages = {}

    def tables_in_stages():
        t0 = time.perf_counter()
        pr = ct.prepare_batch(f0, reader, diameter, cluster_labels='device')
        t1 = time.perf_counter()
        eng.refine_batch(pr.problem, pr.batch)
        t2 = time.perf_counter()
        ct.write_back(pr)
        t3 = time.perf_counter()
        for key, dt in (('prepare_batch', t1 - t0), ('engine_call_incl_pcie', t2 - t1), ('write_back', t3 - t2)):
            stages.setdefault(key, []).append(dt * 1e3)

    # the same bytes first
    res, f = arrays(), tables()
    same = all(res.params[:, k].cpu().numpy().tobytes() == f[col].values.tobytes() for k, col in enumerate(res.columns))
    same = same and res.cost.cpu().numpy().tobytes() == f['cost'].values.tobytes() \
        and np.array_equal(res.cluster.cpu().numpy(), f['cluster'].values)
    prep = prepare_stage()

    calls = dict(prepare_stage=prepare_stage, refine_arrays=arrays, refine_leastsq=tables, stages=tables_in_stages)
    times = {k: [] for k in calls}
    for rep in range(args.reps + 1):
        for key, fn in calls.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[key].append((time.perf_counter() - t0) * 1e3)
    n_fits = int(prep.n_clusters)
    result = dict(
        method=dict(reps=args.reps, warmup_rounds=1,
                    clock='host clock around one call, the device synchronised before and after; the calls alternate '
                          'in one process; median, minimum and maximum of reps',
                    inputs='prepare_stage and refine_arrays: tensors on the device, results left there; refine_leastsq: a '
                           'DataFrame and host frames in, a DataFrame out'),
        workload=dict(name='cfg2', frames=args.frames, shape=list(frames.shape[1:]), rows=n, clusters=n_fits,
                      frame_bytes=int(frames.nbytes), largest_cluster=int(prep.cluster_size.max().item())),
        same_bytes_as_refine_leastsq=bool(same),
        prepare_stage=spread(times['prepare_stage'][1:]),
        refine_arrays=dict(spread(times['refine_arrays'][1:]),
                           fits_per_s=n_fits / (np.median(times['refine_arrays'][1:]) * 1e-3)),
        refine_leastsq=dict(spread(times['refine_leastsq'][1:]),
                            fits_per_s=n_fits / (np.median(times['refine_leastsq'][1:]) * 1e-3),
                            stages={k: spread(v[1:]) for k, v in stages.items()}))
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not same:
        sys.exit('refine_arrays and refine_leastsq disagree')


if __name__ == '__main__':
    main()
