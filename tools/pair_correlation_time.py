"""Time the pair correlation stage on the MI355X (ctr_pair_correlation_device) against the
same rule restated in NumPy on the host (tests/_pair_correlation.py), not against trackpy.

    python tools/pair_correlation_time.py [--reps 5] [--frames 1250] [--rows 20000] [--out profiles/pair_correlation_time.json]

Two tables.  ``cfg2``: the positions that ``find_link_arrays`` returns for `--frames` cfg-2 frames (512 x
512 uint8, 200 Gaussians each, diameter 13, separation 13, search range 5) with ``minmass = 0``, so the
noise maxima are rows too (where the linker refuses the table, ``locate_arrays`` of the same frames
gives it; the file says which).  ``one_frame``: `--rows` uniform points in a 2048 x 2048 box, one frame.
``cutoff = 40``, ``dr = 0.5``, each ``edge`` mode, the table on the device and the results left there; HIP
events on a stream of its own around one call after a warm-up call, median / minimum / maximum of
`reps`.  Next to it, wall clock on one core in the same process, one run: the restatement in ``'arc'``
mode.  The device's counts must equal the host's; the largest deviation of ``weight`` from the
restatement, per reference row, is recorded (the tests bound it by 1e-14).
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

DIAMETER, SEPARATION, SEARCH_RANGE = 13, 13, 5
CUTOFF, DR = 40., 0.5


def spread(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--rows', type=int, default=20000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import _pair_correlation as yard
    import clustertracking_amd as ct
    from clustertracking_amd import _abi, _lib, workloads
    from clustertracking_amd.find import locate_arrays
    from clustertracking_amd.link import SubnetOversizeException

    _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    own = torch.cuda.Stream(dev)

    def timed(fn):
        with torch.cuda.stream(own):
            out = fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(own)
                fn()
                b.record(own)
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
        return out, spread(ms)

    def measure(name, t_pos, t_off):
        res, ok, counts = {}, True, {}
        for edge in ('none', 'interior', 'arc'):
            got, res[edge] = timed(lambda: ct.pair_correlation_arrays(t_pos, t_off, CUTOFF, DR, edge=edge))
            ok = ok and int(got.status) == _abi.PCF_OK
            counts[edge] = got.count.cpu().numpy()
            res[edge].update(ordered_pairs_binned=int(counts[edge].sum()), reference_rows=int(got.n_ref.sum().item()))
            print(name, edge, res[edge], flush=True)
        same = bool((counts['none'] == counts['arc']).all())
        pos, off = t_pos.cpu().numpy(), t_off.cpu().numpy()
        t0 = time.perf_counter()
        want = yard.pair_correlation(pos, off, CUTOFF, DR, edge='arc')
        host_ms = (time.perf_counter() - t0) * 1e3
        weight = got.weight.cpu().numpy()
        dev_w = np.abs(weight - want.weight) / np.maximum(want.n_ref[:, None], 1)
        g, g_want = got.g.cpu().numpy(), want.g
        same = same and bool((counts['arc'] == want.count).all()) and bool((got.n_ref.cpu().numpy() == want.n_ref).all())
        res['arc'].update(host_restatement_ms=host_ms, counts_equal_host=same,
                          largest_weight_deviation_per_reference_row=float(dev_w.max()) if dev_w.size else 0.,
                          largest_relative_deviation_of_g=float(np.nanmax(np.abs(g - g_want) / np.abs(g_want))),
                          g_first_bins=[float(x) for x in g[:4]], g_last_bins=[float(x) for x in g[-4:]])
        print(name, 'host', host_ms, 'ms', flush=True)
        shape = dict(frames=int(len(off) - 1), rows=int(len(pos)), rows_per_frame=float(len(pos)) / max(len(off) - 1, 1),
                     distance_evaluations=int((np.diff(off) ** 2).sum()))
        return shape, res, ok and same

    frames = workloads.cfg2(n_frames=args.frames)[0]
    print('drawn', flush=True)
    d_frames = torch.from_numpy(frames).to(dev)
    try:
        r = ct.find_link_arrays(d_frames, search_range=SEARCH_RANGE, separation=SEPARATION, diameter=DIAMETER, minmass=0,
                                max_queries=1024, max_relocated=1024, _on_device=True)
        t_pos, t_off, source = r.pos, r.frame_offset, 'find_link_arrays'
    except (_lib.EngineError, SubnetOversizeException) as e:
        print('find_link_arrays refused the table (%s): locate_arrays instead' % e, flush=True)
        _, _, pos_i, t_off, _ = locate_arrays(d_frames, SEPARATION, 64, (DIAMETER // 2,) * 2, _on_device=True)
        t_pos, source = pos_i.to(torch.float64), 'locate_arrays (find_link_arrays refused: %s)' % e
    del d_frames
    print('located', int(t_pos.shape[0]), 'rows', flush=True)
    shape_a, res_a, ok_a = measure('cfg2', t_pos, t_off)
    shape_a.update(generator='workloads.cfg2(n_frames=%d), minmass 0' % args.frames, table=source, diameter=DIAMETER,
                   separation=SEPARATION, search_range=SEARCH_RANGE)

    rng = np.random.RandomState(7)
    one = torch.from_numpy(rng.uniform(0., 2048., (args.rows, 2))).to(dev)
    shape_b, res_b, ok_b = measure('one_frame', one, torch.tensor([0, args.rows], dtype=torch.int64, device=dev))
    shape_b.update(generator='uniform points in a 2048 x 2048 box, one frame')

    out = dict(
        method=dict(reps=args.reps, warmup_calls=1, cutoff=CUTOFF, dr=DR, bins=int(np.ceil(CUTOFF / DR)),
                    clock='HIP events on a stream of its own around one call, the default box (a reduction in torch) included; '
                          'median, minimum and maximum of reps',
                    inputs='the table on the device, results left there',
                    host='wall clock, one core, one run, the same process: tests/_pair_correlation.py in arc mode, '
                         'vectorised per frame; not trackpy',
                    max_bins=_abi.PCF_MAX_BINS),
        cfg2=dict(workload=shape_a, device=res_a), one_frame=dict(workload=shape_b, device=res_b))
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not (ok_a and ok_b):
        sys.exit('the device and the host rule disagree')


if __name__ == '__main__':
    main()
