"""Time of the global fit (``ct.refine_global_arrays``, ``ctr_refine_global_device``) on cfg-2 frames
(512 x 512 uint8, 200 Gaussians of size 3, Poisson noise 10, diameter 13; ``size`` global, the rest
default: background per cluster, signal and positions per feature); writes
``profiles/refine_global_time.json``.  Median and range of 5 calls after a warm-up, in one process,
the workloads alternating.

    python tools/refine_global_time.py [--frames 1250] [--out profiles/refine_global_time.json]

Measured: one frame as one problem; all frames as that many problems in one call; all frames as one
problem; ``train_arrays`` on the same tables with everything else constant (what the locals cost
per iteration); ``refine_arrays`` with ``size`` constant at the fitted value (what the coupling
costs over the uncoupled fit); iterations and launches per iteration.  Wall-clock times of the
whole call: the host packs start values and bounds and uploads the tables inside it.
``--reference`` (no GPU needed; where the reference's tree is present, oracle/refshim.py) times the
reference's own global-mode ``refine_leastsq`` on the single frame on one core and adds the figure
to the JSON; until that has run the JSON names it as not measured.
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import clustertracking_amd as ct  # noqa: E402
from clustertracking_amd import _lib, train  # noqa: E402
from train_time import frame_problem  # noqa: E402

rg = importlib.import_module('clustertracking_amd.refine_global')
MODE = dict(size='global')


def timed(calls, n=5):
    """{name: (median ms, [ms])} of the calls, alternating, after one warm-up each"""
    import torch
    for call in calls.values():
        call()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(n):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
    return {name: {'median_ms': float(np.median(t)), 'min_ms': float(min(t)), 'max_ms': float(max(t))}
            for name, t in times.items()}


def time_reference(path):
    """the reference's global-mode refine_leastsq (size global, the rest default, tol=1e-7) on frame 0"""
    import warnings
    import pandas as pd
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import refshim
    ref = refshim.load()
    im, params, _ = frame_problem(0)
    f = pd.DataFrame(params[:, 2:4], columns=['y', 'x'])
    f['signal'], f['size'], f['background'], f['frame'] = params[:, 1], params[:, 4], params[:, 0], 0
    times, size, failed = [], None, 0
    for _ in range(3):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t0 = time.perf_counter()
            res = ref.refine_leastsq(f.copy(), im, 13, fit_function='gauss', param_mode=MODE, tol=1e-7)
            times.append(time.perf_counter() - t0)
        size = float(res['size'].mean())
        failed += int(not np.isfinite(res['cost']).all())      # refine.py:408-412: a failed fit has a NaN cost
    out = json.load(open(path)) if os.path.exists(path) else {}
    out['reference_global_refine_leastsq_one_core_s'] = float(np.median(times))
    out['reference_global_refine_leastsq_size'] = size
    out['reference_global_refine_leastsq_failed_runs'] = failed
    out['reference_note'] = ("the reference's refine_leastsq with size 'global' and the rest default, tol=1e-7 and its default "
                             "limit of 100 SLSQP iterations, on frame 0, one CPU core (tools/refine_global_time.py "
                             "--reference); median of 3; failed_runs counts the runs that ended with a NaN cost (a "
                             "failed fit: the table, the size included, is then unchanged)")
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: out[k] for k in out if k.startswith('reference')}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'refine_global_time.json'))
    ap.add_argument('--reference', action='store_true')
    args = ap.parse_args()
    if args.reference:
        return time_reference(args.out)
    import torch
    probs = [frame_problem(s) for s in range(args.frames)]
    frames = torch.from_numpy(np.stack([p[0] for p in probs])).cuda()
    params = np.concatenate([p[1] for p in probs])
    n_cl = [len(p[2]) - 1 for p in probs]
    n_ft = np.cumsum([0] + [len(p[1]) for p in probs])
    feat_offset = np.concatenate([[0]] + [p[2][1:] + o for p, o in zip(probs, n_ft[:-1])]).astype(np.int32)
    frame_index = np.repeat(np.arange(len(probs)), n_cl).astype(np.int32)
    per_frame = np.cumsum([0] + n_cl).astype(np.int32)
    whole = np.array([0, len(frame_index)], np.int32)
    sizes = np.diff(feat_offset)
    ff = rg.global_param_mode('gauss', 2, True, MODE)
    keep = np.flatnonzero(np.repeat(sizes, sizes) * 3 + 3 <= rg.MAX_COLUMNS)      # (no cfg-2 cluster is beyond 48 columns)
    assert len(keep) == len(params)
    tbounds = train.training_bounds(None, ['size'])

    def one(**kw):
        return ct.refine_global_arrays(frames[:1], probs[0][1], probs[0][2], np.zeros(n_cl[0], np.int32),
                                       np.array([0, n_cl[0]], np.int32), 13, param_mode=MODE, **kw)

    def batch(problem_offset, **kw):
        return ct.refine_global_arrays(frames, params, feat_offset, frame_index, problem_offset, 13, param_mode=MODE, **kw)

    out = {'workload': 'cfg-2 frames: 512x512 uint8, 200 Gaussians, size 3, noise 10, diameter 13; size global, '
                       'background per cluster, signal and positions per feature',
           'frames': args.frames, 'clusters_per_frame_mean': float(np.mean(n_cl)), 'largest_cluster': int(sizes.max()),
           'note': 'wall-clock ms of the whole call (host packing of start and bounds, uploads, the queue, the final '
                   'synchronisation), median and range of 5 after a warm-up, the workloads alternating in one process'}
    res1 = one()
    d = rg.descriptor(ff, (512, 512), np.uint8, 1, (6, 6))
    d.max_locals = rg.n_locals(ff, sizes.max())
    out['launches_per_iteration'] = _lib.refine_global_plan(d).launches_per_iteration
    out['tiles_of_a_row'] = _lib.refine_global_plan(d).tiles
    print('problems ready', flush=True)
    t = timed({
        'global_one_frame': one,
        'train_one_frame': lambda: ct.train_arrays(frames[:1], probs[0][1], probs[0][2], np.zeros(n_cl[0], np.int32),
                                                   np.array([0, n_cl[0]], np.int32), 13, bounds=tbounds),
    })
    out.update(t)
    print('one frame timed', flush=True)
    t = timed({
        'global_all_frames_one_problem_each': lambda: batch(per_frame),
        'global_all_frames_one_problem': lambda: batch(whole),
        'train_all_frames_one_problem_each': lambda: ct.train_arrays(frames, params, feat_offset, frame_index, per_frame, 13,
                                                                     bounds=tbounds),
    })
    out.update(t)
    print('all frames timed', flush=True)
    res_each, res_whole = batch(per_frame), batch(whole)
    tr = ct.train_arrays(frames, params, feat_offset, frame_index, per_frame, 13, bounds=tbounds)
    out['iterations'] = {
        'global_one_frame': int(res1.n_iter[0]), 'rounds_one_frame': int(res1.n_rounds[0]),
        'global_per_frame_mean': float(res_each.n_iter.float().mean()), 'global_per_frame_max': int(res_each.n_iter.max()),
        'rounds_per_frame_max': int(res_each.n_rounds.max()), 'failed_per_frame': int((res_each.status != 0).sum()),
        'global_one_problem': int(res_whole.n_iter[0]), 'rounds_one_problem': int(res_whole.n_rounds[0]),
        'status_one_problem': int(res_whole.status[0]),
        'train_per_frame_mean': float(tr.n_iter.float().mean())}
    # the problems that failed: which status, which frames, how many rounds and iterations they took
    from clustertracking_amd import _abi
    st = res_each.status.cpu().numpy()
    bad = np.flatnonzero(st != 0)
    out['failed_per_frame'] = {
        'statuses': {_abi.STATUS_TEXT.get(int(c), str(int(c))): int((st[bad] == c).sum()) for c in np.unique(st[bad])},
        'frames': [int(i) for i in bad], 'rounds': [int(res_each.n_rounds[i]) for i in bad],
        'iterations': [int(res_each.n_iter[i]) for i in bad]}
    rounds = res_each.n_rounds.cpu().numpy()
    out['rounds_per_frame_histogram'] = {str(int(r)): int((rounds == r).sum()) for r in np.unique(rounds)}
    if int(res_whole.status[0]) != 0:
        out['note_one_problem'] = ('all frames as ONE problem ended with status %d (%s) after %d iterations: its time is that of '
                                   'those iterations' % (int(res_whole.status[0]), _abi.STATUS_TEXT.get(int(res_whole.status[0]), '?'),
                                                         int(res_whole.n_iter[0])))
    finite = lambda x: float(x) if np.isfinite(float(x)) else None
    out['size'] = {'one_frame': finite(res1.globals[0, 0]), 'all_frames_one_problem': finite(res_whole.globals[0, 0]),
                   'train_one_frame': finite(tr.globals[0, 0])}
    # the uncoupled fit of the same frame with the size constant at the fitted value
    p1, size1 = probs[0][1], float(res1.globals[0, 0])
    fo1 = np.array([0, len(p1)], np.int64)
    fo_all = n_ft.astype(np.int64)
    out.update(timed({
        'refine_arrays_one_frame_size_constant': lambda: ct.refine_arrays(
            frames[:1].cpu().numpy(), p1[:, 2:4], fo1, 13, signal=p1[:, 1], size=size1, background=p1[:, 0]),
        'refine_arrays_all_frames_size_constant': lambda: ct.refine_arrays(
            frames, torch.from_numpy(params[:, 2:4].copy()).cuda(), torch.from_numpy(fo_all).cuda(), 13,
            signal=100., size=size1, background=5.),
    }))
    out['reference_global_refine_leastsq_one_core_s'] = 'not measured'
    committed = os.path.join(ROOT, 'profiles', 'refine_global_time.json')
    if os.path.exists(committed):      # what --reference added there earlier stays
        out.update({k: v for k, v in json.load(open(committed)).items() if k.startswith('reference')})
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
