"""Time of the training stage (``ct.train_arrays``, ``ctr_train_device``) on cfg-2 frames
(512 x 512 uint8, 200 Gaussians of size 3, Poisson noise 10, diameter 13); writes
``profiles/train_time.json``.  Median of 5 calls between device events after a warm-up.

    python tools/train_time.py [--frames 1250] [--out profiles/train_time.json]

Measured: one frame as one problem; all frames as that many problems in one call; the same frames
as one call each; the blind queue (``check_every=0``) against reading a flag every K iterations;
iterations per problem; the NumPy yardstick (``tests/_train.py``, one core) on the single frame.
``--reference`` (no GPU needed; where the reference's tree is present, oracle/refshim.py) times the
reference's own global-mode ``refine_leastsq`` on the same single frame on one core and adds the
figure to the JSON; until that has run the JSON names it as not measured.
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

import clustertracking_amd as ct  # noqa: E402
from clustertracking_amd import artificial, train  # noqa: E402


def frame_problem(seed):
    im, truth, p0 = artificial.random_frame((512, 512), 200, 3., 100, 10, seed, margin=13)
    f = np.zeros((len(p0), 5))
    f[:, 0], f[:, 1], f[:, 2:4], f[:, 4] = 5., 100., p0, 3.6
    import pandas as pd
    df = pd.DataFrame(p0, columns=['y', 'x'])
    df['frame'] = 0
    df = ct.find_clusters(df, 13, ['y', 'x'])
    order = np.argsort(df['cluster'].values, kind='stable')
    cl = df['cluster'].values[order]
    starts = np.flatnonzero(np.r_[True, cl[1:] != cl[:-1]])
    return im, f[order], np.append(starts, len(order)).astype(np.int32)


def median_ms(call, n=5):
    import torch
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [float(t) for t in times]


def time_reference(path):
    """the reference's global-mode refine_leastsq (tol=1e-7, as train_leastsq calls it) on frame 0"""
    import warnings
    import pandas as pd
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import refshim
    ref = refshim.load()
    im, params, _ = frame_problem(0)
    f = pd.DataFrame(params[:, 2:4], columns=['y', 'x'])
    f['signal'], f['size'], f['background'], f['frame'] = params[:, 1], params[:, 4], params[:, 0], 0
    mode = dict(y='const', x='const', signal='const', background='const', size='global')
    times, size = [], None
    for _ in range(3):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t0 = time.perf_counter()
            res = ref.refine_leastsq(f.copy(), im, 13, fit_function='gauss', param_mode=mode, tol=1e-7,
                                     bounds=dict(size_rel_diff=(0.9, 9)))
            times.append(time.perf_counter() - t0)
        size = float(res['size'].mean())
    out = json.load(open(path)) if os.path.exists(path) else {}
    out['reference_global_refine_leastsq_one_core_s'] = float(np.median(times))
    out['reference_global_refine_leastsq_size'] = size
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: out[k] for k in out if k.startswith('reference')}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_time.json'))
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
    problem_offset = np.cumsum([0] + n_cl).astype(np.int32)
    bounds = train.training_bounds(None, ['size'])

    def one(i, **kw):
        return ct.train_arrays(frames[i:i + 1], probs[i][1], probs[i][2], np.zeros(n_cl[i], np.int32),
                               np.array([0, n_cl[i]], np.int32), 13, 'gauss', bounds=bounds, **kw)

    def batch(**kw):
        return ct.train_arrays(frames, params, feat_offset, frame_index, problem_offset, 13, 'gauss', bounds=bounds, **kw)

    out = {'workload': 'cfg-2 frames: 512x512 uint8, 200 Gaussians, size 3, noise 10, diameter 13; one shared size',
           'frames': args.frames, 'clusters_per_frame_mean': float(np.mean(n_cl)),
           'note': 'ms between device events around ct.train_arrays (uploads of the tables included), median of 5 '
                   'after a warm-up; the three headline figures with the blind queue (check_every=0), the variants under queue'}
    print('problems ready', flush=True)
    out['one_frame_one_problem_ms'], _ = median_ms(lambda: one(0, check_every=0))
    out['all_frames_one_call_ms'], out['all_frames_one_call_ms_runs'] = median_ms(lambda: batch(check_every=0))
    out['all_frames_one_call_each_ms'], _ = median_ms(lambda: [one(i, check_every=0) for i in range(args.frames)], n=1 if args.frames > 300 else 5)
    print('calls timed', flush=True)
    res = batch()
    out['iterations_per_problem'] = {'mean': float(res.n_iter.float().mean()), 'max': int(res.n_iter.max()),
                                     'failed': int((res.status != 0).sum())}
    out['queue'] = {}
    for k in (0, 4, 8, 16):
        print('queue variant', k, flush=True)
        out['queue']['check_every_%d' % k] = {'one_frame_ms': median_ms(lambda: one(0, check_every=k))[0],
                                              'all_frames_ms': median_ms(lambda: batch(check_every=k))[0]}
    import _train
    t0 = time.perf_counter()
    y = _train.Problem(probs[0][0][None], probs[0][1], probs[0][2], np.zeros(n_cl[0], int), 13)
    x0 = y.start()
    x = y.solve(x0 * 0.1, x0 * 10.)
    out['yardstick_one_frame_one_core_s'] = time.perf_counter() - t0
    out['yardstick_vs_device_size'] = [float(x[0]), float(one(0).globals[0, 0])]
    out['reference_global_refine_leastsq_one_core_s'] = 'not measured'
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
