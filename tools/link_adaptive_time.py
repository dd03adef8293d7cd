"""Time linking with the adaptive search range on the MI355X (ctr_link_adaptive_device).

    python tools/link_adaptive_time.py [--parent-tree DIR] [--runs 5] [--reps 20] [--out FILE]

1. The plain path must not pay for the feature: ``ctr_link_device`` on the cfg-4 shard (1250 levels
   x 200 walkers in 512^2, steps 0.5 px, search_range 3, memory 0), this tree against a built
   checkout of the parent commit (``--parent-tree``; without it only this tree), one fresh process
   per run, alternating, ``--runs`` each: median and range.  The bar is the parent's own range.
2. A dense workload, no bar: the shard with a blob of 60 points in a 10 x 10 px box beside the
   frame in every level, on which the plain call raises.  The adaptive call on it, the host
   restatement on one core, and the adaptive call on the undisturbed shard (no round beyond 0).
Device time: HIP events around ``--reps`` calls after warm-up, positions and offsets already on the
device, outputs preallocated (as tools/link_time.py).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCH_RANGE, ADAPTIVE_STOP, ADAPTIVE_STEP = 3., .3, .9


def shard(blob):
    rng = np.random.RandomState(4)
    pos = rng.uniform(0, 512, (200, 2))
    dense = rng.uniform(0, 10, (60, 2)) + 600.
    levels = []
    for _ in range(1250):
        pos = pos + rng.normal(0, 0.5, pos.shape)
        dense = dense + rng.normal(0, 0.5, dense.shape)
        lvl = np.concatenate([pos, dense]) if blob else pos
        levels.append(lvl[rng.permutation(len(lvl))].copy())
    return levels


def time_device(levels, reps, plan=None, warmup=3):
    """ms per call of ctr_link_device (plan None) or ctr_link_adaptive_device (plan: stop_rel, step, K)"""
    import torch
    from clustertracking_amd import _abi, _lib
    eng = _lib.default_engine(0)
    dev = torch.device('cuda', 0)
    offs = np.r_[0, np.cumsum([len(l) for l in levels])].astype(np.int64)
    pos = torch.from_numpy(np.concatenate(levels)).to(dev)
    off = torch.from_numpy(offs).to(dev)
    n = int(pos.shape[0])
    particle = torch.empty(n, dtype=torch.int64, device=dev)
    rounds = torch.empty(n, dtype=torch.int32, device=dev)
    n_tracks = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    d = _abi.Link() if plan is None else _abi.LinkAdaptive()
    d.ndim, d.memory, d.n_levels, d.n_features = 2, 0, len(levels), n
    d.search_range[0] = d.search_range[1] = SEARCH_RANGE
    d.pos, d.frame_offset = pos.data_ptr(), off.data_ptr()
    d.particle, d.n_tracks, d.status = particle.data_ptr(), n_tracks.data_ptr(), status.data_ptr()
    call = eng.link_device
    if plan is not None:
        d.stop_rel, d.step, d.max_rounds = plan
        d.adaptive_round = rounds.data_ptr()
        call = eng.link_adaptive_device
    torch.cuda.synchronize(dev)
    own = torch.cuda.Stream(dev)
    for _ in range(warmup):
        call(d, own.cuda_stream)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(own)
    for _ in range(reps):
        call(d, own.cuda_stream)
    b.record(own)
    torch.cuda.synchronize(dev)
    assert int(status[0].item()) == 0, status.tolist()
    return a.elapsed_time(b) / reps, particle.cpu().numpy(), rounds.cpu().numpy()


def child_plain(reps):
    ms, ids, _ = time_device(shard(False), reps)
    print(json.dumps(dict(call_ms=ms, n_tracks=int(ids.max()) + 1)))


def run_child(tree, reps):
    env = dict(os.environ, PYTHONPATH=tree)
    env.pop('CTREFINE_LIB', None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--tree', tree, '--reps', str(reps)],
                         env=env, cwd=tree, stdout=subprocess.PIPE, universal_newlines=True, timeout=600, check=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def spread(values):
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)), runs=[float(v) for v in values])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    sys.path.insert(0, args.tree)
    if args.child:
        return child_plain(args.reps)

    out = {}
    trees = [('this', ROOT)] + ([('parent', os.path.abspath(args.parent_tree))] if args.parent_tree else [])
    runs = {name: [] for name, _ in trees}
    for r in range(args.runs):
        for name, tree in trees:
            res = run_child(tree, args.reps)
            runs[name].append(res['call_ms'])
            print('plain, cfg-4 shard, run %d, %s: %.4f ms' % (r, name, res['call_ms']), file=sys.stderr)
    out['plain_cfg4_shard_ms'] = {name: spread(v) for name, v in runs.items()}
    if 'parent' in runs:
        p, t = out['plain_cfg4_shard_ms']['parent'], out['plain_cfg4_shard_ms']['this']
        out['plain_cfg4_shard_ms']['this_median_within_parent_range'] = bool(t['median'] <= p['max'])

    from clustertracking_amd import link as lk
    plan = lk._adaptive_plan((SEARCH_RANGE, SEARCH_RANGE), ADAPTIVE_STOP, ADAPTIVE_STEP)
    plain_levels, dense_levels = shard(False), shard(True)
    try:
        lk.link_levels(dense_levels[:3], SEARCH_RANGE)
        raise SystemExit("the plain call does not raise on the dense table")
    except lk.SubnetOversizeException:
        pass
    t0 = time.perf_counter()
    want_ids, want_rounds = lk.link_levels(dense_levels, SEARCH_RANGE, adaptive_stop=ADAPTIVE_STOP,
                                           adaptive_step=ADAPTIVE_STEP, diag=True)
    host_s = time.perf_counter() - t0
    ms, ids, rounds = time_device(dense_levels, args.reps, plan)
    out['dense'] = dict(levels=len(dense_levels), features=int(len(ids)), adaptive_stop=ADAPTIVE_STOP,
                        adaptive_step=ADAPTIVE_STEP, max_rounds=plan[2], device_ms=ms, host_one_core_ms=host_s * 1e3,
                        largest_round=int(rounds.max()), rows_beyond_round_0=int((rounds > 0).sum()),
                        ids_equal_host=bool(np.array_equal(ids, np.concatenate(want_ids))),
                        rounds_equal_host=bool(np.array_equal(rounds, np.concatenate(want_rounds))))
    print('dense:', json.dumps(out['dense']), file=sys.stderr)
    ms_a, ids_a, rounds_a = time_device(plain_levels, args.reps, plan)
    ms_p, ids_p, _ = time_device(plain_levels, args.reps)
    out['undisturbed_shard'] = dict(adaptive_ms=ms_a, plain_ms=ms_p, ids_equal=bool(np.array_equal(ids_a, ids_p)),
                                    largest_round=int(rounds_a.max()))
    print('undisturbed shard:', json.dumps(out['undisturbed_shard']), file=sys.stderr)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
