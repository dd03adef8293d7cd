"""Time linking with prediction on the MI355X (ctr_link_predict_device).

    python tools/link_predict_time.py [--parent-tree DIR] [--runs 5] [--reps 20] [--out FILE]

The workload is the cfg-4 shard (1250 levels x 200 walkers in 512^2, steps 0.5 px, search_range 3).
One fresh process per run and tree, this tree and a built checkout of the parent commit
(``--parent-tree``; without it only this tree) alternating, ``--runs`` each; inside a process the
calls alternate too, in blocks of ``--reps`` / 4.  Median and range over the processes.
1. The paths that exist must not pay for the feature: ``ctr_link_device`` with memory 0 (one launch
   per kernel) and memory 1 (level by level) on both trees.  The bar is the parent's own range.
2. Both predictors (memory 1) on the shard, beside the parent's memory-1 call, whose launch
   structure they share: one more launch per level, nothing else.
3. The shard with a drift of 2 x search_range per level added along x, which the plain call cannot
   link (what it links are rows that land where another row was: ``n_tracks`` shows it): both
   predictors with that drift as ``initial_velocity``, ids and velocities compared with the host
   linker's.
Device time: HIP events around the calls after warm-up, positions and offsets already on the device,
outputs preallocated (as tools/link_time.py).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCH_RANGE = 3.
DRIFT = (0., 2. * SEARCH_RANGE)
PARENT_CALLS = ('plain_memory0', 'plain_memory1')
CALLS = PARENT_CALLS + ('velocity', 'drift', 'velocity_drifting', 'drift_drifting', 'plain_drifting')


def shard(drifting):
    rng = np.random.RandomState(4)
    pos = rng.uniform(0, 512, (200, 2))
    levels = []
    for t in range(1250):
        pos = pos + rng.normal(0, 0.5, pos.shape)
        lvl = pos + t * np.asarray(DRIFT) if drifting else pos
        levels.append(lvl[rng.permutation(len(lvl))].copy())
    return levels


class Call:
    """one descriptor with its buffers on the device, ready to be queued again and again"""

    def __init__(self, name, tables):
        import torch
        from clustertracking_amd import _abi, _lib
        eng = _lib.default_engine(0)
        self.name = name
        drifting = name.endswith('_drifting')
        self.pos, self.off = tables[drifting]
        n = int(self.pos.shape[0])
        dev = self.pos.device
        self.particle = torch.empty(n, dtype=torch.int64, device=dev)
        self.velocity = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        self.n_tracks = torch.empty(1, dtype=torch.int64, device=dev)
        self.status = torch.empty(4, dtype=torch.int32, device=dev)
        predictor = name.split('_')[0] if not name.startswith('plain') else None
        d = _abi.Link() if predictor is None else _abi.LinkPredict()
        d.ndim, d.n_levels, d.n_features = 2, int(self.off.numel()) - 1, n
        d.memory = 0 if name == 'plain_memory0' else 1
        d.search_range[0] = d.search_range[1] = SEARCH_RANGE
        d.pos, d.frame_offset = self.pos.data_ptr(), self.off.data_ptr()
        d.particle, d.n_tracks, d.status = self.particle.data_ptr(), self.n_tracks.data_ptr(), self.status.data_ptr()
        self.entry = eng.link_device
        if predictor is not None:
            d.predictor = dict(velocity=_abi.LINK_PREDICT_VELOCITY, drift=_abi.LINK_PREDICT_DRIFT)[predictor]
            if drifting:
                d.initial_velocity[0], d.initial_velocity[1] = DRIFT
            d.velocity = self.velocity.data_ptr()
            self.entry = eng.link_predict_device
        self.d = d
        self.ms = []

    def queue(self, stream):
        self.entry(self.d, stream.cuda_stream)


def child(names, reps, dump):
    import torch
    dev = torch.device('cuda', 0)
    tables = {}
    for drifting in {n.endswith('_drifting') for n in names}:
        levels = shard(drifting)
        offs = np.r_[0, np.cumsum([len(l) for l in levels])].astype(np.int64)
        tables[drifting] = (torch.from_numpy(np.concatenate(levels)).to(dev), torch.from_numpy(offs).to(dev))
    calls = [Call(n, tables) for n in names]
    own = torch.cuda.Stream(dev)
    for c in calls:
        for _ in range(3):
            c.queue(own)
    torch.cuda.synchronize(dev)
    blocks, per_block = 4, max(reps // 4, 1)
    for _ in range(blocks):
        for c in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(own)
            for _ in range(per_block):
                c.queue(own)
            b.record(own)
            torch.cuda.synchronize(dev)
            c.ms.append(a.elapsed_time(b) / per_block)
    out = {}
    for c in calls:
        assert int(c.status[0].item()) == 0, (c.name, c.status.tolist())
        out[c.name] = dict(call_ms=float(np.mean(c.ms)), n_tracks=int(c.n_tracks.item()))
        if dump:
            np.savez(os.path.join(dump, c.name + '.npz'), ids=c.particle.cpu().numpy(), velocity=c.velocity.cpu().numpy())
    print(json.dumps(out))


def run_child(tree, names, reps, dump=None):
    env = dict(os.environ, PYTHONPATH=tree)
    env.pop('CTREFINE_LIB', None)
    cmd = [sys.executable, os.path.abspath(__file__), '--child', ','.join(names), '--tree', tree, '--reps', str(reps)]
    if dump:
        cmd += ['--dump', dump]
    out = subprocess.run(cmd, env=env, cwd=tree, stdout=subprocess.PIPE, universal_newlines=True, timeout=600,
                         check=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def spread(values):
    return dict(median=float(np.median(values)), min=float(min(values)), max=float(max(values)), runs=[float(v) for v in values])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument('--dump', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    sys.path.insert(0, args.tree)
    if args.child:
        return child(args.child.split(','), args.reps, args.dump)

    import tempfile
    import time
    trees = [('this', ROOT, CALLS)] + ([('parent', os.path.abspath(args.parent_tree), PARENT_CALLS)] if args.parent_tree else [])
    ms = {name: {c: [] for c in calls} for name, _, calls in trees}
    tracks = {}
    with tempfile.TemporaryDirectory() as dump:
        for r in range(args.runs):
            for name, tree, calls in trees:
                res = run_child(tree, calls, args.reps, dump if (name == 'this' and r == 0) else None)
                for c in calls:
                    ms[name][c].append(res[c]['call_ms'])
                    tracks.setdefault(c, res[c]['n_tracks'])
                    assert tracks[c] == res[c]['n_tracks'], (c, name, tracks[c], res[c]['n_tracks'])
                print('run %d, %s: %s' % (r, name, ', '.join('%s %.4f ms' % (c, res[c]['call_ms']) for c in calls)), file=sys.stderr)
        got = {c: dict(np.load(os.path.join(dump, c + '.npz'))) for c in CALLS}
    out = dict(levels=1250, features_per_level=200, search_range=SEARCH_RANGE, drift_per_level=list(DRIFT),
               runs=args.runs, reps=args.reps)
    out['call_ms'] = {name: {c: spread(v) for c, v in per.items()} for name, per in ms.items()}
    out['n_tracks'] = tracks
    if args.parent_tree:
        for c in PARENT_CALLS:
            p, t = out['call_ms']['parent'][c], out['call_ms']['this'][c]
            out['call_ms']['this'][c]['median_within_parent_range'] = bool(t['median'] <= p['max'])

    from clustertracking_amd import link as lk
    # the plain call on the drifting shard: all it links are rows that land where another row was
    assert tracks['plain_drifting'] > 100 * tracks['plain_memory1'], "the plain call links the drifting shard"
    host = {}
    for drifting in (False, True):
        levels = shard(drifting)
        for predictor in ('velocity', 'drift'):
            name = predictor + ('_drifting' if drifting else '')
            t0 = time.perf_counter()
            ids, vel = lk.link_levels(levels, SEARCH_RANGE, 1, predictor=predictor, initial_velocity=DRIFT if drifting else None,
                                      want_velocity=True)
            host[name] = dict(host_one_core_ms=(time.perf_counter() - t0) * 1e3,
                              ids_equal_host=bool(np.array_equal(got[name]['ids'], np.concatenate(ids))),
                              velocity_equal_host=bool(np.array_equal(got[name]['velocity'], np.concatenate(vel))))
    out['against_host'] = host
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
