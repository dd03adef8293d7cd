"""Time bench.py's workload for several values of ctr_set_tail_absorb: the most
clusters of a 3-4- or 5-10-feature bin that the tail launch of a throughput plan fits whole.

    python tools/tail_absorb_sweep.py --max-count 0 256 512 1024 2048 --repeat 2 \
        -o profiles/tail_absorb_sweep.json -- --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline
    python tools/tail_absorb_sweep.py --features 320 --max-count 0 2048 8192 ...   # a denser cfg 2

Every run is bench.py itself in a process of its own, whose engine handles get the value right
after they are made; the values alternate (0 256 ... 0 256 ...), so that drift of the machine shows
as spread inside a value and not as a difference between values.  With -o the runs are added to
the file under the key of the batch ('cfg2' or 'cfg2_features_<N>').
"""
import argparse
import functools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP = ('ms_per_step', 'value')


def child(max_count, features, bench_args):
    sys.path.insert(0, ROOT)
    from clustertracking_amd import _lib, workloads
    make = _lib.Engine.__init__

    def make_and_set(self, *a, **kw):
        make(self, *a, **kw)
        self.set_tail_absorb(max_count)

    _lib.Engine.__init__ = make_and_set
    if features:
        workloads.cfg2 = functools.partial(workloads.cfg2, n_features=features)
    import bench
    sys.argv = ['bench.py'] + bench_args
    bench.main()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--max-count', type=int, nargs='+', default=[])
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--features', type=int, default=None, help='features per frame of cfg 2 (its own: 200)')
    ap.add_argument('--timeout', type=int, default=240, help='seconds per run')
    ap.add_argument('--child', type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument('-o', '--output', default=None)
    ap.add_argument('bench_args', nargs=argparse.REMAINDER)
    args = ap.parse_args()
    bench_args = [a for a in args.bench_args if a != '--']
    if args.child is not None:
        return child(args.child, args.features, bench_args)
    if not args.max_count:
        ap.error('--max-count: at least one value')
    key ='cfg2' if not args.features else 'cfg2_features_%d' % args.features
    runs = []
    for rep in range(args.repeat):
        for n in args.max_count:
            cmd = [sys.executable, os.path.abspath(__file__), '--child', str(n)]
            if args.features:
                cmd += ['--features', str(args.features)]
            out = subprocess.run(cmd + ['--'] + bench_args, stdout=subprocess.PIPE, timeout=args.timeout, check=True)
            line = json.loads(out.stdout.decode().strip().splitlines()[-1])
            run = dict(max_count=n, repeat=rep, clusters=line.get('config', {}).get('cluster_fits_per_gpu'))
            run.update({k: line.get(k) for k in KEEP})
            run['in_flight_results_identical'] = line.get('in_flight_results_identical')
            runs.append(run)
            print(json.dumps(run), flush=True)
    if args.output:
        doc = {}
        if os.path.exists(args.output):
            with open(args.output) as f:
                doc = json.load(f)
        doc[key] = dict(bench_args=bench_args, runs=runs)
        with open(args.output, 'w') as f:
            json.dump(doc, f, indent=1)


if __name__ == '__main__':
    main()
