"""Time the cluster tracks on the MI355X (ctr_cluster_tracks_device, ctr_track_positions_device;
DESIGN.md 7b) against the host code that the step replaces.

    python tools/cluster_tracks_time.py [--reps 5] [--out profiles/cluster_tracks_time.json]

Workloads (tables only: no frames, no oracle, no reference):
  tetramers: the motion benchmark's 200 tetramer tracks x 1250 frames in 3D (tools/motion_time.py's
    generator, 2 % of the (track, frame) cells missing), 4 rows per cell: about 1 M rows, particle ids
    shuffled, cluster labels restarting in every frame;
  dimers: 1250 frames of 78 dimers in 2D (156 rows per frame, the feature count of a cfg-2 frame) with
    what goes wrong in practice (tests/_cluster_tracks.py: random_video).
Timed per workload, inputs on the device, median / minimum / maximum of `reps` after a warm-up call,
HIP events on a stream of its own around one call (the host's waits inside the call included):
  cluster_tracks_arrays with the round bound queued blind (check_every = 0) and with the host reading
    one word every K rounds (K = 1, 2, 4), the rounds used against the bound;
  track_positions_arrays;
  the upload of the table, apart.
Baselines, wall clock on one core, never the code under test: the rule in vectorised NumPy / SciPy
(tests/_cluster_tracks.py: tracks_vectorised), whose result the device's is compared with, and the
host path inside ``motion.orientation_df(track_column=...)`` (its sort and dense block; the device call
behind it replaced by a stub) on the same table with the ``cluster_track`` column.
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

TRACKS, FRAMES, DIMERS = 200, 1250, 78


def tetramer_table(seed=0):
    from motion_time import tetramers
    pos = tetramers(seed, TRACKS, FRAMES)                      # [tracks, frames, 4, 3], NaN cells
    rng = np.random.RandomState(seed + 1)
    ids = rng.permutation(TRACKS * 4).astype(np.int64).reshape(TRACKS, 4)
    there = ~np.isnan(pos[:, :, 0, 0]).T                       # [frames, tracks]
    off = np.r_[0, np.cumsum(4 * there.sum(1))].astype(np.int64)
    par, clu, xyz = [], [], []
    for f in range(FRAMES):
        tracks = np.flatnonzero(there[f])
        order = rng.permutation(4 * len(tracks))
        par.append(ids[tracks].reshape(-1)[order])
        clu.append(np.repeat(rng.permutation(TRACKS)[:len(tracks)], 4)[order])
        xyz.append(pos[tracks, f].reshape(-1, 3)[order])
    return off, np.concatenate(par), np.concatenate(clu).astype(np.int64), np.concatenate(xyz)


def spread(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), all_ms=[float(x) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import pandas as pd
    import torch
    import _cluster_tracks as yard
    import clustertracking_amd as ct
    from clustertracking_amd import _lib, motion
    ctmod = sys.modules['clustertracking_amd.cluster_tracks']

    _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    own = torch.cuda.Stream(dev)

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(own)
        out = fn()
        b.record(own)
        torch.cuda.synchronize()
        return out, a.elapsed_time(b)

    def timed(fn):
        with torch.cuda.stream(own):
            fn()
            torch.cuda.synchronize()
            runs = [once(fn) for _ in range(args.reps)]
        return runs[-1][0], spread([r[1] for r in runs])

    workloads = dict(tetramers=(tetramer_table(), 4, 1),
                     dimers=(yard.random_video(7, n_frames=FRAMES, n_clusters=DIMERS, cluster_size=2, ndim=2), 2, 3))
    result = dict(method=dict(reps=args.reps, warmup_calls=1,
                              clock='HIP events on a stream of its own around one call, the host\'s waits inside '
                                    'the call included; median, minimum and maximum of reps',
                              inputs='the table on the device, results left there; the upload timed apart',
                              baselines='wall clock, one core, one run'))
    ok = True
    for name, ((off, par, clu, pos), cs, mf) in workloads.items():
        print(name, len(par), 'rows', flush=True)
        P = int(par.max()) + 1
        t0 = time.perf_counter()
        t_off, t_par, t_clu, t_pos = (torch.from_numpy(a).to(dev) for a in (off, par, clu, pos))
        torch.cuda.synchronize()
        upload_ms = (time.perf_counter() - t0) * 1e3
        max_rounds, jumps = ctmod.round_bound(P)
        first = {}
        for k in (0, 1, 2, 4):
            (res, rounds), first['check_every_%d' % k] = timed(lambda: ct.cluster_tracks_arrays(
                t_off, t_par, t_clu, cs, mf, n_particles=P, check_every=k, return_rounds=True))
            first['check_every_%d' % k].update(rounds_used=rounds, status=res.status)
        block, second = timed(lambda: ct.track_positions_arrays(t_pos, t_off, t_par, res.track_of_particle, res.n_tracks, cs))

        t0 = time.perf_counter()
        v_track, v_n, v_pos, v_present = yard.tracks_vectorised(off, par, clu, pos, cs, mf)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        same = (res.status == 0 and res.n_tracks == v_n and np.array_equal(res.track_of_particle.cpu().numpy(), v_track)
                and np.array_equal(block.present.cpu().numpy(), v_present)
                and block.pos.cpu().numpy().tobytes() == v_pos.tobytes())
        ok = ok and same

        columns = ['y', 'x'] if pos.shape[1] == 2 else ['z', 'y', 'x']
        f = pd.DataFrame(pos, columns=columns)
        f['frame'] = np.repeat(np.arange(len(off) - 1), np.diff(off))
        f['particle'], f['cluster'] = par, clu
        f['cluster_track'] = np.where(par >= 0, v_track[np.maximum(par, 0)], -1)
        f = f[f['cluster_track'] >= 0]
        real = motion.orientation_arrays
        motion.orientation_arrays = lambda dense, *a, **k: (np.zeros(dense.shape[:2] + (3,)), np.zeros(1))
        try:
            t0 = time.perf_counter()
            motion.orientation_df(f, cs, ndim=pos.shape[1], track_column='cluster_track',
                                  angles=np.zeros((v_n, 2, len(off) - 1)) if (cs, pos.shape[1]) == (2, 3) else None)
            df_ms = (time.perf_counter() - t0) * 1e3
        finally:
            motion.orientation_arrays = real
        present = block.present.cpu().numpy()
        result[name] = dict(
            workload=dict(rows=int(len(par)), frames=int(len(off) - 1), particles=P, cluster_size=cs, ndim=int(pos.shape[1]),
                          min_frames=mf, n_tracks=int(res.n_tracks), keys=int(len(par) * (cs - 1)),
                          largest_track=int(res.n_members.max().item()) if res.n_tracks else 0,
                          cells_complete=int((present == cs).sum()), cells_conflict=int((present > cs).sum()),
                          cells_incomplete=int((present < cs).sum())),
            round_bound=dict(max_rounds=max_rounds, jumps_per_round=jumps),
            upload_ms=upload_ms,
            cluster_tracks_arrays=first, track_positions_arrays=second,
            host=dict(numpy_vectorised_ms=numpy_ms, orientation_df_host_path_ms=df_ms, equals_device=bool(same)))
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not ok:
        sys.exit('the device and the NumPy form disagree')


if __name__ == '__main__':
    main()
