"""Time the contacts stage on the MI355X (ctr_contacts_device): the whole call, its two
phases and the sort between them apart, against the nearest-neighbour walk on the same table and against
the same rule on one host core.

    python tools/contacts_time.py [--reps 5] [--frames 1250] [--out profiles/contacts_time.json]

Two tables.  ``cfg2``: what ``find_link_arrays`` returns for `--frames` cfg-2 frames (512 x 512 uint8, 200
Gaussians each, diameter 13, separation 13, search range 5) with ``minmass = 0``, so the noise maxima are
rows too: the table of ``tools/twopoint_time.py``; ``r_on = 15``, ``r_off = 18``, ``gap = 2``.  ``tetramers``: 200
tetramer tracks in every one of `--frames` frames -- squares of side 10 around a random walker, every
particle with a localisation noise of 0.3 per axis, every row dropped with 2 %, every frame in a row order
of its own: permanent bonds, chains of `--frames` entries; ``r_on = 11``, ``r_off = 13``, ``gap = 2``.  The table
on the device, ``n_particles`` and ``max_entries`` (the entries of a first call) given, the results left
there: nothing is read back.  HIP events on a stream of its own around one call after a warm-up call,
median / minimum / maximum of `reps`; within the call, events after the entries (the count and fill
walks), after torch's stable sort and its gathers, and after the episodes.  Alternating with it, in the
same process, ``neighbors_arrays(k=1)``: the yardstick of one all-pairs walk over the same frames (the
contacts walk every frame twice).  Next to them, wall clock on one core, one run: a ``cKDTree`` per frame
for the entries, then the run detection (duplicates, chains, first on-entry, lifetimes) vectorised in
NumPy; and the rule restated in ``tests/_contacts.py``, which every output of the device must equal.
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


def spread(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)))


def host_rule(pos, off, par, P, r_on, r_off, gap):
    """the rule on one core: ``(n_entries, n_episodes, sum of the lifetimes)``; a kd-tree per frame (its pairs
    are within ``r_off`` inclusive, the rule's strictly: d2 is compared again), then NumPy"""
    from scipy.spatial import cKDTree
    keys, frames, d2s = [], [], []
    takes = np.isfinite(pos).all(1) & (par >= 0)
    for t in range(len(off) - 1):
        rows = np.arange(off[t], off[t + 1])
        rows = rows[takes[rows]]
        if len(rows) < 2:
            continue
        q, p = pos[rows], par[rows]
        ij = cKDTree(q).query_pairs(r_off, output_type='ndarray')
        d = q[ij[:, 1]] - q[ij[:, 0]]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        a, b = np.minimum(p[ij[:, 0]], p[ij[:, 1]]), np.maximum(p[ij[:, 0]], p[ij[:, 1]])
        keep = (d2 < r_off * r_off) & (a != b)
        keys.append((a * P + b)[keep])
        frames.append(np.full(int(keep.sum()), t, dtype=np.int64))
        d2s.append(d2[keep])
    if not keys:
        return 0, 0, 0
    key, frame, d2 = np.concatenate(keys), np.concatenate(frames), np.concatenate(d2s)
    order = np.argsort(key, kind='stable')
    key, frame, d2 = key[order], frame[order], d2[order]
    n_entries = len(key)
    same = key[1:] == key[:-1]
    first = np.concatenate([[True], ~(same & (frame[1:] == frame[:-1]))])              # not a duplicate
    key, frame, d2 = key[first], frame[first], d2[first]
    head = np.concatenate([[True], (key[1:] != key[:-1]) | (frame[1:] - frame[:-1] > gap + 1)])
    start = np.flatnonzero(head)
    last = np.concatenate([start[1:], [len(key)]]) - 1
    index = np.where(d2 < r_on * r_on, np.arange(len(key)), len(key))
    on = np.minimum.reduceat(index, start)
    has = on <= last
    lifetime = frame[last[has]] - frame[on[has]] + 1
    return n_entries, int(has.sum()), int(lifetime.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import _contacts as yard
    import clustertracking_amd as ct
    from clustertracking_amd import _abi, _lib, workloads

    _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    own = torch.cuda.Stream(dev)

    def measure(name, t_pos, t_off, t_par, P, r_on, r_off, gap):
        with torch.cuda.stream(own):
            first = ct.contacts_arrays(t_pos, t_off, t_par, r_on, r_off, gap, n_particles=P)      # counts the entries: one read
            M = int(first.n_entries)
            marks = {}

            def mark(what):
                marks[what] = torch.cuda.Event(enable_timing=True)
                marks[what].record(own)

            def contacts():
                return ct.contacts_arrays(t_pos, t_off, t_par, r_on, r_off, gap, n_particles=P, max_entries=M, _mark=mark)

            nbr = lambda: ct.neighbors_arrays(t_pos, t_off, k=1)
            res = contacts()                             # the warm-up calls
            nbr()
            torch.cuda.synchronize()
            ms = dict(whole=[], entries=[], sort=[], episodes=[], neighbors=[])
            for _ in range(args.reps):                   # alternating
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(own)
                contacts()
                b.record(own)
                torch.cuda.synchronize()
                ms['whole'].append(a.elapsed_time(b))
                ms['entries'].append(a.elapsed_time(marks['entries']))
                ms['sort'].append(marks['entries'].elapsed_time(marks['sort']))
                ms['episodes'].append(marks['sort'].elapsed_time(marks['episodes']))
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(own)
                nbr()
                b.record(own)
                torch.cuda.synchronize()
                ms['neighbors'].append(a.elapsed_time(b))
        pos, off, par = t_pos.cpu().numpy(), t_off.cpu().numpy(), t_par.cpu().numpy()
        t0 = time.perf_counter()
        host = host_rule(pos, off, par, P, r_on, r_off, gap)
        host_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        want = yard.contacts(pos, off, par, r_on, r_off, gap, n_particles=P)
        yard_ms = (time.perf_counter() - t0) * 1e3
        got = yard.of_tensors(res, M)
        try:
            yard.assert_same(got, want, name)
            same = True
        except AssertionError as e:
            print('the device differs from the restatement:', e, flush=True)
            same = False
        rows = np.diff(off)
        complete = ~(want.left_open | want.right_open)
        out = dict(workload=dict(frames=int(len(off) - 1), rows=int(len(pos)), particles=int(P), r_on=r_on, r_off=r_off, gap=gap,
                                 distance_evaluations_of_one_walk=int((rows ** 2).sum())),
                   contacts_whole_call=spread(ms['whole']), entries_count_and_fill=spread(ms['entries']),
                   sort_and_gathers=spread(ms['sort']), episodes=spread(ms['episodes']), neighbors_k1=spread(ms['neighbors']),
                   host_kdtree_and_runs_ms=host_ms, host_restatement_ms=yard_ms,
                   every_output_equals_the_restatement=same,
                   host_kdtree_counts_agree=bool(host == (want.n_entries, want.n_episodes, int(want.lifetime.sum()))),
                   n_entries=int(want.n_entries), duplicates=int(want.duplicates), n_episodes=int(want.n_episodes),
                   n_pairs=int(want.n_pairs), complete_episodes=int(complete.sum()),
                   longest_lifetime=int(want.lifetime.max()) if want.n_episodes else 0,
                   episodes_of_every_frame=int((want.lifetime == len(off) - 1).sum()),
                   median_lifetime=float(np.median(want.lifetime)) if want.n_episodes else None)
        print(name, out, flush=True)
        return out, same

    frames = workloads.cfg2(n_frames=args.frames)[0]
    print('drawn', flush=True)
    d_frames = torch.from_numpy(frames).to(dev)
    r = ct.find_link_arrays(d_frames, search_range=SEARCH_RANGE, separation=SEPARATION, diameter=DIAMETER, minmass=0,
                            max_queries=1024, max_relocated=1024, _on_device=True)
    del d_frames
    P = int(r.n_tracks.item()) if hasattr(r.n_tracks, 'item') else int(r.n_tracks)
    print('linked', int(r.pos.shape[0]), 'rows', P, 'tracks', flush=True)
    res_a, ok_a = measure('cfg2', r.pos, r.frame_offset, r.particle, P, 15., 18., 2)
    res_a['workload'].update(generator='workloads.cfg2(n_frames=%d), minmass 0' % args.frames, table='find_link_arrays',
                             diameter=DIAMETER, separation=SEPARATION, search_range=SEARCH_RANGE)

    F, K = args.frames, 200
    rng = np.random.RandomState(7)
    centre = rng.uniform(0., 2000., (1, K, 1, 2)) + np.cumsum(rng.normal(0., 0.5, (F, K, 1, 2)), axis=0)
    corners = 5. * np.array([[-1., -1.], [-1., 1.], [1., 1.], [1., -1.]])
    pos = (centre + corners[None, None] + rng.normal(0., 0.3, (F, K, 4, 2))).reshape(F, 4 * K, 2)
    shuffle = np.argsort(rng.uniform(size=(F, 4 * K)), axis=1)
    pos = np.take_along_axis(pos, shuffle[..., None], axis=1).reshape(-1, 2)
    par = shuffle.reshape(-1).astype(np.int64)
    keep = rng.uniform(size=len(pos)) > 0.02
    frame = np.repeat(np.arange(F), 4 * K)[keep]
    t_pos, t_par = torch.from_numpy(pos[keep]).to(dev), torch.from_numpy(par[keep]).to(dev)
    t_off = torch.from_numpy(np.searchsorted(frame, np.arange(F + 1)).astype(np.int64)).to(dev)
    res_b, ok_b = measure('tetramers', t_pos, t_off, t_par, 4 * K, 11., 13., 2)
    res_b['workload'].update(generator='200 squares of side 10 around random walkers (step 0.5), noise 0.3 per axis, 2 % of the '
                                       'rows dropped, shuffled rows')

    out = dict(
        method=dict(reps=args.reps, warmup_calls=1,
                    clock='HIP events on a stream of its own around one call, and after each of its parts; median, minimum and '
                          'maximum of reps; contacts and neighbours alternate in one process',
                    inputs='the table on the device, n_particles and max_entries given, results left there',
                    host='wall clock, one core, one run, the same process: a cKDTree per frame and the run detection in NumPy; '
                         'tests/_contacts.py'),
        cfg2=res_a, tetramers=res_b)
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not (ok_a and ok_b):
        sys.exit('the device and the rule restated in NumPy disagree')


if __name__ == '__main__':
    main()
