"""Time the centre-of-mass refinement on the MI355X (ctr_refine_com_device and
ctr_find_link_refine_device).

    python tools/refine_com_time.py [--reps 5] [--frames 1250] [--out profiles/refine_com_time.json]

Workload: the video of tools/find_link_time.py -- `--frames` frames of 512 x 512 uint8 drawn by
``workloads.cfg2(n_frames=...)``, 10 features per frame dimmed below ``minmass``, diameter 13
(radius 6: a 16-lane row per feature), separation 13, search range 5, ``max_queries`` and
``max_relocated`` 512.
Timed, in one process:
  ``find_link_arrays(refine=True)`` and ``find_link_arrays(refine=False)``, alternating call by
    call after a warm-up call of each (frames on the device, results left there), so that a drift
    of the machine reaches both alike;
  ``refine_com_arrays`` alone on the located rows (positions and offsets on the device);
  the same rule in NumPy (tests/_refine_com.py, one core) on the located rows of the first
    `--host-frames` frames, whose results the device's are compared with.
Device time: HIP events on a stream of its own around one call; median, minimum and maximum of
`reps`.  The events bracket the host's waits inside a call too (the location's), so this is the
time of the call as a user sees it.  ``refine=False`` queues the kernels of ``ctr_find_link_device``
as before: its range is what a run of tools/find_link_time.py at the commit before is compared
with (``--parent-json``: that run's file, copied into the output).
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

PER_FRAME, DIM_TO = 10, 0.3
DIAMETER, SEPARATION, SEARCH_RANGE = 13, 13, 5
MAX_QUERIES = MAX_RELOCATED = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--host-frames', type=int, default=4)
    ap.add_argument('--parent-json', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import _refine_com as RC
    import clustertracking_amd as ct
    from clustertracking_amd import _lib, workloads
    from clustertracking_amd.find import _characterize_device, locate_arrays

    _lib.default_engine(0)      # EngineError without a library or a GPU: nothing is timed on a CPU
    dev = torch.device('cuda', 0)
    F = args.frames
    frames, _, truth, _ = workloads.cfg2(n_frames=F)
    print('drawn', flush=True)
    rng = np.random.RandomState(0)
    truth = truth.reshape(F, -1, 2)
    r = DIAMETER // 2 + 2
    for f in range(F):      # as tools/find_link_time.py
        for y, x in np.round(truth[f, rng.choice(truth.shape[1], PER_FRAME, replace=False)]).astype(int):
            win = frames[f, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1]
            win[...] = np.round(win * DIM_TO).astype(np.uint8)
    first = ct.locate(frames[:1], SEPARATION, DIAMETER)
    minmass = 0.5 * float(np.median(np.sort(first['mass'].values)[-200:]))
    d_frames = torch.from_numpy(frames).to(dev)
    kw = dict(search_range=SEARCH_RANGE, separation=SEPARATION, diameter=DIAMETER, memory=0, minmass=minmass,
              max_queries=MAX_QUERIES, max_relocated=MAX_RELOCATED, _on_device=True)
    radius = (DIAMETER // 2,) * 2
    own = torch.cuda.Stream(dev)     # see tools/characterize_time.py

    # the located rows, as find_link_arrays selects them
    t, pix, pos, off, _ = locate_arrays(d_frames, SEPARATION, 64, radius, _on_device=True)
    mass, _, _ = _characterize_device(t, pos, off, radius, True, 1., 0, pix)
    rows = torch.nonzero(mass >= minmass).reshape(-1)
    frame_of = torch.repeat_interleave(torch.arange(F, device=dev), off[1:] - off[:-1], output_size=int(pos.shape[0]))
    loc_off = torch.zeros(F + 1, dtype=torch.int64, device=dev)
    loc_off[1:] = torch.cumsum(torch.bincount(frame_of.index_select(0, rows), minlength=F), 0)
    loc_pos = pos.index_select(0, rows).to(torch.float64)

    calls = dict(
        refine_true=lambda: ct.find_link_arrays(d_frames, refine=True, **kw),
        refine_false=lambda: ct.find_link_arrays(d_frames, refine=False, **kw),
        stand_alone=lambda: ct.refine_com_arrays(d_frames, loc_pos, loc_off, radius, _on_device=True))

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(own)
        out = fn()
        b.record(own)
        torch.cuda.synchronize()
        return out, a.elapsed_time(b)

    ms = {k: [] for k in calls}
    out = {}
    with torch.cuda.stream(own):
        for k, fn in calls.items():      # warm-up: the same shapes as the timed passes
            fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):       # alternating
            for k in ('refine_true', 'refine_false'):
                out[k], t_ms = once(calls[k])
                ms[k].append(t_ms)
        print('find_link timed', flush=True)
        for _ in range(args.reps):
            out['stand_alone'], t_ms = once(calls['stand_alone'])
            ms['stand_alone'].append(t_ms)
    stats = {k: dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), all_ms=[float(x) for x in v])
             for k, v in ms.items()}
    res_t, res_f = out['refine_true'], out['refine_false']
    sa_pos, sa_mass, sa_iter = (x.cpu().numpy() for x in out['stand_alone'])

    HF = min(args.host_frames, F)
    h_off = loc_off[:HF + 1].cpu().numpy()
    h_pos = loc_pos[:int(h_off[-1])].cpu().numpy()
    t0 = time.perf_counter()
    host = RC.compose(frames[:HF], h_pos, h_off, radius)
    host_ms = (time.perf_counter() - t0) * 1e3
    n_head = len(h_pos)
    same = (np.array_equal(host['pos'], sa_pos[:n_head]) and np.array_equal(host['mass'], sa_mass[:n_head])
            and np.array_equal(host['n_iter'], sa_iter[:n_head]))
    n = int(loc_pos.shape[0])
    result = dict(
        workload=dict(generator='workloads.cfg2(n_frames=%d), %d features per frame dimmed to %.1f' % (F, PER_FRAME, DIM_TO),
                      frames=F, shape=list(frames.shape[1:]), dtype=str(frames.dtype), diameter=DIAMETER, radius=list(radius),
                      separation=SEPARATION, search_range=SEARCH_RANGE, memory=0, minmass=minmass,
                      max_queries=MAX_QUERIES, max_relocated=MAX_RELOCATED, located_rows=n, located_rows_per_frame=n / F,
                      max_iterations=10, shift_thresh=0.6),
        method=dict(reps=args.reps, warmup_passes=1, order='refine=True and refine=False alternate call by call',
                    clock="HIP events on a stream of its own around one call, the host's waits inside the call "
                          "included; median, minimum and maximum of reps",
                    inputs='frames on the device, results left there'),
        device=dict(find_link_refine_true=stats['refine_true'], find_link_refine_false=stats['refine_false'],
                    refine_com_arrays_on_located_rows=stats['stand_alone'],
                    refine_true_minus_false_ms=stats['refine_true']['median_ms'] - stats['refine_false']['median_ms'],
                    refine_true_minus_false_us_per_level=1e3 * (stats['refine_true']['median_ms']
                                                                - stats['refine_false']['median_ms']) / F,
                    stand_alone_ns_per_row=1e6 * stats['stand_alone']['median_ms'] / max(n, 1),
                    stand_alone_windows=int(sa_iter.sum()), stand_alone_rows_that_walk=int((sa_iter >= 2).sum()),
                    rows=dict(refine_true=int(res_t.pos.shape[0]), refine_false=int(res_f.pos.shape[0])),
                    tracks=dict(refine_true=int(res_t.n_tracks.item()), refine_false=int(res_f.n_tracks.item())),
                    relocated_rows=dict(refine_true=int(res_t.relocated.sum().item()),
                                        refine_false=int(res_f.relocated.sum().item()))),
        host_restatement=dict(frames=HF, rows=n_head, ms=host_ms, ms_per_frame=host_ms / HF,
                              us_per_row=1e3 * host_ms / max(n_head, 1), equals_device=bool(same)),
    )
    if args.parent_json:
        with open(args.parent_json) as fh:
            parent = json.load(fh)
        result['parent_commit'] = dict(tool='tools/find_link_time.py at the commit before, same machine and day',
                                       find_link_arrays=parent['device']['find_link_arrays'])
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not same:
        sys.exit('the device and the restatement disagree')


if __name__ == '__main__':
    main()
