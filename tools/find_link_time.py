"""Time find and link with relocation on the MI355X (ctr_find_link_device).

    python tools/find_link_time.py [--reps 5] [--frames 1250] [--out profiles/find_link_time.json]

Workload: the video of tools/relocate_time.py -- `--frames` frames of 512 x 512 uint8 drawn by
``workloads.cfg2(n_frames=...)`` with 200 Gaussians each, diameter 13, separation 13, search range
5 -- in which 10 features per frame are dimmed to 0.3 of their brightness, below ``minmass`` (half
the median mass of the 200 brightest located rows of frame 0, which also cuts the noise maxima).
cfg 2 draws every frame from a seed of its own: its features do not persist, so nearly every source
is lost, nearly every sub-network of a level looks again, and few candidates are claimed -- the
relocation runs at about the level's feature count, not at 10 queries.  ``max_queries`` and
``max_relocated`` are 512 for that.
Timed: ``find_link_arrays`` (frames on the device, results left there), and on the same block
``locate_arrays`` + characterize + ``link_arrays``, the chain without relocation.  Device time: HIP
events on a stream of its own around one call, after a warm-up call; the median of `reps`.  The
events bracket the host's waits inside a call too (the location's), so this is the time of the
call as a user sees it; the wall clock is recorded next to it.  Host synchronisations per call are
counted by wrapping what waits (torch.cuda.synchronize, Tensor.cpu / .item, torch.nonzero).
Host time: wall clock of tests/_find_link.py (NumPy, one core) on the first `--host-frames` frames.
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
RELOCATE_US_PER_CALL = 207.      # profiles/relocate_time.json: one call of 10 queries per frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=1250)
    ap.add_argument('--host-frames', type=int, default=4)
    ap.add_argument('--memory', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import torch
    import _find_link as R
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
    for f in range(F):
        for y, x in np.round(truth[f, rng.choice(truth.shape[1], PER_FRAME, replace=False)]).astype(int):
            win = frames[f, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1]
            win[...] = np.round(win * DIM_TO).astype(np.uint8)
    first = ct.locate(frames[:1], SEPARATION, DIAMETER)
    minmass = 0.5 * float(np.median(np.sort(first['mass'].values)[-200:]))
    d_frames = torch.from_numpy(frames).to(dev)
    kw = dict(search_range=SEARCH_RANGE, separation=SEPARATION, diameter=DIAMETER, memory=args.memory, minmass=minmass)
    own = torch.cuda.Stream(dev)     # see tools/characterize_time.py

    def with_relocation():
        return ct.find_link_arrays(d_frames, max_queries=MAX_QUERIES, max_relocated=MAX_RELOCATED, _on_device=True, **kw)

    def without_relocation():
        t, pix, pos, off, _ = locate_arrays(d_frames, SEPARATION, 64, (DIAMETER // 2,) * 2, _on_device=True)
        mass, _, _ = _characterize_device(t, pos, off, (DIAMETER // 2,) * 2, True, 1., 0, pix)
        rows = torch.nonzero(mass >= minmass).reshape(-1)
        frame_of = torch.repeat_interleave(torch.arange(F, device=dev), off[1:] - off[:-1], output_size=int(pos.shape[0]))
        loc_off = torch.zeros(F + 1, dtype=torch.int64, device=dev)
        loc_off[1:] = torch.cumsum(torch.bincount(frame_of.index_select(0, rows), minlength=F), 0)
        return ct.link_arrays(pos.index_select(0, rows).to(torch.float64), loc_off, SEARCH_RANGE, args.memory, _on_device=True)

    waits = [0]

    def counting(fn):
        def wrapped(*a, **k):
            waits[0] += 1
            return fn(*a, **k)
        return wrapped

    def timed(fn):
        with torch.cuda.stream(own):
            out = fn()                                # warm-up: the same shapes as the timed passes
            torch.cuda.synchronize()
            ms, wall = [], []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record(own)
                fn()
                b.record(own)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(a.elapsed_time(b))
            saved = torch.cuda.synchronize, torch.Tensor.cpu, torch.Tensor.item, torch.nonzero
            torch.cuda.synchronize, torch.Tensor.cpu = counting(saved[0]), counting(saved[1])
            torch.Tensor.item, torch.nonzero = counting(saved[2]), counting(saved[3])
            waits[0] = 0
            try:
                fn()
            finally:
                torch.cuda.synchronize, torch.Tensor.cpu, torch.Tensor.item, torch.nonzero = saved
            n_waits = waits[0]
            torch.cuda.synchronize()
        return out, dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)),
                         host_wall_median_ms=float(np.median(wall)), host_synchronisations=n_waits)

    res, t_fl = timed(with_relocation)
    print('find_link timed', flush=True)
    ids, t_ll = timed(without_relocation)
    n_rows = int(res.pos.shape[0])
    n_reloc = int(res.relocated.sum().item())
    HF = min(args.host_frames, F)
    t0 = time.perf_counter()
    log = []
    host = R.find_link(frames[:HF], log=log, **kw)
    host_ms = (time.perf_counter() - t0) * 1e3
    off = res.frame_offset.cpu().numpy()
    n_head = int(off[HF])
    same = (len(host['pos']) == n_head and np.array_equal(host['pos'], res.pos[:n_head].cpu().numpy())
            and np.array_equal(host['particle'], res.particle[:n_head].cpu().numpy()))
    out = dict(
        workload=dict(generator='workloads.cfg2(n_frames=%d), %d features per frame dimmed to %.1f' % (F, PER_FRAME, DIM_TO),
                      frames=F, shape=list(frames.shape[1:]), dtype=str(frames.dtype), diameter=DIAMETER,
                      separation=SEPARATION, search_range=SEARCH_RANGE, memory=args.memory, minmass=minmass,
                      max_queries=MAX_QUERIES, max_relocated=MAX_RELOCATED, rows=n_rows, rows_per_frame=n_rows / F,
                      tracks=int(res.n_tracks.item())),
        method=dict(reps=args.reps, warmup_passes=1, clock='HIP events on a stream of its own around one call, the '
                    "host's waits inside the call included; median of reps", inputs='frames on the device, results left there'),
        device=dict(find_link_arrays=t_fl, locate_characterize_link_arrays=t_ll,
                    find_link_ms_per_frame=t_fl['median_ms'] / F, locate_link_ms_per_frame=t_ll['median_ms'] / F,
                    relocation_and_loop_ms_per_level=(t_fl['median_ms'] - t_ll['median_ms']) / max(F - 1, 1),
                    relocate_call_of_10_queries_us=RELOCATE_US_PER_CALL,
                    relocated_rows=n_reloc, coupled_levels=int(res.coupled.sum().item()),
                    host_synchronisations_inside_the_loop=0),
        host_restatement=dict(frames=HF, ms=host_ms, ms_per_frame=host_ms / HF, queries=len(log),
                              relocated_rows=int(host['relocated'].sum()), equals_device=bool(same)),
    )
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    if not same:
        sys.exit('the device and the restatement disagree')


if __name__ == '__main__':
    main()
