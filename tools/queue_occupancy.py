"""Reduce a rocprofv3 kernel trace (``--kernel-trace --output-format csv``: *_kernel_trace.csv) of
``bench.py`` to a summary of a few KB: which hardware queues carried the engine's kernels, how
busy each was, and how long every step took on the device.

    python tools/queue_occupancy.py TRACE.csv --calls 133:153 -o profiles/r05_queue_occupancy.json

A *call* is one ``ctr_refine_batch_device``: the dispatches from the first of its head (the fill
right before ``frame_max_kernel``) up to the next call's, in dispatch order (the host queues a call
completely before the next one).  ``--calls A:B``
keeps the calls A <= i < B, e.g. the timed steps of ``bench.py --steps 20 --warmup 3`` with ten
batches in flight: 10 set-up calls + 4 x 30 of the layout trial + 3 warm-up = 133 before them.

Per queue: dispatches by kernel, busy time (union of the kernels' intervals), idle time inside
the window, and the longest gaps with the kernel that was running elsewhere meanwhile.  Per call:
first start to last end, and ``gap_before_call``: how long the queue on which the call begins had
been without a refine kernel when it began.  Times in milliseconds.
"""
import argparse
import csv
import json
import re
from collections import Counter, defaultdict


def short(name):
    """'refine_block_kernel<2,true,1,2,...>' from the demangled name"""
    name = re.sub(r'\(anonymous namespace\)::', '', name)
    name = re.sub(r'^void ', '', name)
    m = re.match(r'([A-Za-z_0-9:]+)(<[^>]*>)?', name)
    base = m.group(1) if m else name
    targs = (m.group(2) or '') if m else ''
    return base + targs.replace(' ', '')


def union_ms(intervals):
    busy, end = 0, None
    for a, b in sorted(intervals):
        if end is None or a > end:
            busy += b - a
            end = b
        elif b > end:
            busy += b - end
            end = b
    return busy / 1e6


def summarise(rows, calls=None, top_gaps=3):
    rows = sorted(rows, key=lambda r: r['dispatch'])
    # a call begins with the first dispatch of its head: the fill (memset of the encoded maxima)
    # that the runtime dispatches on the same stream right before frame_max_kernel, if there is one
    call = -1
    for i, r in enumerate(rows):
        nxt = rows[i + 1] if i + 1 < len(rows) else None
        fill_of_head = (r['name'].startswith('__amd_rocclr_fill') and nxt is not None and
                        nxt['name'].startswith('frame_max_kernel') and nxt['stream'] == r['stream'])
        if fill_of_head or (r['name'].startswith('frame_max_kernel') and not r.get('head_begun')):
            call += 1
            if fill_of_head:
                nxt['head_begun'] = True
        r['call'] = call
        r['first_of_call'] = fill_of_head or (r['name'].startswith('frame_max_kernel') and not r.get('head_begun'))
    n_calls = call + 1
    lo, hi = calls if calls else (0, n_calls)
    kept = [r for r in rows if lo <= r['call'] < hi]
    if not kept:
        raise SystemExit("no dispatch in calls %d:%d (the trace has %d calls)" % (lo, hi, n_calls))
    t0 = min(r['start'] for r in kept)
    t1 = max(r['end'] for r in kept)
    queues = defaultdict(list)
    for r in kept:
        queues[r['queue']].append(r)
    out_q = {}
    for q, rs in sorted(queues.items()):
        rs.sort(key=lambda r: r['start'])
        busy = union_ms([(r['start'], r['end']) for r in rs])
        gaps = []
        end = t0
        for r in rs:
            if r['start'] > end:
                # what ran elsewhere during most of the gap
                mid = (end + r['start']) // 2
                others = [o for o in kept if o['queue'] != q and o['start'] <= mid < o['end']]
                longest = max(others, key=lambda o: o['end'] - o['start'])['name'] if others else None
                gaps.append({"ms": (r['start'] - end) / 1e6, "before": r['name'], "running_elsewhere": longest})
            end = max(end, r['end'])
        gaps.sort(key=lambda g: -g['ms'])
        out_q[str(q)] = {
            "dispatches": len(rs),
            "streams": sorted({r['stream'] for r in rs}),
            "kernels": dict(Counter(r['name'] for r in rs).most_common()),
            "kernel_ms": {k: round(sum((r['end'] - r['start']) for r in rs if r['name'] == k) / 1e6, 3)
                          for k in sorted({r['name'] for r in rs})},
            "busy_ms": round(busy, 3),
            "idle_ms": round((t1 - t0) / 1e6 - busy, 3),
            "longest_gaps": [dict(g, ms=round(g['ms'], 3)) for g in gaps[:top_gaps]],
        }
    per_call = []
    for c in range(lo, hi):
        rs = [r for r in kept if r['call'] == c]
        if rs:
            per_call.append({"call": c, "start_ms": round((min(r['start'] for r in rs) - t0) / 1e6, 3),
                             "first_start_to_last_end_ms": round((max(r['end'] for r in rs) - min(r['start'] for r in rs)) / 1e6, 3),
                             "queues": sorted({r['queue'] for r in rs})})
    # On the queue on which a call begins: from the end of the last refine kernel of an earlier call
    # there (or of whatever ran there last, if no refine kernel did) to the call's first dispatch,
    # and the longest kernel that was running on another queue in the middle of that gap.
    head_gaps = []
    for r in kept:
        if not r['first_of_call']:
            continue
        before = [o for o in kept if o['queue'] == r['queue'] and o['end'] <= r['start'] and o['call'] < r['call']]
        refine = [o for o in before if o['name'].startswith('refine_')]
        if not before:
            continue
        prev = max(refine or before, key=lambda o: o['end'])
        busy_between = union_ms([(max(o['start'], prev['end']), o['end']) for o in before if o['end'] > prev['end']])
        mid = (prev['end'] + r['start']) // 2
        others = [o for o in kept if o['queue'] != r['queue'] and o['start'] <= mid < o['end']]
        longest = max(others, key=lambda o: o['end'] - o['start'])['name'] if others else None
        head_gaps.append({"call": r['call'], "queue": r['queue'], "after": prev['name'],
                          "gap_ms": round((r['start'] - prev['end']) / 1e6, 3),
                          "queue_busy_in_gap_ms": round(busy_between, 3), "running_elsewhere": longest})
    dur = defaultdict(list)
    for r in kept:
        dur[r['name']].append((r['end'] - r['start']) / 1e6)
    return {
        "calls_in_trace": n_calls, "calls": [lo, hi], "window_ms": round((t1 - t0) / 1e6, 3),
        "ms_per_call": round((t1 - t0) / 1e6 / max(1, hi - lo), 4),
        "queues_with_engine_kernels": len(out_q),
        "queues": out_q,
        "kernel_duration_ms": {k: {"n": len(v), "mean": round(sum(v) / len(v), 4), "max": round(max(v), 4)}
                               for k, v in sorted(dur.items())},
        "per_call": per_call,
        "gap_before_call": head_gaps,
    }


def read_trace(path):
    rows = []
    with open(path, newline='') as f:
        for r in csv.DictReader(f):
            if r.get('Kind', 'KERNEL_DISPATCH') != 'KERNEL_DISPATCH':
                continue
            rows.append({"queue": int(r['Queue_Id']), "stream": int(r.get('Stream_Id') or 0),
                         "dispatch": int(r['Dispatch_Id']), "name": short(r['Kernel_Name']),
                         "start": int(r['Start_Timestamp']), "end": int(r['End_Timestamp'])})
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('trace')
    ap.add_argument('--calls', default=None, help="A:B, the calls to keep (default: all)")
    ap.add_argument('-o', '--output', default=None)
    ap.add_argument('--note', default=None, help="free text stored with the summary (command, environment)")
    args = ap.parse_args()
    calls = tuple(int(x) for x in args.calls.split(':')) if args.calls else None
    out = summarise(read_trace(args.trace), calls)
    out["trace"] = args.trace.split('/')[-1]
    if args.note:
        out["note"] = args.note
    text = json.dumps(out, indent=1)
    if args.output:
        with open(args.output, 'w') as f:
            f.write(text + '\n')
    else:
        print(text)


if __name__ == '__main__':
    main()
