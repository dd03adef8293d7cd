"""The drift rule (include/ctrefine.h) restated with plain loops: the yardstick of the
device path.  No engine, no oracle.  Every mean is ``math.fsum(...) / n``: the correctly rounded sum,
divided once.  Also the generators of the test tables and the bound of ``drift``."""
import collections
import math

import numpy as np

Drift = collections.namedtuple('Drift', ['drift', 'n_pairs', 'dx', 'pairs'])
Stubs = collections.namedtuple('Stubs', ['particle', 'count'])


def _mean(values, ndim):
    """the mean of a list of [ndim] vectors per coordinate, or None of an empty list"""
    if not values:
        return None
    return np.array([math.fsum(v[d] for v in values) / len(values) for d in range(ndim)])


def compute_drift(pos, frame_offset, particle, smoothing=0):
    pos = np.asarray(pos, dtype=np.float64)
    off = np.asarray(frame_offset, dtype=np.int64)
    particle = np.asarray(particle, dtype=np.int64)
    T, ndim = len(off) - 1, pos.shape[1]
    n_pairs = np.zeros(T, dtype=np.int32)
    dx = np.zeros((T, ndim))
    pairs = []                                   # (t, i, j) of every pair
    for t in range(1, T):
        lowest = {}                              # clause 1: the lowest row of frame t - 1 with an id
        for j in range(off[t - 1], off[t]):
            if particle[j] >= 0:
                lowest.setdefault(int(particle[j]), j)
        steps = []
        for i in range(off[t], off[t + 1]):      # every row of frame t that has a match counts
            j = lowest.get(int(particle[i])) if particle[i] >= 0 else None
            if j is not None:
                steps.append(pos[i] - pos[j])
                pairs.append((t, i, j))
        n_pairs[t] = len(steps)                  # clause 2
        if steps:
            dx[t] = _mean(steps, ndim)
    sm = np.zeros((T, ndim))                     # clause 3
    for t in range(1, T):
        if smoothing <= 1:
            window = [t]
        else:
            window = range(max(1, t - smoothing + 1), t + 1)
        m = _mean([dx[u] for u in window if n_pairs[u] > 0], ndim)
        if m is not None:
            sm[t] = m
    drift = np.zeros((T, ndim))                  # clause 4
    for t in range(1, T):
        drift[t] = drift[t - 1] + sm[t]
    return Drift(drift, n_pairs, dx, pairs)


def frame_of(frame_offset, n):
    off = np.asarray(frame_offset, dtype=np.int64)
    out = np.empty(n, dtype=np.int64)
    for t in range(len(off) - 1):
        out[off[t]:off[t + 1]] = t
    return out


def subtract_drift(pos, frame_offset, drift):
    """clause 5"""
    pos = np.asarray(pos, dtype=np.float64)
    return pos - np.asarray(drift)[frame_of(frame_offset, len(pos))]


def filter_stubs(particle, threshold, n_particles=None):
    """clause 6"""
    particle = np.asarray(particle, dtype=np.int64)
    P = int(n_particles) if n_particles is not None else (max(int(particle.max()) + 1, 0) if len(particle) else 0)
    count = np.zeros(P, dtype=np.int32)
    for p in particle:
        if p >= 0:
            count[p] += 1
    out = np.array([p if p >= 0 and count[p] >= threshold else -1 for p in particle], dtype=np.int64)
    return Stubs(out, count)


def bound(res, pos):
    """|device drift[t] - drift[t]| <= 2^-50 n_max (t + 1) D per coordinate: n_max the largest
    n_pairs, D the largest absolute displacement component of any pair.  With u = 2^-53, to first
    order: the device's sum of n doubles of size <= D, in whatever order, is off by at most
    (n - 1) n D u and its mean by n D u, the yardstick's fsum mean by D u; the mean over a window of
    w <= t frames adds w D u; the running sum collects t such terms, t (n + 1 + t) D u, and its own
    adds (a chain here, a tree and a carry on the device, at most t (t + 1) / 2 + 10 t roundings of
    u |drift| <= u t D between them) come on top.  For the tables of up to 6 frames that the device
    tests take with rounding (n_max >= 2) that is below 8 n_max (t + 1) D u; the long tables have
    steps that are multiples of 1/4 and windows of 1 or 2 frames, so every operation on them is
    exact.  Derived, not measured; a logic error is nine or more orders above it."""
    pos = np.asarray(pos, dtype=np.float64)
    T = len(res.n_pairs)
    n_max = int(res.n_pairs.max()) if T else 0
    D = max([np.abs(pos[i] - pos[j]).max() for _, i, j in res.pairs], default=0.)
    return 2. ** -50 * n_max * (np.arange(T) + 1.)[:, None] * D


def table(frames, ndim=2):
    """``frames``: per frame a list of (particle, position tuple) -> (pos, frame_offset, particle)"""
    off, par, pos = [0], [], []
    for rows in frames:
        for p, x in rows:
            par.append(p)
            pos.append(x)
        off.append(len(par))
    return (np.array(pos, dtype=np.float64).reshape(-1, ndim), np.array(off, dtype=np.int64),
            np.array(par, dtype=np.int64))


def drifting_video(seed, n_frames=6, n_particles=5, ndim=2, absent=(1, 3), unlinked=True, jitter=0.05):
    """particles on a known drift plus jitter, rows of a frame in random order; particle
    ``absent[0]`` is missing in frame ``absent[1]``; one unlinked row in frame 2"""
    rng = np.random.RandomState(seed)
    start = rng.uniform(10., 90., (n_particles, ndim))
    velocity = np.array([0.7, -0.4, 0.25])[:ndim]
    frames = []
    for t in range(n_frames):
        rows = [(p, tuple(start[p] + t * velocity + rng.normal(0., jitter, ndim)))
                for p in range(n_particles) if not (absent and (p, t) == tuple(absent))]
        if unlinked and t == 2:
            rows.append((-1, tuple(rng.uniform(10., 90., ndim))))
        frames.append([rows[k] for k in rng.permutation(len(rows))])
    return table(frames, ndim)


def relabelled_video(seed, ndim=2):
    """T = 5, four particles; every id changes between frames 2 and 3: n_pairs[3] == 0"""
    rng = np.random.RandomState(seed)
    start = rng.uniform(10., 90., (4, ndim))
    frames = [[(p + (4 if t >= 3 else 0), tuple(start[p] + 0.5 * t + rng.normal(0., 0.05, ndim))) for p in range(4)]
              for t in range(5)]
    return table(frames, ndim)


def shuffled_video(seed, rows=3000, n_frames=3, ndim=2):
    """``rows`` particles in every frame, each frame in its own random order"""
    rng = np.random.RandomState(seed)
    start = rng.uniform(0., 1000., (rows, ndim))
    frames = []
    for t in range(n_frames):
        now = start + 0.3 * t + rng.normal(0., 0.1, (rows, ndim))
        frames.append([(int(p), tuple(now[p])) for p in rng.permutation(rows)])
    return table(frames, ndim)


def long_video(seed, n_frames, n_particles, empty=None, ndim=2):
    """``n_particles`` in every frame (none in frame ``empty``), steps that are multiples of 1/4:
    every sum of displacements is exact in any order, so a chunk carry or a stride that goes wrong
    shows as a difference, not as rounding"""
    rng = np.random.RandomState(seed)
    steps = rng.randint(-8, 9, (n_frames, n_particles, ndim)) / 4.
    now = 100. + np.cumsum(steps, axis=0)
    return table([[] if t == empty else [(p, tuple(now[t, p])) for p in range(n_particles)] for t in range(n_frames)], ndim)
