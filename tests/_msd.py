"""The MSD rule (include/ctrefine.h) restated with plain loops: the yardstick of the
device path.  No engine, no oracle.  Every mean is ``math.fsum(...) / n``: the correctly rounded sum,
divided once.  Also an independent brute force over all row pairs, the generators of the test tables
and the derived bounds of the means."""
import collections
import math

import numpy as np

Result = collections.namedtuple('Result', ['msd', 'mean_d', 'mean_d2', 'n', 'max_d'])
U = 2. ** -53


def _moments(terms, ndim):
    """(msd, mean_d, mean_d2, n, max |d|) of a list of displacement vectors; clauses 4 to 7 and 9"""
    n = len(terms)
    if n == 0:
        nan = np.full(ndim, np.nan)
        return np.nan, nan, nan, 0, np.zeros(ndim)
    columns = [[float(d[a]) for d in terms] for a in range(ndim)]
    mean_d = np.array([math.fsum(c) / n for c in columns])
    mean_d2 = np.array([math.fsum(x * x for x in c) / n for c in columns])
    total = mean_d2[0]
    for a in range(1, ndim):
        total = total + mean_d2[a]
    return total, mean_d, mean_d2, n, np.array([max(abs(x) for x in c) for c in columns])


def tracks_of(frame_offset, particle):
    """clause 1: per id >= 0 a dict frame -> its lowest row"""
    off = np.asarray(frame_offset, dtype=np.int64)
    tracks = {}
    for t in range(len(off) - 1):
        for i in range(off[t], off[t + 1]):
            p = int(particle[i])
            if p >= 0:
                tracks.setdefault(p, {}).setdefault(t, i)
    return tracks


def _terms(pos, scale, track, k):
    """clauses 2 and 3: the displacements of a track at lag k, in frame order ([n, ndim])"""
    frames = [t for t in sorted(track) if t + k in track]
    return (pos[[track[t + k] for t in frames]] - pos[[track[t] for t in frames]]) * scale


def _scale(mpp, ndim):
    scale = np.asarray(mpp, dtype=np.float64)
    return np.repeat(scale, ndim) if scale.ndim == 0 else scale


def _result(cells, shape, ndim):
    """cells: a flat list of _moments results for the cells of ``shape``"""
    return Result(np.array([c[0] for c in cells], dtype=np.float64).reshape(shape),
                  np.array([c[1] for c in cells], dtype=np.float64).reshape(shape + (ndim,)),
                  np.array([c[2] for c in cells], dtype=np.float64).reshape(shape + (ndim,)),
                  np.array([c[3] for c in cells], dtype=np.int64).reshape(shape),
                  np.array([c[4] for c in cells], dtype=np.float64).reshape(shape + (ndim,)))


def msd(pos, frame_offset, particle, max_lagtime, mpp=1., particles=None, n_particles=None):
    """the per-particle rule: Result with [M, L] tables; ``particles`` defaults to 0 .. P - 1"""
    pos = np.asarray(pos, dtype=np.float64)
    particle = np.asarray(particle, dtype=np.int64)
    ndim = pos.shape[1]
    scale = _scale(mpp, ndim)
    P = int(n_particles) if n_particles is not None else (max(int(particle.max()) + 1, 0) if len(particle) else 0)
    ids = list(range(P)) if particles is None else [int(p) for p in particles]
    tracks = tracks_of(frame_offset, particle)
    cells = [_moments(_terms(pos, scale, tracks.get(p, {}), k), ndim) for p in ids for k in range(1, max_lagtime + 1)]
    return _result(cells, (len(ids), max_lagtime), ndim)


def emsd(pos, frame_offset, particle, max_lagtime, mpp=1.):
    """clause 10: the pairs of all particles pooled, in particle order; Result with [L] tables"""
    pos = np.asarray(pos, dtype=np.float64)
    particle = np.asarray(particle, dtype=np.int64)
    ndim = pos.shape[1]
    scale = _scale(mpp, ndim)
    tracks = tracks_of(frame_offset, particle)
    span = {p: max(track) - min(track) for p, track in tracks.items()}
    cells = []
    for k in range(1, max_lagtime + 1):
        pooled = []
        for p in sorted(tracks):
            if span[p] >= k:                     # a shorter track has no pair at this lag
                pooled.extend(list(_terms(pos, scale, tracks[p], k)))
        cells.append(_moments(pooled, ndim))
    return _result(cells, (max_lagtime,), ndim)


def brute_force(pos, frame_offset, particle, max_lagtime, mpp=1.):
    """Independent of the above: every pair of rows i < j is looked at once.  Returns
    ``{(p, k): _moments(...)}`` for the cells with a pair and ``{k: _moments(...)}`` pooled."""
    pos = np.asarray(pos, dtype=np.float64)
    off = np.asarray(frame_offset, dtype=np.int64)
    ndim = pos.shape[1]
    scale = _scale(mpp, ndim)
    frame = np.full(len(pos), -1)
    for t in range(len(off) - 1):
        frame[off[t]:off[t + 1]] = t
    exists = [particle[i] >= 0 and frame[i] >= 0 and
              not any(frame[h] == frame[i] and particle[h] == particle[i] for h in range(i)) for i in range(len(pos))]
    cells, pooled = {}, {}
    for i in range(len(pos)):
        for j in range(i + 1, len(pos)):
            k = frame[j] - frame[i]
            if exists[i] and exists[j] and particle[i] == particle[j] and 1 <= k <= max_lagtime:
                d = (pos[j] - pos[i]) * scale
                cells.setdefault((int(particle[i]), int(k)), []).append(d)
                pooled.setdefault(int(k), []).append(d)
    return ({key: _moments(v, ndim) for key, v in cells.items()}, {k: _moments(v, ndim) for k, v in pooled.items()})


def bound(want, squares=False, extra=0):
    """|device mean - yardstick mean| per cell and coordinate, for ``want.n`` terms of size at most
    ``X = want.max_d`` (``X**2`` for the squares): (n + 3 + extra) X u, u = 2^-53.  The terms are the
    same doubles on both sides (a subtraction, a product with mpp, a rounded square).  The device's
    recursive sum of n terms of size <= X, in whatever order, is off by at most (n - 1) n X u to
    first order and its mean by (n - 1) X u; the division rounds once more, X u; the yardstick's
    fsum is the rounded exact sum, off by n X u and its mean by X u, and its division adds X u: (n + 2)
    X u, and one X u more covers the terms of second order, (n u)^2 X, for any n below 2^26.  Derived,
    not measured; a logic error is many orders above it."""
    X = want.max_d ** 2 if squares else want.max_d
    return (want.n[..., None] + 3. + extra) * X * U


def bound_msd(want):
    """msd is the sum of ndim means of squares, added in the same order on both sides: the bounds of
    those means, plus 2 (ndim - 1) roundings of a partial sum that is at most msd (ndim - 1 additions
    on either side)."""
    ndim = want.mean_d2.shape[-1]
    return bound(want, squares=True).sum(-1) + 2. * (ndim - 1) * np.nan_to_num(want.msd) * U * (1. + 2. ** -40)


def assert_equal_bits(got, want, what=''):
    """msd, mean_d, mean_d2 and n of the device equal the yardstick's bit for bit (NaN where it has NaN)"""
    for name in ('msd', 'mean_d', 'mean_d2'):
        g, w = np.asarray(getattr(got, name)), getattr(want, name)
        assert g.shape == w.shape and g.dtype == np.float64, (what, name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes() or (np.isnan(g) == np.isnan(w)).all() and (g[~np.isnan(w)] == w[~np.isnan(w)]).all(), \
            (what, name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])
    assert (np.asarray(got.n) == want.n).all(), (what, 'n')


def assert_within_bounds(got, want, what=''):
    """the same NaN cells and counts; every mean within its derived bound; prints the largest errors"""
    assert (np.asarray(got.n) == want.n).all(), (what, 'n')
    for name, lim in (('mean_d', bound(want)), ('mean_d2', bound(want, squares=True)), ('msd', bound_msd(want))):
        g, w = np.asarray(getattr(got, name)), getattr(want, name)
        assert (np.isnan(g) == np.isnan(w)).all(), (what, name, 'NaN cells')
        err = np.nan_to_num(np.abs(g - w))
        print(what, name, 'max error', err.max() if err.size else 0., 'bound there', lim.reshape(-1)[err.argmax()] if err.size else 0.)
        assert (err <= lim).all(), (what, name, err.max())


# ---- tables ----
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


def exact_tracks(seed, tracks, n_frames=None, ndim=2, extra=()):
    """Tracks whose steps are multiples of 1/4: with mpp a power of two every sum of displacements
    and of their squares is exact in any order (below 2^53 units of mpp^2 / 16), so a stride, a tile
    edge or a chunk carry that goes wrong shows as a difference, not as rounding.  ``tracks``: per id
    the list of its frames (ascending; gaps as wanted); ``extra``: (frame, id) rows added behind the
    rows of that frame with a position of their own: a repeated id (any id >= 0) or an unlinked row
    (id < 0).  The rows of a frame are in a random order, the extra rows last."""
    rng = np.random.RandomState(seed)
    T = n_frames if n_frames is not None else 1 + max([f[-1] for f in tracks if len(f)] + [e[0] for e in extra] + [0])
    frames = [[] for _ in range(T)]
    for p, fr in enumerate(tracks):
        if not len(fr):
            continue
        fr = np.asarray(fr)
        walk = 100. + np.cumsum(rng.randint(-8, 9, (fr[-1] - fr[0] + 1, ndim)) / 4., axis=0)
        for t in fr:
            frames[t].append((p, tuple(walk[t - fr[0]])))
    frames = [[rows[i] for i in rng.permutation(len(rows))] for rows in frames]
    for t, p in extra:
        frames[t].append((p, tuple(rng.randint(0, 800, ndim) / 4.)))
    return table(frames, ndim)


def span_with_gap(first, span, gap):
    """the frames first .. first + span - 1 without first + gap[0] .. first + gap[1] - 1"""
    return [first + f for f in range(span) if not gap[0] <= f < gap[1]]


def jittered_video(seed, n_frames=6, n_particles=5, ndim=2, absent=(1, 3), jitter=0.05):
    """as ``_drift.drifting_video``: particles on a common drift plus jitter, rows of a frame in random
    order, particle ``absent[0]`` missing in frame ``absent[1]``, one unlinked row in frame 2"""
    rng = np.random.RandomState(seed)
    start = rng.uniform(10., 90., (n_particles, ndim))
    velocity = np.array([0.7, -0.4, 0.25])[:ndim]
    frames = []
    for t in range(n_frames):
        rows = [(p, tuple(start[p] + t * velocity + rng.normal(0., jitter, ndim)))
                for p in range(n_particles) if (p, t) != tuple(absent)]
        if t == 2:
            rows.append((-1, tuple(rng.uniform(10., 90., ndim))))
        frames.append([rows[k] for k in rng.permutation(len(rows))])
    return table(frames, ndim)
