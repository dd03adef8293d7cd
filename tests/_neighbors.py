"""The nearest-neighbour rule of ``clustertracking_amd/static.py`` (include/ctrefine.h)
restated in NumPy, clause by clause and vectorised per frame: the yardstick of
``test_neighbors_rule.py`` and ``test_gpu_neighbors.py``, and the builders of their cases.  Nothing here
imports the package."""
import collections

import numpy as np

from _pair_correlation import assert_equal_bits, lattice, table, uniform_frames      # noqa: F401 (the tests use them from here)

Result = collections.namedtuple('Result', ['dist', 'dist2', 'index', 'count', 'particle_min', 'particle_min2'])
TILE = 256          # rows of a work item of the device path: the cases stand on its edges


def neighbors(pos, frame_offset, k=1, mpp=1., max_dist=None, group=None, pairs='all', lag=0, particle=None,
              n_particles=None):
    """clauses 1 to 8 for a table whose frame_offset is good"""
    pos = np.asarray(pos, dtype=np.float64)
    off = np.asarray(frame_offset, dtype=np.int64)
    N, ndim = pos.shape
    T = len(off) - 1
    q = pos * (np.asarray(mpp, dtype=np.float64) * np.ones(ndim))               # 1
    exists = np.isfinite(q).all(1)                                              # 2
    limit2 = np.inf if max_dist is None else np.float64(max_dist) * np.float64(max_dist)
    dist2 = np.full((N, k), np.nan)                                             # 7: rows with no result
    index = np.full((N, k), -1, dtype=np.int64)
    count = np.zeros(N, dtype=np.int64)
    for t in range(T):
        if t + lag >= T:                                                        # 3: no candidate frame
            continue
        rows = np.arange(off[t], off[t + 1])
        cand = np.arange(off[t + lag], off[t + lag + 1])
        rows_i, rows_j = rows[exists[rows]], cand[exists[cand]]
        if not len(rows_j):
            continue
        for c in range(0, len(rows_i), 512):                                    # 512 rows at a time: memory
            some = rows_i[c:c + 512]
            d = q[rows_j][None, :, :] - q[some][:, None, :]                     # 4: [i, j, axis]
            d2 = d[..., 0] * d[..., 0]
            for a in range(1, ndim):
                d2 = d2 + d[..., a] * d[..., a]
            keep = d2 < limit2                                                  # strict
            if lag == 0:
                keep &= rows_j[None, :] != some[:, None]
            if pairs != 'all':
                same = (group[rows_j][None, :] == group[some][:, None]) & (group[some][:, None] >= 0)
                keep &= same if pairs == 'same' else ~same
            count[some] = keep.sum(1)                                           # 5
            d2 = np.where(keep, d2, np.inf)                                     # a qualifying d2 is below +inf
            first = np.argsort(d2, axis=1, kind='stable')[:, :k]                # 6: (d2, j), rows_j ascends
            best = np.take_along_axis(d2, first, axis=1)
            found = best < np.inf
            m = first.shape[1]
            dist2[some, :m] = np.where(found, best, np.nan)
            index[some, :m] = np.where(found, rows_j[first], -1)
    dist = np.sqrt(dist2)
    particle_min = particle_min2 = None
    if particle is not None:                                                    # 8
        particle = np.asarray(particle, dtype=np.int64)
        P = max(int(particle.max()) + 1, 0) if n_particles is None and len(particle) else int(n_particles or 0)
        particle_min2 = np.full(P, np.nan)
        has = (index[:, 0] >= 0) & (particle >= 0) & (particle < P)
        best = np.full(P, np.inf)
        np.minimum.at(best, particle[has], dist2[has, 0])
        seen = np.zeros(P, dtype=bool)
        seen[particle[has]] = True
        particle_min2[seen] = best[seen]
        particle_min = np.sqrt(particle_min2)
    return Result(dist, dist2, index, count, particle_min, particle_min2)


def refused(n, k, n_particles=None):
    """clause 9: what a refused table gives"""
    per = None if n_particles is None else np.full(n_particles, np.nan)
    return Result(np.full((n, k), np.nan), np.full((n, k), np.nan), np.full((n, k), -1, dtype=np.int64),
                  np.zeros(n, dtype=np.int64), per, per)


def ulps(got, want):
    """the largest distance in units of the last place between two float arrays with NaN in the same
    places; both non-negative, so the bit patterns order as the values do"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    if not ok.any():
        return 0
    return int(np.abs(got[ok].view(np.int64) - want[ok].view(np.int64)).max())


# ---- the cases: the builders of the g(r) cases (table, uniform_frames, lattice) serve here too ----
def tile_edges(ndim=2, seed=3):
    """frames of 0, 1, 2, 255, 256, 257 and 513 rows: the tile's edge on the owner side and on the
    candidate side, an empty frame, a one-row frame, 9 work items"""
    return uniform_frames(seed, (0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1), (60., 45., 30.)[:ndim], ndim)


SHARED_CUTOFF, SHARED_DR = 8., 0.5      # 16 bins: r_edges[16] = 8 exactly, the box is a few cutoffs wide


def shared_rule(ndim):
    """(pos, frame_offset, group) for the rule that g(r) and the neighbours share -- the same d2, the same
    existence, the same group filter: the table of the tile edges with a row that does not exist inside
    a tile and groups -3 .. 11.  With ``edge='none'`` and the default box every finite row is a
    reference row, so ``count[t, :].sum()`` of g(r) at (SHARED_CUTOFF, SHARED_DR) is the sum over the rows
    of frame t of the neighbours' ``count`` at ``max_dist = SHARED_CUTOFF``, ``lag = 0``."""
    pos, off = tile_edges(ndim)
    pos = pos.copy()
    pos[off[5] + 100] = np.nan
    group = np.random.RandomState(6).randint(-3, 12, len(pos)).astype(np.int64)
    return pos, off, group


def counts_per_frame(count, frame_offset):
    """the neighbours' count[i] summed over the rows of every frame"""
    return np.array([count[a:b].sum() for a, b in zip(frame_offset[:-1], frame_offset[1:])], dtype=np.int64)
