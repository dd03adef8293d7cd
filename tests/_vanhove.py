"""The van Hove rule (include/ctrefine.h) restated with plain loops: the yardstick of
the device path.  No engine, no oracle.  The tracks and the pairs of a lag are ``_msd``'s (clauses 1 to
3 are the MSD rule's); a bin is ``np.searchsorted(edges, d, side='right') - 1`` against the edges the
host computes; ``d2`` is summed in axis order; every mean is ``math.fsum(...) / n``; ``alpha2`` is the
clause-9 expression in float64.  Also an independent brute force over all row pairs, with the bins
found by comparing against every edge, and the derived bound of ``mean_d4``."""
import collections
import math

import numpy as np

import _msd

Result = collections.namedtuple('Result', ['lags', 'edges', 'r_edges', 'count', 'below', 'above', 'density', 'count_r',
                                           'above_r', 'density_r', 'n', 'mean_d', 'mean_d2', 'mean_d4', 'alpha2', 'max_d'])
U = _msd.U
FLOATS = ('density', 'density_r', 'mean_d', 'mean_d2', 'mean_d4', 'alpha2')
COUNTS = ('count', 'below', 'above', 'count_r', 'above_r', 'n')


def bins(bin_width, max_disp):
    """clauses 5 and 6: (H, edges [2 H + 1], r_edges [H + 1], edge2 [H + 1])"""
    half = int(math.ceil(max_disp / bin_width))
    edges = (np.arange(2 * half + 1, dtype=np.float64) - half) * bin_width
    r_edges = np.arange(half + 1, dtype=np.float64) * bin_width
    return half, edges, r_edges, r_edges * r_edges


def alpha2_of(mean_d2, mean_d4):
    """clause 9 in float64, every operation rounded on its own; NaN where mean_d2 is 0 or NaN"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.asarray(mean_d4, dtype=np.float64) / (3. * (np.asarray(mean_d2, dtype=np.float64) * mean_d2)) - 1.


def _cell(terms, ndim, half, edges, edge2, bin_width):
    """clauses 5 to 10 for the displacement vectors of one lag"""
    n = len(terms)
    count, below, above = np.zeros((ndim, 2 * half), dtype=np.int64), np.zeros(ndim, dtype=np.int64), np.zeros(ndim, dtype=np.int64)
    count_r, above_r = np.zeros(half, dtype=np.int64), 0
    columns = [[float(d[a]) for d in terms] for a in range(ndim)]
    for a, col in enumerate(columns):
        for x in col:
            if x != x:                           # a NaN is in no bin and in neither tail
                continue
            b = int(np.searchsorted(edges, x, side='right')) - 1
            if b < 0:
                below[a] += 1
            elif b >= 2 * half:
                above[a] += 1
            else:
                count[a, b] += 1
    for i in range(n):
        d2 = columns[0][i] * columns[0][i]
        for a in range(1, ndim):
            d2 = d2 + columns[a][i] * columns[a][i]
        if d2 != d2:
            continue
        b = int(np.searchsorted(edge2, d2, side='right')) - 1
        if b >= half:
            above_r += 1
        else:
            count_r[b] += 1
    nan = np.full(ndim, np.nan)
    if n == 0:
        return (count, below, above, np.full((ndim, 2 * half), np.nan), count_r, above_r, np.full(half, np.nan), 0,
                nan, nan, nan, nan, np.zeros(ndim))
    mean_d = np.array([math.fsum(c) / n for c in columns])
    mean_d2 = np.array([math.fsum(x * x for x in c) / n for c in columns])
    mean_d4 = np.array([math.fsum((x * x) * (x * x) for x in c) / n for c in columns])
    per = n * bin_width
    return (count, below, above, count / per, count_r, above_r, count_r / per, n, mean_d, mean_d2, mean_d4,
            alpha2_of(mean_d2, mean_d4), np.array([max([abs(x) for x in c if x == x] + [0.]) for c in columns]))


def _result(lags, edges, r_edges, cells):
    stack = lambda i, dtype: np.array([c[i] for c in cells], dtype=dtype)
    return Result(np.array(lags, dtype=np.int64), edges, r_edges, stack(0, np.int64), stack(1, np.int64), stack(2, np.int64),
                  stack(3, np.float64), stack(4, np.int64), stack(5, np.int64), stack(6, np.float64), stack(7, np.int64),
                  stack(8, np.float64), stack(9, np.float64), stack(10, np.float64), stack(11, np.float64), stack(12, np.float64))


def vanhove(pos, frame_offset, particle, lags, bin_width, max_disp, mpp=1.):
    """the rule: Result with a leading axis of ``len(lags)``; the pairs pooled in particle order"""
    pos = np.asarray(pos, dtype=np.float64)
    particle = np.asarray(particle, dtype=np.int64)
    ndim = pos.shape[1]
    scale = _msd._scale(mpp, ndim)
    half, edges, r_edges, edge2 = bins(bin_width, max_disp)
    tracks = _msd.tracks_of(frame_offset, particle)
    cells = []
    for k in lags:
        pooled = []
        for p in sorted(tracks):
            if max(tracks[p]) - min(tracks[p]) >= k:
                pooled.extend(list(_msd._terms(pos, scale, tracks[p], k)))
        cells.append(_cell(pooled, ndim, half, edges, edge2, bin_width))
    return _result(lags, edges, r_edges, cells)


def brute_force(pos, frame_offset, particle, lags, bin_width, max_disp, mpp=1.):
    """Independent of the above: every pair of rows i < j is looked at once, and a bin is found by
    comparing with every edge.  Returns ``{k: (count, below, above, count_r, above_r, n, sums of d, of d^2,
    of d^4)}`` for every lag, the sums as lists of terms."""
    pos = np.asarray(pos, dtype=np.float64)
    off = np.asarray(frame_offset, dtype=np.int64)
    ndim = pos.shape[1]
    scale = _msd._scale(mpp, ndim)
    half = int(math.ceil(max_disp / bin_width))
    frame = np.full(len(pos), -1)
    for t in range(len(off) - 1):
        frame[off[t]:off[t + 1]] = t
    exists = [particle[i] >= 0 and frame[i] >= 0 and
              not any(frame[h] == frame[i] and particle[h] == particle[i] for h in range(i)) for i in range(len(pos))]
    out = {k: [np.zeros((ndim, 2 * half), dtype=np.int64), np.zeros(ndim, dtype=np.int64), np.zeros(ndim, dtype=np.int64),
               np.zeros(half, dtype=np.int64), 0, 0, [[] for _ in range(ndim)], [[] for _ in range(ndim)],
               [[] for _ in range(ndim)]] for k in lags}
    for i in range(len(pos)):
        for j in range(i + 1, len(pos)):
            k = int(frame[j] - frame[i])
            if not (exists[i] and exists[j] and particle[i] == particle[j] and k in out):
                continue
            cell = out[k]
            d = (pos[j] - pos[i]) * scale
            cell[5] += 1
            d2 = 0.
            for a in range(ndim):
                x = float(d[a])
                cell[6][a].append(x)
                cell[7][a].append(x * x)
                cell[8][a].append((x * x) * (x * x))
                d2 = x * x if a == 0 else d2 + x * x
                if x < (0 - half) * bin_width:
                    cell[1][a] += 1
                elif x >= (2 * half - half) * bin_width:
                    cell[2][a] += 1
                for b in range(2 * half):
                    if (b - half) * bin_width <= x < (b + 1 - half) * bin_width:
                        cell[0][a, b] += 1
            if d2 >= (half * bin_width) * (half * bin_width):
                cell[4] += 1
            for b in range(half):
                if (b * bin_width) * (b * bin_width) <= d2 < ((b + 1) * bin_width) * ((b + 1) * bin_width):
                    cell[3][b] += 1
    return out


def bound_d4(want):
    """|device mean_d4 - yardstick mean_d4| per lag and coordinate: ``_msd.bound``'s argument with ``X =
    max |d|**4``: the terms are the same doubles on both sides (a subtraction, a product with mpp, two
    rounded squares), n of them of size at most X; the device's recursive sum in whatever order and
    its division, the yardstick's fsum and its division, and one X u for second order: (n + 3) X u."""
    return (want.n[..., None] + 3.) * want.max_d ** 4 * U


def same_floats(g, w):
    """equal bit for bit, NaN where the yardstick has NaN"""
    g, w = np.asarray(g), np.asarray(w)
    return g.shape == w.shape and g.dtype == np.float64 and bool(((g == w) | (np.isnan(g) & np.isnan(w))).all())


def assert_counts(got, want, what=''):
    for name in COUNTS:
        g, w = np.asarray(getattr(got, name)), getattr(want, name)
        assert g.dtype == np.int64 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert (g == w).all(), (what, name, np.argwhere(g != w)[:5])
    assert (np.asarray(got.lags) == want.lags).all()
    assert np.asarray(got.edges).tobytes() == want.edges.tobytes() and np.asarray(got.r_edges).tobytes() == want.r_edges.tobytes()


def assert_equal_bits(got, want, what=''):
    """counts, tails, the three means, alpha2 and the densities of the device equal the yardstick's"""
    assert_counts(got, want, what)
    for name in FLOATS:
        assert same_floats(getattr(got, name), getattr(want, name)), (what, name, getattr(got, name), getattr(want, name))
