"""The two-point displacement correlation rule of ``clustertracking_amd/twopoint.py`` (include/ctrefine.h,
DESIGN.md 7b) restated in NumPy, clause by clause and vectorised per frame and lag, with Python integers
for the sums: the yardstick of ``test_twopoint_rule.py`` and ``test_gpu_twopoint.py``, and the builders of
their cases.  Nothing here imports the package."""
import collections
import math

import numpy as np

Result = collections.namedtuple('Result', ['r_edges', 'lags', 'n', 'sums', 'n_moved', 'beyond', 'unit'])
Means = collections.namedtuple('Means', ['dot', 'longitudinal', 'transverse', 'cos'])
TILE = 256          # rows of a work item of the device path
MATCH_TILE = 2048   # rows of the partner's frame in one LDS table
CHUNK = 256         # rows of a frame taken at a time here: memory, and int64 partial sums that cannot overflow


def bins(cutoff, dr):
    """clause 1: (r_edges [B + 1], edge2 [B + 1])"""
    n_bins = int(math.ceil(cutoff / dr))
    r_edges = np.arange(n_bins + 1, dtype=np.float64) * dr
    return r_edges, r_edges * r_edges


def fixed_point(max_disp):
    """clauses 5 and 8: (max2, e, unit)"""
    max2 = float(np.float64(max_disp) * np.float64(max_disp))
    e = math.frexp(max2)[1]                # max2 <= 2^e, and 2^(e - 1) <= max2
    if max2 == 2. ** (e - 1):
        e -= 1
    return max2, e, 2. ** (e - 40)


def partners(particle, rows, cand):
    """clause 4: for every row of ``rows`` the lowest row of ``cand`` (ascending) with its id, or -1"""
    ids, first = np.unique(particle[cand][particle[cand] >= 0], return_index=True)      # the first occurrence
    first_rows = cand[particle[cand] >= 0][first]
    p = particle[rows]
    if not len(ids):
        return np.full(len(rows), -1, dtype=np.int64)
    at = np.minimum(np.searchsorted(ids, p), len(ids) - 1)
    return np.where((p >= 0) & (ids[at] == p), first_rows[at], -1)


def displacements(q, particle, off, t, k, max2):
    """clauses 4 and 5 for frame t at lag k: (rows, u, u2, moved, beyond) of the rows of the frame"""
    T = len(off) - 1
    rows = np.arange(off[t], off[t + 1])
    ndim = q.shape[1]
    u = np.full((len(rows), ndim), np.nan)
    if t + k < T:
        partner = partners(particle, rows, np.arange(off[t + k], off[t + k + 1]))
        has = partner >= 0
        with np.errstate(invalid='ignore', over='ignore'):
            u[has] = q[partner[has]] - q[rows[has]]
    with np.errstate(invalid='ignore', over='ignore'):
        u2 = u[:, 0] * u[:, 0]
        for a in range(1, ndim):
            u2 = u2 + u[:, a] * u[:, a]
        finite = np.isfinite(u).all(1)             # a finite u: both rows exist
        moved = finite & (u2 <= max2)
        beyond = finite & (u2 > max2)
    return rows, u, u2, moved, beyond


def twopoint(pos, frame_offset, particle, lagtime, cutoff, dr=0.5, max_disp=None, mpp=1., group=None, pairs='all'):
    """clauses 1 to 9 for a table that is not refused; ``sums[k][b][s]`` are Python integers"""
    pos = np.asarray(pos, dtype=np.float64)
    off = np.asarray(frame_offset, dtype=np.int64)
    particle = np.asarray(particle, dtype=np.int64)
    N, ndim = pos.shape
    T = len(off) - 1
    lags = [int(k) for k in (lagtime if isinstance(lagtime, (list, tuple, np.ndarray)) else [lagtime])]
    r_edges, edge2 = bins(cutoff, dr)                                               # 1
    B = len(edge2) - 1
    q = pos * (np.asarray(mpp, dtype=np.float64) * np.ones(ndim))                   # 2
    max2, e, unit = fixed_point(max_disp)                                           # 8
    inv_unit, inv_cos = 2. ** (40 - e), 2. ** 40
    n = np.zeros((len(lags), B), dtype=np.int64)
    sums = [[[0, 0, 0] for _ in range(B)] for _ in lags]
    n_moved, beyond = np.zeros(len(lags), dtype=np.int64), np.zeros(len(lags), dtype=np.int64)
    if group is not None:
        group = np.asarray(group, dtype=np.int64)
    for ki, k in enumerate(lags):
        for t in range(T):
            rows, u, u2, moved, far = displacements(q, particle, off, t, k, max2)   # 4, 5
            n_moved[ki] += moved.sum()
            beyond[ki] += far.sum()
            R, U, U2, Q = rows[moved], u[moved], u2[moved], q[rows[moved]]
            for c in range(0, len(R), CHUNK):                                       # 6: (i, j), i of the chunk
                s = slice(c, c + CHUNK)
                d = Q[None, :, :] - Q[s][:, None, :]                                # R_a = q_j - q_i: [i, j, axis]
                d2 = d[..., 0] * d[..., 0]
                for a in range(1, ndim):
                    d2 = d2 + d[..., a] * d[..., a]
                keep = (d2 < edge2[B]) & (d2 > 0.) & (R[None, :] != R[s][:, None])
                if pairs != 'all':
                    same = (group[R][None, :] == group[R[s]][:, None]) & (group[R[s]][:, None] >= 0)
                    keep &= same if pairs == 'same' else ~same
                ii, jj = np.nonzero(keep)
                if not len(ii):
                    continue
                assert len(ii) <= 2 ** 21                                           # 2^41 per pair: an int64 holds the partial sums
                dd2, dv, ui, uj = d2[ii, jj], d[ii, jj], U[s][ii], U[jj]
                dot, ai, aj = ui[:, 0] * uj[:, 0], ui[:, 0] * dv[:, 0], uj[:, 0] * dv[:, 0]          # 7
                for a in range(1, ndim):
                    dot, ai, aj = dot + ui[:, a] * uj[:, a], ai + ui[:, a] * dv[:, a], aj + uj[:, a] * dv[:, a]
                along = (ai * aj) / dd2
                uu = U2[s][ii] * U2[jj]
                cs = np.where(uu > 0., dot / np.sqrt(np.where(uu > 0., uu, 1.)), 0.)
                b = np.searchsorted(edge2, dd2, side='right') - 1                   # edge2[b] <= d2 < edge2[b + 1]
                np.add.at(n[ki], b, 1)                                              # 9
                for si, (x, scale) in enumerate(((dot, inv_unit), (along, inv_unit), (cs, inv_cos))):
                    part = np.zeros(B, dtype=np.int64)
                    np.add.at(part, b, np.rint(x * scale).astype(np.int64))         # 8: ties to even, exact scaling
                    for bb in np.nonzero(part)[0]:
                        sums[ki][bb][si] += int(part[bb])
    return Result(r_edges, np.array(lags, dtype=np.int64), n, sums, n_moved, beyond, unit)


def words(sums):
    """clause 9: Python integers [K][B][3] as int64 [K, B, 3, 2] (hi, lo) of their 128-bit two's complement"""
    out = np.zeros((len(sums), len(sums[0]), 3, 2), dtype=np.int64)
    for k, per_lag in enumerate(sums):
        for b, cell in enumerate(per_lag):
            for s, v in enumerate(cell):
                two = v % (1 << 128)
                hi, lo = two >> 64, two & ((1 << 64) - 1)
                out[k, b, s, 0] = hi - (1 << 64) if hi >= 1 << 63 else hi
                out[k, b, s, 1] = lo - (1 << 64) if lo >= 1 << 63 else lo
    return out


def integer(word):
    """the Python integer of one (hi, lo)"""
    return int(word[0]) * (1 << 64) + (int(word[1]) % (1 << 64))


def integers(w):
    """int64 [K, B, 3, 2] back to Python integers [K][B][3]"""
    return [[[integer(w[k, b, s]) for s in range(3)] for b in range(w.shape[1])] for k in range(w.shape[0])]


def as_double(v):
    """clause 10: the integer v of a 128-bit sum as a double"""
    if -(1 << 63) <= v < (1 << 63):
        return float(v)                                    # one rounding, to nearest even
    two = v % (1 << 128)
    hi, lo = two >> 64, two & ((1 << 64) - 1)
    hi = hi - (1 << 64) if hi >= 1 << 63 else hi
    return float(np.float64(hi) * np.float64(2. ** 64) + np.float64(float(lo)))


def means(n, w, unit, ndim):
    """clause 10 from the counts and the words (hi, lo)"""
    K, B = n.shape
    out = Means(*(np.full((K, B), np.nan) for _ in range(4)))
    unit_cos = 2. ** -40
    for k in range(K):
        for b in range(B):
            if n[k, b] == 0:
                continue
            count = np.float64(float(int(n[k, b])))
            s_dot, s_l, s_c = (integer(w[k, b, s]) for s in range(3))
            out.dot[k, b] = (np.float64(as_double(s_dot)) * unit) / count
            out.longitudinal[k, b] = (np.float64(as_double(s_l)) * unit) / count
            out.cos[k, b] = (np.float64(as_double(s_c)) * unit_cos) / count
            out.transverse[k, b] = ((np.float64(as_double(s_dot - s_l)) * unit) / count) / np.float64(ndim - 1)
    return out


def assert_equal_bits(got, want, what=''):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, np.argwhere(~same)[:5], got[~same][:5], want[~same][:5])


# ---- the cases ----
def walkers(sizes, box, step, seed, ndim=2, n_walkers=None):
    """random walkers in a box, frame t holding ``sizes[t]`` of them in shuffled row order:
    (pos, frame_offset, particle)"""
    rs = np.random.RandomState(seed)
    P = n_walkers or max(sizes)
    start = rs.uniform(0., box, (P, ndim))
    pos, particle = [], []
    for t, rows in enumerate(sizes):
        start = start + rs.normal(0., step, (P, ndim)) if t else start
        who = rs.permutation(P)[:rows]
        pos.append(start[who])
        particle.append(who)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(pos), off, np.concatenate(particle).astype(np.int64)


TILE_SIZES = (2 * TILE + 1, TILE + 1, TILE, TILE - 1, 2, 1, 0, 2 * TILE + 1)
TILE_LAGS = (1, 2, 7)
TILE_KW = dict(cutoff=8., dr=0.5, max_disp=1.5)


def tile_edges(ndim=2, seed=11):
    """frames of 513, 257, 256, 255, 2, 1, 0 and 513 rows over 520 walkers: the tile's edge on the owner side
    and on the candidate side, an empty frame, and lag 7 from the first frame to the last; with an unlinked
    row, a repeated id in a frame on either side of a lag, a row that does not exist on either side, and a
    coincident pair that has moved.  (pos, frame_offset, particle, group)"""
    pos, off, particle = walkers(TILE_SIZES, (60., 30.)[ndim - 2], 0.4, seed, ndim, 520)
    pos, particle = pos.copy(), particle.copy()
    everywhere = set(particle[:off[1]]) & set(particle[off[1]:off[2]]) & set(particle[off[7]:]) - set(particle[:40])
    a, b = sorted(everywhere)[:2]                      # two walkers of the frames 0, 1 and 7 on one path: coincident and moved
    for t in range(len(off) - 1):
        rows = np.arange(off[t], off[t + 1])
        ra, rb = rows[particle[rows] == a], rows[particle[rows] == b]
        if len(ra) and len(rb):
            pos[rb[0]] = pos[ra[0]]
    particle[5] = -1                                   # unlinked
    particle[7] = particle[3]                          # a repeated id in the owners' frame: both have the same partner
    particle[off[1] + 9] = particle[off[1] + 4]        # ... in a partners' frame: the lower row is the partner
    particle[off[7] + 300] = particle[off[7] + 260]    # ... across the owners' tile edge of the last frame
    pos[10] = np.nan                                   # a row that does not exist
    pos[off[1] + 30, 0] = np.inf                       # ... and a partner that does not
    pos[off[7] + 2] = np.nan
    pos[21] = pos[20]                                  # coincident: d2 == 0 is no pair
    pos[off[2] + 256 - 1] = pos[off[2]]                # ... across the frame
    group = np.random.RandomState(seed + 1).randint(-2, 9, len(pos)).astype(np.int64)
    return pos, off, particle, group


def matching_edges(variant):
    """frames of 2049, 2048 and 2049 rows: the partners' frame is one full LDS table, or a table and one row
    more.  variant 'alone': the particle of the last row of the last frame has no other row there, so its
    only row lies in the second table; 'repeated': that row repeats the id of the row before it, on the
    other side of the edge, and of row 3: the lowest is the partner.  (pos, frame_offset, particle)"""
    pos, off, particle = walkers((MATCH_TILE + 1, MATCH_TILE, MATCH_TILE + 1), 150., 0.3, 5, 2, MATCH_TILE + 1)
    pos, particle = pos.copy(), particle.copy()
    last = off[2] + MATCH_TILE                         # row 2048 of the last frame
    if variant == 'repeated':
        particle[last] = particle[last - 1]
        particle[off[1] + 7] = particle[last - 1]      # so that an owner of frame 1 asks for it
        far = particle[off[2] + 3]
        particle[off[2] + 3] = particle[last - 2]      # and an id on rows 3 and 2046 of one table
        particle[off[1] + 8] = particle[last - 2]
        assert far >= 0
    else:
        assert (particle[off[2]:last] != particle[last]).all()
        particle[off[1] + 7] = particle[last]          # an owner of frame 1 asks for it
        particle[5] = particle[last]                   # and one of frame 0, at lag 2
    return pos, off, particle


def flush_table():
    """two frames of 8193 rows in a box 400 wide: 33 candidate tiles, so a workgroup flushes in the middle of
    its walk; independent steps, so sums of either sign.  (pos, frame_offset, particle)"""
    return walkers((32 * TILE + 1, 32 * TILE + 1), 400., 0.3, 2, 2)


def lattice_frames(nx, ny, moves):
    """frames of an nx x ny unit lattice, row-major; frame t + 1 is frame t moved by moves[t] (a vector for
    all rows or one per row): (pos, frame_offset, particle)"""
    base = np.stack(np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing='ij'), -1).reshape(-1, 2)
    frames = [base]
    for m in moves:
        frames.append(frames[-1] + np.asarray(m, dtype=np.float64))
    n = len(base)
    off = np.arange(len(frames) + 1, dtype=np.int64) * n
    return np.concatenate(frames), off, np.tile(np.arange(n, dtype=np.int64), len(frames))


def linked_table():
    """a DataFrame of four frames, 3 .. 6, in shuffled row order: a dimer (cluster 0, bond 3 along x) that moves
    by 0.5 along y per frame, and a dimer (cluster 1) whose two rows move by 0.25 along x, opposite ways"""
    import pandas as pd
    rows = []
    for t in range(4):
        rows += [(3 + t, 10. + 0.5 * t, 10., 10, 0), (3 + t, 10. + 0.5 * t, 13., 20, 0), (3 + t, 30., 30. - 0.25 * t, 35, 1),
                 (3 + t, 33., 30. + 0.25 * t, 40, 1)]
    f = pd.DataFrame(rows, columns=['frame', 'y', 'x', 'particle', 'cluster']).astype({'frame': np.int64, 'particle': np.int64, 'cluster': np.int32})
    return f.iloc[np.random.RandomState(3).permutation(len(f))]
