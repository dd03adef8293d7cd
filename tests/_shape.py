"""The rule of clustertracking_amd.shape restated in plain NumPy with loops (the CPU yardstick of
tests/test_shape_rule.py and tests/test_gpu_shape.py, and of tools/shape_time.py), and the launch
decision of the dynamics kernel restated from the host code that takes it.  Nothing here touches the
engine.

The rule is the project's own (include/ctrefine.h): rule 1 the coordinates of a frame,
rule 2 their displacement statistics and static moments, rule 3 their histograms.
"""
import math

import numpy as np

# ---- the launch decision of ctr_shape_dynamics_device (clustertracking_amd/csrc/) ----------------
SHP_THREADS, SHP_TILE, SHP_NSUM, SHP_RED_ROW = 256, 256, 4, 80                # shape_kernels.h:31-36
SHP_RED = (SHP_THREADS // 64) * SHP_RED_ROW                                   # shape_kernels.h:37
SHP_HALO_CAP = 768                                                            # shape_kernels.h:38, ctrefine.h
SHP_LDS_MAX = 64 * 1024                                                       # tu_shape.hip:18
TILE = SHP_TILE


def n_coords(cluster_size):
    n = cluster_size
    return n * (n - 1) // 2 + n * (n - 1) * (n - 2) // 2 + 1


def shp_halo_max(C):
    """tu_shape.hip:22-25: as many frames as fit beside the tile in 64 KiB, SHP_HALO_CAP at the most"""
    return min((SHP_LDS_MAX // 8 - SHP_RED) // C - SHP_TILE, SHP_HALO_CAP)


def shp_halo(n_frames, C):
    """frames staged in LDS behind a tile (tu_shape.hip:30-33): those beyond the first tile, up to
    shp_halo_max; it depends on the number of frames and of coordinates alone, never on the lags"""
    return min(max(n_frames - SHP_TILE, 0), shp_halo_max(C))


def shp_lds_bytes(halo, C):
    """tu_shape.hip:35"""
    return 8 * (SHP_RED + C * (SHP_TILE + halo))


def shp_reads_global(n_frames, C, lag):
    """does any row of this lag read its later frame from global memory?  Lane i of a tile that starts
    at b0 finds frame b0 + i + lag in LDS while i + lag < min(SHP_TILE + halo, n_frames - b0)
    (shape_kernels.h:211, shape_partial_kernel)"""
    if lag < 1 or lag >= n_frames:
        return False
    staged = SHP_TILE + shp_halo(n_frames, C)
    for b0 in range(0, n_frames, SHP_TILE):
        last = min(b0 + SHP_TILE, n_frames - lag) - 1 - b0          # last lane of the tile with a row
        if last >= 0 and last + lag >= min(staged, n_frames - b0):
            return True
    return False


# ---- rule 1: the coordinates ---------------------------------------------------------------------
def names(cluster_size):
    n = cluster_size
    out = ['bond_%d%d' % (a, b) for a in range(n) for b in range(a + 1, n)]
    for a in range(n):
        others = [i for i in range(n) if i != a]
        for i, b in enumerate(others):
            for c in others[i + 1:]:
                out.append('angle_%d_%d%d' % (a, b, c))
    return tuple(out + ['rg'])


def _scale(mpp, ndim):
    s = np.asarray(mpp, dtype=np.float64)
    return np.repeat(s, ndim) if s.ndim == 0 else s


def coords(pos, cluster_size, ndim, mpp=1.):
    """pos [T, F, n, ndim] -> coords [T, F, C].  The loops run over features and axes; every line is one
    IEEE operation per frame (NumPy's elementwise float64 arithmetic contracts nothing)"""
    pos = np.asarray(pos, dtype=np.float64)
    n = cluster_size
    assert pos.ndim == 4 and pos.shape[2:] == (n, ndim)
    scale = _scale(mpp, ndim)
    x = [[pos[:, :, i, k] * scale[k] for k in range(ndim)] for i in range(n)]
    present = np.ones(pos.shape[:2], dtype=bool)
    for i in range(n):
        for k in range(ndim):
            present &= np.isfinite(x[i][k])
    out = []
    with np.errstate(all='ignore'):
        for a in range(n):
            for b in range(a + 1, n):
                s = np.zeros(pos.shape[:2])
                for k in range(ndim):
                    d = x[b][k] - x[a][k]
                    s = s + d * d
                out.append(np.sqrt(s))
        for a in range(n):
            others = [i for i in range(n) if i != a]
            for i, b in enumerate(others):
                for c in others[i + 1:]:
                    u = [x[b][k] - x[a][k] for k in range(ndim)]
                    v = [x[c][k] - x[a][k] for k in range(ndim)]
                    dot = np.zeros(pos.shape[:2])
                    for k in range(ndim):
                        dot = dot + u[k] * v[k]
                    if ndim == 2:
                        cr = np.abs(u[0] * v[1] - u[1] * v[0])
                    else:
                        c0 = u[1] * v[2] - u[2] * v[1]
                        c1 = u[2] * v[0] - u[0] * v[2]
                        c2 = u[0] * v[1] - u[1] * v[0]
                        cr = np.sqrt(c0 * c0 + c1 * c1 + c2 * c2)
                    out.append(np.arctan2(cr, dot))
        cen = []
        for k in range(ndim):
            s = np.zeros(pos.shape[:2])
            for i in range(n):
                s = s + x[i][k]
            cen.append(s / float(n))
        s = np.zeros(pos.shape[:2])
        for i in range(n):
            for k in range(ndim):
                e = x[i][k] - cen[k]
                s = s + e * e
        out.append(np.sqrt(s / float(n)))
    out = np.stack(out, -1)
    assert out.shape[2] == n_coords(n)
    out[~present] = np.nan
    return out


# ---- rule 2: dynamics ----------------------------------------------------------------------------
def dynamics(q, lags, fps=1.):
    """q [T, F, C] (the coordinates), lags [L]: a dict of the outputs of shape_dynamics_arrays"""
    q = np.asarray(q, dtype=np.float64)
    T, F, C = q.shape
    L = len(lags)
    n = np.zeros((T, C, L), dtype=np.int64)
    sums = np.zeros((3, T, C, L))
    for t in range(T):
        for c in range(C):
            for i, k in enumerate(lags):
                k = int(k)
                if k < 1 or k >= F:
                    continue
                a, b = q[t, :-k, c], q[t, k:, c]
                rows = np.isfinite(a) & np.isfinite(b)
                d = b[rows] - a[rows]
                d2 = d * d
                n[t, c, i] = len(d)
                sums[:, t, c, i] = d.sum(), d2.sum(), (d2 * d2).sum()
    lag = np.asarray(lags, dtype=np.float64)
    out = dict(n=n, pooled_n=n.sum(0))
    with np.errstate(invalid='ignore', divide='ignore'):
        for j, name in enumerate(('mean_d', 'mean_d2', 'mean_d4')):
            out[name] = np.where(n > 0, sums[j] / n, np.nan)
            out['pooled_' + name] = np.where(out['pooled_n'] > 0, sums[j].sum(0) / out['pooled_n'], np.nan)
        out['flex'] = out['mean_d2'] * 0.5 * fps / lag
        out['pooled_flex'] = out['pooled_mean_d2'] * 0.5 * fps / lag
    count = np.zeros((T, C), dtype=np.int64)
    mom = np.full((4, T, C), np.nan)
    for t in range(T):
        for c in range(C):
            v = q[t, :, c]
            v = v[np.isfinite(v)]
            count[t, c] = len(v)
            if len(v):
                mean = v.sum() / len(v)
                mom[:, t, c] = mean, ((v - mean) ** 2).sum() / len(v), v.min(), v.max()
    out.update(n_frames=count, mean=mom[0], var=mom[1], min=mom[2], max=mom[3])
    return out


# ---- rule 3: distributions -----------------------------------------------------------------------
def edges(bond_max, bond_dr, angle_bins):
    B = max(int(math.ceil(bond_max / bond_dr)), 1)
    return np.arange(B + 1, dtype=np.float64) * bond_dr, np.linspace(0., np.pi, angle_bins + 1)


def _count(values, e, closed):
    """values into the bins of e by comparison: (count [bins], above); closed: the last bin takes e[-1]"""
    bins = len(e) - 1
    count, above = np.zeros(bins, dtype=np.int64), 0
    for v in values:
        if np.isnan(v) or v < e[0]:
            continue
        if v > e[-1] or (v == e[-1] and not closed):
            above += 1
            continue
        b = min(int(np.searchsorted(e, v, side='right')) - 1, bins - 1)
        assert e[b] <= v and (v < e[b + 1] or (closed and b == bins - 1))
        count[b] += 1
    return count, above


def histogram(q, cluster_size, bond_max, bond_dr, angle_bins, per_track=False):
    """q [T, F, C]: a dict of the outputs of shape_histogram_arrays"""
    q = np.asarray(q, dtype=np.float64)
    T, F, C = q.shape
    nb = cluster_size * (cluster_size - 1) // 2
    na = C - 1 - nb
    be, ae = edges(bond_max, bond_dr, angle_bins)
    B, A = len(be) - 1, len(ae) - 1
    groups = [q[t] for t in range(T)] if per_track else [q.reshape(T * F, C)]
    G = len(groups)
    count_bond, above = np.zeros((G, nb + 1, B), dtype=np.int64), np.zeros((G, nb + 1), dtype=np.int64)
    count_angle, n = np.zeros((G, na, A), dtype=np.int64), np.zeros(G, dtype=np.int64)
    for g, rows in enumerate(groups):
        n[g] = (~np.isnan(rows[:, 0])).sum()
        for r, c in enumerate(list(range(nb)) + [C - 1]):
            count_bond[g, r], above[g, r] = _count(rows[:, c], be, False)
        for r in range(na):
            count_angle[g, r], over = _count(rows[:, nb + r], ae, True)
            assert over == 0
    with np.errstate(invalid='ignore', divide='ignore'):
        nn = n.astype(np.float64)
        density_bond = np.where(nn[:, None, None] > 0, count_bond / (nn[:, None, None] * bond_dr), np.nan)
        density_angle = np.where(nn[:, None, None] > 0, count_angle / (nn[:, None, None] * (np.pi / A)), np.nan)
    out = dict(bond_edges=be, angle_edges=ae, count_bond=count_bond, above=above, count_angle=count_angle, n=n,
               density_bond=density_bond, density_angle=density_angle)
    if not per_track:
        for key in ('count_bond', 'above', 'count_angle', 'density_bond', 'density_angle'):
            out[key] = out[key][0]
    return out


def min_angle_edge_distance(q, cluster_size, angle_bins):
    """the smallest distance of a finite angle of q [.., C] to an interior angle edge (the ends 0 and pi
    belong to their bins whatever the rounding); inf without angles or interior edges"""
    nb = cluster_size * (cluster_size - 1) // 2
    ang = np.asarray(q)[..., nb:-1].ravel()
    ang = ang[np.isfinite(ang)]
    inner = np.linspace(0., np.pi, angle_bins + 1)[1:-1]
    if not len(ang) or not len(inner):
        return np.inf
    return float(np.abs(ang[:, None] - inner[None, :]).min())


# ---- inputs ----------------------------------------------------------------------------------------
def clusters(rng, T, F, cluster_size, ndim):
    """tests/test_gpu_motion.py:_clusters: features a few pixels apart around a wandering centre; per
    track its own missing frames and one missing coordinate"""
    pos = rng.uniform(20., 60., (T, F, 1, ndim)) + rng.uniform(-4., 4., (T, F, cluster_size, ndim))
    for t in range(T):
        gone = rng.rand(F) < 0.1 * (t + 1)
        pos[t, gone] = np.nan
        if F > 2:
            pos[t, (5 * t + 1) % F, cluster_size - 1, 0] = np.nan     # one coordinate missing
    return pos


def clusters_off_edges(seed, T, F, cluster_size, ndim, mpp, angle_bins, margin=1e-9, tries=50):
    """`clusters` drawn with seed, seed + 1, ... until no angle of the restatement lies within `margin`
    of an interior angle edge: (pos, coordinates, the seed that held).  A condition on the inputs of
    the histogram tests: device angles are a few ulp from NumPy's, not bit for bit"""
    for s in range(seed, seed + tries):
        pos = clusters(np.random.RandomState(s), T, F, cluster_size, ndim)
        q = coords(pos, cluster_size, ndim, mpp)
        if min_angle_edge_distance(q, cluster_size, angle_bins) > margin:
            return pos, q, s
    raise AssertionError("no seed in [%d, %d) keeps the angles off the edges" % (seed, seed + tries))


# the inputs of the histogram tests: tests/test_shape_rule.py checks on the CPU that the seeds hold the
# condition of clusters_off_edges, tests/test_gpu_shape.py runs them.  B = 1 and A = 1; B = 4096 and A =
# 1024; per_track with T = 3; more frames than one workgroup's chunk of 4096 (shape_kernels.h:39)
HIST_CASES = {
    'b1_a1': dict(seed=11, T=1, F=300, cluster_size=3, ndim=2, mpp=0.5, bond_max=3., bond_dr=3., angle_bins=1,
                  per_track=False),
    'b4096_a1024': dict(seed=12, T=3, F=300, cluster_size=4, ndim=3, mpp=(0.5, 0.25, 0.25), bond_max=2.,
                        bond_dr=2. ** -11, angle_bins=1024, per_track=False),
    'per_track': dict(seed=13, T=3, F=513, cluster_size=3, ndim=3, mpp=0.37, bond_max=2.5, bond_dr=0.05, angle_bins=90,
                      per_track=True),
    'tetramer_2d': dict(seed=14, T=2, F=257, cluster_size=4, ndim=2, mpp=1., bond_max=6., bond_dr=0.1, angle_bins=180,
                        per_track=True),
    'two_chunks': dict(seed=15, T=3, F=1500, cluster_size=2, ndim=2, mpp=0.2, bond_max=1.5, bond_dr=0.01, angle_bins=7,
                       per_track=False),
}


def assert_rows(got, want, what=''):
    """got, want [T, C, ...]: equal NaN pattern, every (track, coordinate) row within 1e-10 of the
    largest magnitude of its wanted values (sums of float64 terms: n eps is far below), the project's
    tensor tolerance (tests/_motion.py:assert_tensors)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (np.isnan(got) == np.isnan(want)).all(), what
    g, w = got.reshape(got.shape[0] * got.shape[1], -1), want.reshape(got.shape[0] * got.shape[1], -1)
    for i in range(len(w)):
        ok = np.isfinite(w[i])
        if ok.any():
            err, top = np.abs(g[i][ok] - w[i][ok]).max(), np.abs(w[i][ok]).max()
            assert err <= 1e-10 * top, (what, i, err, top)
