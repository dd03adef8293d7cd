"""The rule of clustertracking_amd.motion restated in vectorised NumPy (the CPU yardstick of
tests/test_motion_rule.py and tests/test_gpu_motion.py, and of tools/motion_time.py), and the
launch decision of the diffusion kernel restated from the host code that takes it.

The rule is the reference's (motion.py:40-198); tests/golden/motion/motion_cases.npz pins this
restatement to it.  Nothing here touches the engine.
"""
import numpy as np

PERMUTATIONS = {
    2: [[0, 1], [1, 0]],
    3: [[0, 1, 2], [2, 0, 1], [1, 2, 0], [2, 1, 0], [0, 2, 1], [1, 0, 2]],
    4: [[0, 1, 2, 3], [0, 2, 3, 1], [0, 3, 1, 2], [1, 0, 2, 3], [1, 2, 3, 0], [1, 3, 0, 2],
        [2, 0, 1, 3], [2, 1, 3, 0], [2, 3, 0, 1], [3, 0, 1, 2], [3, 1, 2, 0], [3, 2, 0, 1]],
}

# ---- the launch decision of ctr_diffusion_device (clustertracking_amd/csrc/) -----------------
MOT_THREADS, MOT_TILE, MOT_ROW, MOT_NSUM, MOT_NPAD = 256, 256, 12, 22, 24     # motion_kernels.h:30-34
MOT_RED = (MOT_THREADS // 64) * MOT_NPAD                                      # motion_kernels.h:35
MOT_LDS_MAX = 64 * 1024                                                       # tu_motion.hip:17
MOT_HALO_MAX = (MOT_LDS_MAX // 8 - MOT_RED) // MOT_ROW - MOT_TILE             # tu_motion.hip:19
TILE = MOT_TILE


def mot_halo(n_frames):
    """frames staged in LDS behind a tile (tu_motion.hip:25-28): those beyond the first tile, as
    many as fit; it depends on the number of frames alone, never on the lags"""
    return min(max(n_frames - MOT_TILE, 0), MOT_HALO_MAX)


def mot_lds_bytes(halo):
    """tu_motion.hip:30"""
    return 8 * (MOT_RED + MOT_ROW * (MOT_TILE + halo))


def mot_reads_global(n_frames, lag):
    """does any row of this lag read its later frame from global memory?  Lane i of a tile that
    starts at b0 finds frame b0 + i + lag in LDS while i + lag < min(MOT_TILE + halo, n_frames - b0)
    (motion_kernels.h: diffusion_partial_kernel)"""
    if lag < 1 or lag >= n_frames:
        return False
    staged = MOT_TILE + mot_halo(n_frames)
    for b0 in range(0, n_frames, MOT_TILE):
        last = min(b0 + MOT_TILE, n_frames - lag) - 1 - b0          # last lane of the tile with a row
        if last >= 0 and last + lag >= min(staged, n_frames - b0):
            return True
    return False


# ---- orientation -----------------------------------------------------------------------------
def _unit(v):
    with np.errstate(invalid='ignore', divide='ignore'):
        return v / np.sqrt((v * v).sum(-1))[..., None]


def _rotate_about(z, theta, v):
    """reference rotation_matrix(z, theta) applied to v, for arrays of axes [..., 3]"""
    with np.errstate(invalid='ignore', divide='ignore'):
        axis = z / np.sqrt((z * z).sum(-1))[..., None]
    a = np.cos(theta / 2.0)
    s = np.sin(theta / 2.0)
    b, c, d = -axis[..., 0] * s, -axis[..., 1] * s, -axis[..., 2] * s
    aa, bb, cc, dd = a * a, b * b, c * c, d * d
    bc, ad, ac, ab, bd, cd = b * c, a * d, a * c, a * b, b * d, c * d
    R = np.stack([np.stack([aa + bb - cc - dd, 2 * (bc + ad), 2 * (bd - ac)], -1),
                  np.stack([2 * (bc - ad), aa + cc - bb - dd, 2 * (cd + ab)], -1),
                  np.stack([2 * (bd + ac), 2 * (cd - ab), aa + dd - bb - cc], -1)], -2)
    return np.einsum('...ij,...j', R, v)


def orientation(pos, cluster_size, ndim, mpp=1., sizes=None, angles=None):
    """pos [T, F, cluster_size, ndim] (z,) y, x; returns com [T, F, 3], bases [T, P, F, 3, 3]"""
    pos = np.asarray(pos, dtype=np.float64)
    T, F = pos.shape[:2]
    perms = PERMUTATIONS[cluster_size]
    w = np.ones(cluster_size) if sizes is None else np.asarray(sizes, dtype=np.float64) ** ndim
    c = np.zeros((T, F, cluster_size, 3))
    c[..., :ndim] = (pos * mpp)[..., ::-1]
    present = np.isfinite(c).all((-1, -2))
    com = np.full((T, F, 3), np.nan)
    bases = np.full((T, len(perms), F, 3, 3), np.nan)
    for p, perm in enumerate(perms):
        cp = c[:, :, perm]
        s = np.zeros((T, F, 3))
        for k in range(cluster_size):               # np.sum over the features, in their order
            s = s + cp[:, :, k] * w[k]
        com_p = s / w.sum()
        if ndim == 2:
            x = _unit(cp[:, :, 0] - com_p)
            z = np.zeros((T, F, 3))
            z[..., 2] = 1.
        else:
            z = _unit(cp[:, :, 0] - com_p)
            if cluster_size == 2:
                v = np.cross(np.array([1., 0., 0.]), z)
                x = _rotate_about(z, np.asarray(angles, dtype=np.float64)[:, p], v)
            elif cluster_size == 3:
                x = np.cross(z, cp[:, :, 1] - com_p)
            else:
                x = np.cross(z, cp[:, :, 2] - cp[:, :, 1])
            x = _unit(x)
        y = _unit(np.cross(z, x))
        B = np.stack([x, y, z], -2)
        good = present & np.isfinite(B).all((-1, -2))
        B[~good] = np.nan
        bases[:, p] = B
        com = np.where(present[..., None], com_p, np.nan)      # the last permutation's stays
    return com, bases


# ---- diffusion tensor --------------------------------------------------------------------------
def displacements(positions, bases, lag):
    """positions [F, 3], bases [P, F, 3, 3]: the pooled 6-vectors [n, 6] of one track and lag"""
    F = positions.shape[0]
    if lag >= F:
        return np.zeros((0, 6))
    dp = positions[lag:] - positions[:-lag]
    B, C = bases[:, :-lag], bases[:, lag:]
    with np.errstate(invalid='ignore'):
        tr = np.einsum('pbij,bj->pbi', B, dp)
        M = np.einsum('pbkj,pbij->pbki', B, C)          # M[k, i] = (B C[i])_k
        rot = 0.5 * np.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], -1)
    x = np.concatenate([tr, rot], -1).reshape(-1, 6)
    return x[np.isfinite(x).all(1)]


def diffusion_tensor(positions, bases, lags, fps=1., ndim=3):
    """positions [T, F, 3], bases [T, P, F, 3, 3], lags [L]: tensor [T, L, D, D], counts [T, L]"""
    positions, bases = np.asarray(positions, dtype=np.float64), np.asarray(bases, dtype=np.float64)
    T, D = positions.shape[0], 3 if ndim == 2 else 6
    tensor = np.full((T, len(lags), D, D), np.nan)
    counts = np.zeros((T, len(lags)), dtype=np.int64)
    for t in range(T):
        for i, lag in enumerate(lags):
            x = displacements(positions[t], bases[t], int(lag))
            if ndim == 2:
                x = x[:, [0, 1, 5]]
            counts[t, i] = len(x)
            if len(x):
                tensor[t, i] = (x[:, :, None] * x[:, None, :]).mean(0) * 0.5 / (lag / fps)
    return tensor, counts


# ---- the fixtures of tests/golden/make_golden_motion.py ------------------------------------------
def load_cases():
    """[dict(name, ndim, cluster_size, mpp, fps, sizes, angles, table, com, bases, lags, tensors)]"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'motion', 'motion_cases.npz'))
    cases = []
    for name in sorted({k.split('__')[0] for k in z.files}):
        ndim, cluster_size, mpp, fps = z[name + '__meta']
        sizes = z[name + '__sizes']
        cases.append(dict(name=name, ndim=int(ndim), cluster_size=int(cluster_size), mpp=float(mpp), fps=float(fps),
                          sizes=None if len(sizes) == 0 else sizes,
                          angles=z[name + '__angles'] if name + '__angles' in z.files else None,
                          table=z[name + '__table'], com=z[name + '__com'], bases=z[name + '__bases'],
                          lags=z[name + '__lags'], tensors=z[name + '__tensors']))
    return cases


def table_frame(case):
    """the case's table as the DataFrame orientation_df takes"""
    import pandas as pd
    return pd.DataFrame(case['table'], columns=['frame', 'cluster', 'particle'] + ['z', 'y', 'x'][3 - case['ndim']:])


def dense_from_table(case):
    """pos [1, F, cluster_size, ndim] of the case's table, built without pandas: rows ordered by
    (frame, cluster, particle), a frame with exactly cluster_size rows counts"""
    tab = case['table']
    tab = tab[np.lexsort((tab[:, 2], tab[:, 1], tab[:, 0]))]
    frame = tab[:, 0].astype(np.int64) - int(tab[:, 0].min())
    dense = np.full((1, int(frame.max()) + 1, case['cluster_size'], case['ndim']), np.nan)
    for f in np.unique(frame):
        rows = tab[frame == f]
        if len(rows) == case['cluster_size']:
            dense[0, f] = rows[:, 3:]
    return dense


def assert_same(got, want, atol, what=''):
    """equal NaN pattern, finite values within atol"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (np.isnan(got) == np.isnan(want)).all(), what
    ok = np.isfinite(want)
    if ok.any():
        err = np.abs(got[ok] - want[ok]).max()
        assert err <= atol, (what, err, atol)


def assert_tensors(got, want, what=''):
    """every [D, D] tensor within 1e-10 of its largest entry (sums of float64 terms: n eps is far
    below), NaN tensors NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.reshape(-1, got.shape[-1] ** 2), want.reshape(-1, want.shape[-1] ** 2)
    for i in range(len(w)):
        if np.isnan(w[i]).all():
            assert np.isnan(g[i]).all(), (what, i)
        else:
            assert np.isfinite(w[i]).all() and np.isfinite(g[i]).all(), (what, i)
            err, top = np.abs(g[i] - w[i]).max(), np.abs(w[i]).max()
            assert err <= 1e-10 * top, (what, i, err, top)
