"""Writes tests/golden/motion/motion_cases.npz: what the REFERENCE's motion.orientation_df and
motion.diffusion_tensor give for one cluster track per geometry (2D dimer and trimer, 3D trimer,
tetramer and dimer), through oracle/refshim.py.  Runs only where the reference is present; the
file holds data only.

Per case: about 40 frames that start at a non-zero frame number, non-unit mpp, unequal sizes (one
more 2D trimer case has sizes=None), two frames without rows, one frame with a feature missing,
features several pixels apart.  The tensors are taken at lags 1, 3 and F - 1 (the first and the
last frame are complete, so that lag has one row per permutation).  For the 3D dimer np.random is
seeded and every draw of the reference is recorded in call order: 2 pi draw is the azimuth of
(frame, permutation), stored as angles [P, F].

Keys, per case name: <name>__table [N, 3 + ndim] (frame, cluster, particle, (z,) y, x; rows
shuffled), __meta (ndim, cluster_size, mpp, fps), __sizes (empty: None), __angles [P, F] (3D dimer),
__com [F, 3], __bases [P, F, 3, 3], __lags [3], __tensors [3, D, D].
"""
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'oracle'))

import refshim  # noqa: E402

SHAPES = {      # feature positions of the rigid cluster, in pixels, x, y, z
    2: np.array([[-2.5, 0., 0.], [2.5, 0., 0.]]),
    3: np.array([[0., 3., 0.], [-2.6, -1.5, 0.], [2.6, -1.5, 0.]]),
    4: np.array([[3., 3., 3.], [3., -3., -3.], [-3., 3., -3.], [-3., -3., 3.]]) * 0.7,
}
CASES = [   # name, ndim, cluster_size, mpp, fps, sizes, seed
    ('d2_dimer', 2, 2, 0.21, 15., [1.0, 1.3], 11),
    ('d2_trimer', 2, 3, 0.21, 15., [1.0, 1.2, 0.9], 12),
    ('d2_trimer_equal', 2, 3, 0.5, 7., None, 13),
    ('d3_trimer', 3, 3, 0.33, 30., [1.1, 0.8, 1.0], 14),
    ('d3_tetramer', 3, 4, 0.33, 30., [1.0, 1.2, 0.9, 1.1], 15),
    ('d3_dimer', 3, 2, 0.4, 10., [0.9, 1.4], 16),
]
N_FRAMES, FIRST, NO_ROWS, ONE_SHORT = 40, 7, (12, 25), 18


def random_rotation(rng, ndim, step):
    if ndim == 2:
        a = rng.normal(0., step)
        return np.array([[np.cos(a), -np.sin(a), 0.], [np.sin(a), np.cos(a), 0.], [0., 0., 1.]])
    v = rng.normal(0., step, 3)
    K = np.array([[0., -v[2], v[1]], [v[2], 0., -v[0]], [-v[1], v[0], 0.]])
    t = np.sqrt((v * v).sum())
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / t ** 2 * K.dot(K)


def make_table(rng, ndim, cluster_size):
    shape = SHAPES[cluster_size].copy()
    centre = np.array([60., 50., 40.])
    R = random_rotation(rng, ndim, 2.)
    rows = []
    for t in range(N_FRAMES):
        R = random_rotation(rng, ndim, 0.15).dot(R)
        centre = centre + rng.normal(0., 0.4, 3) * ([1, 1, 0] if ndim == 2 else [1, 1, 1])
        xyz = shape.dot(R.T) + centre + rng.normal(0., 0.05, shape.shape)
        if t in NO_ROWS:
            continue
        for k in range(cluster_size):
            if t == ONE_SHORT and k == 1:
                continue
            rows.append([FIRST + t, 5, 10 + k] + list(xyz[k, :ndim][::-1]))
    table = np.array(rows)
    return table[rng.permutation(len(table))]


def run_reference(motion, table, ndim, cluster_size, mpp, fps, sizes, seed):
    f = pd.DataFrame(table, columns=['frame', 'cluster', 'particle'] + ['z', 'y', 'x'][3 - ndim:])
    draws = []
    real = np.random.random

    def recording(*args):
        v = real(*args)
        draws.append(v)
        return v
    np.random.seed(seed)
    np.random.random = recording
    try:
        com, bases = motion.orientation_df(f, cluster_size, mpp, ndim, sizes)
    finally:
        np.random.random = real
    F, P = len(com), len(bases)
    out = dict(com=com, bases=bases)
    if draws:       # call order: frames that qualify, rising; per frame the permutations
        frames = np.flatnonzero(np.isfinite(com).all(1))
        assert len(draws) == len(frames) * P
        angles = np.zeros((P, F))
        angles[:, frames] = (np.array(draws) * 2 * np.pi).reshape(len(frames), P).T
        out['angles'] = angles
    lags = np.array([1, 3, F - 1])
    out['lags'] = lags
    out['tensors'] = np.stack([motion.diffusion_tensor(com, bases, int(lag), fps, ndim) for lag in lags])
    return out


def main():
    refshim.load()
    import clustertracking.motion as motion
    data = {}
    for name, ndim, cluster_size, mpp, fps, sizes, seed in CASES:
        rng = np.random.RandomState(seed)
        table = make_table(rng, ndim, cluster_size)
        res = run_reference(motion, table, ndim, cluster_size, mpp, fps, sizes, seed)
        assert len(res['com']) == N_FRAMES and np.isfinite(res['tensors']).all()
        data[name + '__table'] = table
        data[name + '__meta'] = np.array([ndim, cluster_size, mpp, fps])
        data[name + '__sizes'] = np.zeros(0) if sizes is None else np.array(sizes, dtype=np.float64)
        for k, v in res.items():
            data[name + '__' + k] = v
    os.makedirs(os.path.join(HERE, 'motion'), exist_ok=True)
    out = os.path.join(HERE, 'motion', 'motion_cases.npz')
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
