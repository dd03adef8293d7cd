"""Edge-case golden vectors for the linkers from the REFERENCE's ``Linker`` class
(clustertracking/find_link.py:579-733), run through oracle/refshim.py in the build
container:  python tests/golden/make_golden_link_edges.py

Empty levels (in the middle, in a row, at the start), a single level, one feature per level and
integer positions, with and without memory.  Layout as link_cases.npz.  Every case is asserted
to be reproduced by ``link.link_levels`` before it is saved: these are sparse inputs, where the
reference's recursion is optimal."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, HERE)
from make_golden_link import random_walkers, reference_ids  # noqa: E402  (loads the reference)

from clustertracking_amd import link as lk  # noqa: E402


def with_empty(levels, which):
    return [np.zeros((0, lv.shape[1])) if t in which else lv for t, lv in enumerate(levels)]


def main():
    rng = np.random.RandomState(321)
    w2 = lambda n, frames, p_drop=0.: random_walkers(rng, n, frames, 2, 300., 1.0, p_drop, 0.5)
    cases = {
        'empty_mid_m0': (with_empty(w2(30, 8), {4}), (5., 5.), 0),
        'empty_mid_m2': (with_empty(w2(30, 8, 0.1), {4}), (5., 5.), 2),
        'empty_two_m2': (with_empty(w2(30, 9, 0.1), {3, 4}), (5., 5.), 2),       # a gap of exactly memory
        'empty_three_m2': (with_empty(w2(30, 10, 0.1), {3, 4, 5}), (5., 5.), 2),  # memory + 1
        'empty_first_m0': (with_empty(w2(20, 6), {0}), (5., 5.), 0),
        'empty_first_m1': (with_empty(w2(20, 6, 0.1), {0}), (5., 5.), 1),
        'single_level': (w2(25, 1), (5., 5.), 0),
        'one_per_level_m0': (random_walkers(rng, 1, 10, 2, 50., 1.0, 0., 0.), (5., 5.), 0),
        'one_per_level_m2': (random_walkers(rng, 1, 12, 2, 50., 1.0, 0.3, 0.), (5., 5.), 2),
        'one_per_level_3d': (random_walkers(rng, 1, 8, 3, 50., 1.0, 0., 0.), (4., 5., 5.), 1),
        'integer_m0': ([np.round(lv) for lv in random_walkers(rng, 25, 8, 2, 400., 1.0, 0., 0.5)], (4., 4.), 0),
        'integer_m1': ([np.round(lv) for lv in random_walkers(rng, 25, 8, 2, 400., 1.0, 0.1, 0.5)], (4., 4.), 1),
    }
    out = {}
    for name, (levels, sr, memory) in cases.items():
        ids = reference_ids(levels, sr, memory)
        ours = lk.link_levels(levels, sr, memory)
        for a, b in zip(ids, ours):
            np.testing.assert_array_equal(a, b, err_msg=name)
        counts = np.array([len(l) for l in levels])
        ndim = len(sr)
        out[name + '_pos'] = np.concatenate([l.reshape(-1, ndim) for l in levels])
        out[name + '_counts'] = counts
        out[name + '_sr'] = np.array(sr)
        out[name + '_memory'] = np.array(memory)
        out[name + '_ids'] = (np.concatenate(ids) if counts.sum() else np.zeros(0)).astype(np.int64)
        print(name, 'levels', len(levels), 'points', counts.sum(), 'tracks', len(set(out[name + '_ids'])))
    np.savez_compressed(os.path.join(HERE, 'link', 'link_edge_cases.npz'), **out)


if __name__ == '__main__':
    main()
