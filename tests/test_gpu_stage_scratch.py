"""The scratch blocks of an engine handle that stages share (ctrefine.hip: Scratch, reserve,
run_stage): a block that has to grow between two calls, and the block that the diffusion tensor and
its bootstrap interval both use.  A small call gives the same bytes before and after; the calls in
between pass the assertions of their own tests (tests/_motion.py, tests/_motion_ci.py, the host
linker)."""
import numpy as np
import pytest

import _motion as M
import _motion_ci as C
from clustertracking_amd import link as lk
from clustertracking_amd import motion, motion_ci

pytestmark = pytest.mark.gpu


def _track(rng, T, F, P):
    return rng.normal(0., 1., (T, F, 3)).cumsum(1), rng.normal(0., 1., (T, P, F, 3, 3))


def test_diffusion_scratch_grows_and_is_shared(engine):
    rng = np.random.RandomState(3)
    small, large = _track(rng, 2, 16, 2), _track(rng, 8, 600, 2)          # 2D dimers: two permutations
    lags, lags_large, fps, B = [1, 2], [1, 2, 300], 10., 64
    first, n_first = motion.diffusion_tensor(*small, lags, fps, 2, return_counts=True)
    grown, n_grown = motion.diffusion_tensor(*large, lags_large, fps, 2, return_counts=True)
    interval, det = motion_ci.diffusion_tensor_ci(*small, lags, fps, 2, n_samples=B, return_details=True)
    last, n_last = motion.diffusion_tensor(*small, lags, fps, 2, return_counts=True)
    assert first.tobytes() == last.tobytes() and n_first.tobytes() == n_last.tobytes()
    for got, n_got, (positions, bases), ks in ((first, n_first, small, lags), (grown, n_grown, large, lags_large)):
        want, want_n = M.diffusion_tensor(positions, bases, ks, fps, 2)
        assert (n_got == want_n).all() and (want_n > 0).all()
        M.assert_tensors(got, want)
    for at in np.ndindex(2, len(lags)):
        res = C.ci(C.rows(small[0][at[0]], small[1][at[0]], lags[at[1]], 2), lags[at[1]], fps, 0.05, B, 'bca', 0)
        C.assert_conditions(res, B)
        C.assert_matches((interval[at], {k: v[at] for k, v in det.items()}), res, B, what=at)


def _walkers(rng, n, n_levels, step=0.5):
    pos = rng.uniform(0., 400., (n, 2))
    levels = []
    for _ in range(n_levels):
        pos = pos + rng.normal(0., step, pos.shape)
        levels.append(pos[rng.permutation(n)])
    return np.concatenate(levels), np.arange(n_levels + 1) * n, levels


def test_link_scratch_grows(engine):
    rng = np.random.RandomState(4)
    small, large = _walkers(rng, 4, 2), _walkers(rng, 64, 40)
    first = lk.link_arrays(small[0], small[1], 3.)
    grown = lk.link_arrays(large[0], large[1], 3.)
    last = lk.link_arrays(small[0], small[1], 3.)
    assert first.dtype == np.int64 and (first == last).all()
    for got, (_, _, levels) in ((first, small), (grown, large)):
        assert (got == np.concatenate(lk.link_levels(levels, 3.))).all()
        assert got.max() == len(levels[0]) - 1                  # every walker keeps its track


@pytest.mark.parametrize('n_levels', [255, 256, 257, 513])
def test_link_levels_at_the_chunk_of_the_scan(engine, n_levels):
    """three walkers whose steps leave the search range now and then, so tracks start at many levels:
    the first ids of the levels are scanned by one workgroup in chunks of 256 levels"""
    pos, off, levels = _walkers(np.random.RandomState(n_levels), 3, n_levels, step=1.5)
    want = np.concatenate(lk.link_levels(levels, 3.))
    assert want[-3:].max() > n_levels // 20               # tracks still start near the end
    got = lk.link_arrays(pos, off, 3.)
    assert got.dtype == np.int64 and (got == want).all()
