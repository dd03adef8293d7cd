"""Every kernel cell of the dispatch (tests/_dispatch.py) against the C oracle, at the edges of
its tile band.  Needs a real MI355X.

Per cell: status equal; cost to rtol 1e-7 (atol 1e-12); positions to 1e-6 px and every parameter
to rtol = atol = 1e-6 on clusters with status 0; params_std (compute_error) with equal NaN sets and
finite values to rtol 1e-6 where the oracle gives it (gaussian, not the large-cluster path), NaN
from the engine elsewhere.  Per problem type, every cell's clusters in one shuffled batch give
what each cluster gives alone to 1e-12.  Clusters beyond the engine get status 5 and leave their
neighbours in the batch alone."""

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_equal

import _dispatch as D
from clustertracking_amd import _abi

pytestmark = pytest.mark.gpu

CELLS = {D.cell_id(c): c for c in D.launchable_cells()}


def clone(b):
    return _abi.HostBatch(b.frames, b.frame_index, b.feat_offset, b.params, b.low, b.high,
                          want_std=b.params_std is not None)


def std_from_oracle(cell):
    """The oracle gives params_std for the gaussian; the engine not on the large-cluster path."""
    return cell.family not in ('ring', 'disc', 'inv_series', 'large', 'large_lowpass')


def assert_engine_matches_oracle(b, ref, nd, with_std, what):
    assert_equal(b.status, ref.status, err_msg=what)
    ok = b.status == 0
    assert np.isnan(b.cost[~ok]).all() and np.isnan(ref.cost[~ok]).all()
    assert_allclose(b.cost[ok], ref.cost[ok], rtol=1e-7, atol=1e-12, err_msg=what)
    rows = np.repeat(ok, np.diff(b.feat_offset))
    d = np.abs(b.params_out[rows, 2:2 + nd] - ref.params_out[rows, 2:2 + nd])
    assert d.size == 0 or d.max() < 1e-6, (what, d.max())
    assert_allclose(b.params_out[rows], ref.params_out[rows], rtol=1e-6, atol=1e-6, err_msg=what)
    assert_equal(b.params_out[~rows], b.params[~rows])
    if with_std:
        assert_equal(np.isnan(b.params_std), np.isnan(ref.params_std), err_msg=what)
        fin = ~np.isnan(ref.params_std)
        assert_allclose(b.params_std[fin], ref.params_std[fin], rtol=1e-6, err_msg=what)
    else:
        assert np.isnan(b.params_std).all(), what


@pytest.mark.parametrize('cid', sorted(CELLS))
def test_cell_engine_vs_oracle(engine, oracle, cid):
    cell = CELLS[cid]
    for case in D.build_case(cell):
        prep = case.prepare(compute_error=True)
        b, ref = clone(prep.batch), clone(prep.batch)
        engine.refine_batch(prep.problem, b)
        oracle.run_batch(prep.problem, ref)
        assert (ref.status == 0).all()
        assert_engine_matches_oracle(b, ref, cell.ndim, std_from_oracle(cell),
                                     '%s n=%s' % (cid, case.n_features))


# ---- one batch per problem type ---------------------------------------------------------------

def sub_batch(b, order):
    """The clusters `order` of batch b, in that order, as a batch of their own."""
    rows = np.concatenate([np.arange(b.feat_offset[c], b.feat_offset[c + 1]) for c in order])
    off = np.concatenate([[0], np.cumsum(np.diff(b.feat_offset)[order])])
    return _abi.HostBatch(b.frames, b.frame_index[order], off, b.params[rows], b.low[rows],
                          b.high[rows], want_std=True)


@pytest.mark.parametrize('t', D.problem_types(), ids=lambda t: t.name)
def test_problem_type_in_one_batch_equals_per_cluster(engine, t):
    """Every cell one problem type reaches, in ONE call with the clusters in shuffled order, gives
    what each cluster gives alone: the bins launched together, the work counters and
    front_load_kernel's order change nothing."""
    from clustertracking_amd import _lib
    prep = D.build_type_case(t).prepare(compute_error=True)
    hb = prep.batch
    kinds = {(k.bin, k.nt) for k in (_lib.cluster_kernel(prep.problem, int(n)) for n in np.diff(hb.feat_offset))}
    assert {(_abi.KBIN_BLOCK, nt) for nt in range(1, 9)} <= kinds and any(b == _abi.KBIN_CONS for b, _ in kinds)
    perm = np.random.RandomState(7).permutation(hb.n_clusters)
    m = sub_batch(hb, perm)
    engine.refine_batch(prep.problem, m)
    for k, c in enumerate(perm):
        a = sub_batch(hb, [c])
        engine.refine_batch(prep.problem, a)
        rm = slice(m.feat_offset[k], m.feat_offset[k + 1])
        what = '%s cluster %d (n=%d)' % (t.name, c, a.n_features)
        assert m.status[k] == a.status[0], what
        assert m.n_iter[k] == a.n_iter[0], what
        assert_allclose(m.cost[k], a.cost[0], rtol=1e-12, atol=0, equal_nan=True, err_msg=what)
        assert_allclose(m.params_out[rm], a.params_out, rtol=0, atol=1e-12, err_msg=what)
        assert_allclose(m.params_std[rm], a.params_std, rtol=1e-12, atol=0, equal_nan=True, err_msg=what)


# ---- beyond the engine ------------------------------------------------------------------------

@pytest.mark.parametrize('tl', D.TOO_LARGE_CELLS, ids=lambda t: t.name)
def test_too_large_status_5_neighbours_unaffected(engine, oracle, tl):
    prep = D.build_too_large(tl).prepare(compute_error=True)
    b, ref = clone(prep.batch), clone(prep.batch)
    engine.refine_batch(prep.problem, b)
    oracle.run_batch(prep.problem, ref)
    r0 = slice(b.feat_offset[0], b.feat_offset[1])
    assert b.status[0] == _abi.STATUS_TOO_LARGE
    assert np.isnan(b.cost[0]) and np.isnan(b.params_std[r0]).all()
    assert_equal(b.params_out[r0], b.params[r0])
    # the ordinary cluster of the same call
    one = lambda x: _abi.HostBatch(x.frames, x.frame_index[1:], x.feat_offset[1:] - x.feat_offset[1],
                                   x.params[x.feat_offset[1]:], x.low[x.feat_offset[1]:],
                                   x.high[x.feat_offset[1]:], want_std=True)
    bo, ro = one(b), one(ref)
    for name in ('params_out', 'params_std'):
        getattr(bo, name)[:] = getattr(b, name)[b.feat_offset[1]:]
        getattr(ro, name)[:] = getattr(ref, name)[ref.feat_offset[1]:]
    for x, y in ((bo, b), (ro, ref)):
        x.status[:], x.cost[:] = y.status[1:], y.cost[1:]
    assert ro.status[0] == 0
    assert_engine_matches_oracle(bo, ro, tl.ndim, tl.profile == 'gauss', tl.name)
