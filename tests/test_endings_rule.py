"""The oracle against the table of tests/_endings.py on every launchable cell of the dispatch: how
a fit ends other than converged.  No GPU.  The expectations are written out here, not read back
from the oracle; tests/test_gpu_endings.py then holds every kernel family to the same oracle runs.

An empty bound interval on a free variable (low > high) is status 3, the solver's failure
(include/ctrefine.h; SciPy raises on such a box), with n_rounds 1, n_iter 0 and the outputs of any
failed cluster.

Not tested: the ``gain <= CTR_STALL_TOL`` edge and the ``mu > 1e30`` exit.  Neither can be reached
by a case that the input decides.
"""
import numpy as np
import pytest

import _dispatch as D
import _endings as E
from clustertracking_amd import _abi

GEOM_IDS = ['%dd-%s' % (nd, 'iso' if iso else 'aniso') for nd, iso in D.GEOMS]


def cells_of(geom):
    return [cid for cid in E.CELLS if ('-%s-' % geom) in cid or cid.endswith('-' + geom)]


def test_every_cell_has_a_geometry():
    assert sorted(sum((cells_of(g) for g in GEOM_IDS), [])) == sorted(E.CELLS)
    assert len(E.CELLS) == len(D.launchable_cells())


def check_failed(hb, c, status, n_iter, n_rounds, what):
    assert (hb.status[c], hb.n_iter[c], hb.n_rounds[c]) == (status, n_iter, n_rounds), what
    assert E.failed_outputs_ok(hb, c), what


def check_case(cid, calls, seen):
    cols, pc, names = calls.cols, calls.per_cluster, calls.names
    x = cols.pos[-1]
    assert names[0] is None and names[-1] is None
    assert pc.status[0] == 0 and pc.n_rounds[0] >= 1 and pc.n_iter[0] >= 1 and np.isfinite(pc.cost[0]), cid
    # the unedited copies: first, last, and alone
    assert E.same_bytes(pc, 0, pc, len(names) - 1), cid
    assert E.same_bytes(pc, 0, calls.alone, 0) and E.same_bytes(pc, 0, calls.alone, calls.alone.n_clusters - 1), cid
    n = int(pc.feat_offset[1])
    for k, name in enumerate(names):
        if name is None:
            assert E.same_bytes(pc, 0, pc, k), (cid, k)
            continue
        seen.add(name)
        what = '%s %s' % (cid, name)
        r = E.rows_of(pc, k)
        if name in E.FAILS:
            check_failed(pc, k, *E.FAILS[name], what=what)
            assert name != 'nonfinite' or np.isnan(pc.params_out[r.stop - 1, 1]), what
        elif name == 'empty_interval_const':
            assert E.same_bytes(pc, 0, pc, k), what
        elif name == 'bound_active':
            assert pc.status[k] == 0 and pc.n_rounds[k] >= 1, what
            excess = pc.params_out[r, x] - pc.high[r, x]
            if cols.constrained(n):
                assert excess.max() < 1e-9, (what, excess.max())   # (the retraction's own tolerance)
            else:
                assert pc.params_out[r, x].tobytes() == pc.high[r, x].tobytes(), (what, excess)
        elif name == 'start_clipped':
            assert pc.status[k] == 0 and pc.n_rounds[k] >= 1, what
            assert pc.params_out[r.stop - 1, x] - pc.high[r.stop - 1, x] < (1e-9 if cols.constrained(n) else 1e-300), what
            # the other columns of the last feature, and the other features, fit as they did
            d = np.abs(pc.params_out[r, cols.pos[0]:x + 1] - pc.params_out[E.rows_of(pc, 0), cols.pos[0]:x + 1])
            assert d[:-1].max(initial=0.) < 0.5 and d[-1, :-1].max(initial=0.) < 0.5, (what, d)
        else:
            raise AssertionError(name)
    # per-call endings: both copies alike
    unedited = calls.alone
    for name in E.PER_CALL:
        seen.add(name)
        p, hb = calls.per_call[name]
        what = '%s %s' % (cid, name)
        assert E.same_bytes(hb, 0, hb, hb.n_clusters - 1), what
        for c in range(hb.n_clusters):
            if name == 'solver_limit':
                assert p.solver_maxiter == 2
                check_failed(hb, c, _abi.STATUS_NO_CONVERGENCE, 2, 1, what)
            elif name == 'rms':
                assert unedited.cost[0] > 0 and p.max_rms_dev == 0.5 * unedited.cost[0]
                check_failed(hb, c, _abi.STATUS_RMS_DEV, unedited.n_iter[0], unedited.n_rounds[0], what)
            elif name == 'round_cap':
                assert (hb.status[c], hb.n_rounds[c]) == (0, 1) and np.isfinite(hb.cost[c]), what
            elif name == 'two_rounds':
                assert (hb.status[c], hb.n_rounds[c]) == (0, 2) and np.isfinite(hb.cost[c]), what
    # the stability conditions behind round_cap and two_rounds, measured again on the results
    start = calls.per_call['round_cap'][1].params
    one, two = calls.per_call['round_cap'][1].params_out, calls.per_call['two_rounds'][1].params_out
    assert E.shift_of(one, start, cols).max() > 2 * E.SMALL_SHIFT, cid
    assert E.shift_of(two, one, cols).max() < E.SMALL_SHIFT / 2, cid


@pytest.mark.parametrize('geom', GEOM_IDS)
def test_oracle_endings_of_every_cell(oracle, geom):
    seen = set()
    cids = cells_of(geom)
    assert cids
    fetched = E.prefetch(oracle, cids)      # (raises where an expectation is not stable)
    for cid in cids:
        cases = fetched[cid]
        assert cases
        for calls in cases:
            check_case(cid, calls, seen)
    assert seen == set(E.PER_CLUSTER) | set(E.PER_CALL), sorted(seen)


def test_empty_interval_is_the_solvers_failure(oracle):
    """low > high on a free variable: status 3 with n_rounds 1, n_iter 0, outputs equal to the
    start; one on a const column changes nothing"""
    cid = 'small-2d-iso-single-8lanes'
    prep = D.build_case(E.CELLS[cid])[0].prepare(compute_error=True)
    cols = E.Columns(prep.problem)
    hb = E.copies(prep.batch, 0, 3)
    E.apply(hb, 1, 'empty_interval', cols)
    E.apply(hb, 2, 'empty_interval_const', cols)
    oracle.run_batch(prep.problem, hb)
    assert list(hb.status) == [0, _abi.STATUS_NO_CONVERGENCE, 0]
    assert list(hb.n_rounds[1:2]) == [1] and list(hb.n_iter[1:2]) == [0]
    assert E.failed_outputs_ok(hb, 1)
    assert E.same_bytes(hb, 0, hb, 2)
