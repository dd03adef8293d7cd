"""Every refine kernel family where a fit ends other than converged (tests/_endings.py; DESIGN.md,
"how a fit ends"), against the C oracle.  Needs a real MI355X.

Per cell of the dispatch (tests/_dispatch.py): one call with a copy of the cell's cluster per
ending between two unedited copies, and one call per setting of the problem (solver_limit, rms,
round_cap, two_rounds).  status and n_rounds equal the oracle's everywhere; n_iter where the table
gives a number (0, 2) and is printed beside the oracle's elsewhere; a failed cluster has cost NaN,
params_out the bytes of params and params_std all NaN; a cluster that fits is held to the bounds
of tests/test_gpu_dispatch_matrix.py (cost rtol 1e-7, positions 1e-6 px, parameters 1e-6,
params_std rtol 1e-6); bound_active ends bitwise on the bound where no constraint retracts it; the
unedited copies have the bytes of each other and of a call without any edited copy.

Then where clusters share execution state -- lane groups of a wavefront that pull their next
cluster (small kernels), the workgroups of the tail launch that loop over entries, the bins of one
call: the same cluster list twice, once with every third cluster edited, once as it is.  Every
unedited cluster has the same bytes in both calls, every edited one matches the oracle.

Each test prints the largest position and cost difference of its fits against the oracle.

Not tested: the ``gain <= CTR_STALL_TOL`` edge, on which engine and oracle differ in the last bits,
and the ``mu > 1e30`` exit.  Neither can be reached by a case that the input decides.
"""
import numpy as np
import pytest

import clustertracking_amd as cta
import _dispatch as D
import _endings as E
from clustertracking_amd import _abi, _lib
from test_gpu_dispatch_matrix import assert_engine_matches_oracle
from test_gpu_tail_absorb import NT1, NT2, PAIRS, absorb
from test_gpu_tail_fusion import DIAMETER, _cap, draw

pytestmark = pytest.mark.gpu


def oracle_gives_std(problem, n_features):
    """the oracle gives params_std for the gaussian; the engine not on the large-cluster path"""
    return problem.fit_function == _abi.FIT_GAUSS and \
        _lib.cluster_kernel(problem, n_features).bin != _abi.KBIN_LARGE


def figures(got, ref, cols):
    """(max |dpos| px, max relative dcost) over the clusters that fit"""
    ok = (got.status == 0) & (ref.status == 0)
    rows = np.repeat(ok, np.diff(got.feat_offset))
    sl = slice(cols.pos[0], cols.pos[-1] + 1)
    dp = np.abs(got.params_out[rows, sl] - ref.params_out[rows, sl])
    dc = np.abs(got.cost[ok] - ref.cost[ok]) / np.abs(ref.cost[ok])
    return (dp.max() if dp.size else 0.), (dc.max() if dc.size else 0.)


def check_against_oracle(got, ref, problem, cols, names, what, n_iter_of=None, every_bound=False):
    """got: the engine's batch, ref: the oracle's, names[c]: the ending of cluster c or None.
    bound_active without a constraint: the engine ends bitwise on the bound where the oracle does;
    with every_bound on every feature (the cells: tests/test_endings_rule.py holds the oracle to it)"""
    assert list(got.status) == list(ref.status), what
    assert list(got.n_rounds) == list(ref.n_rounds), what
    for c, name in enumerate(names):
        n = int(got.feat_offset[c + 1] - got.feat_offset[c])
        r = E.rows_of(got, c)
        if name in E.FAILS:
            assert (got.status[c], got.n_iter[c], got.n_rounds[c]) == E.FAILS[name], (what, c, name)
        if n_iter_of is not None:
            assert got.n_iter[c] == n_iter_of, (what, c, name)
        if got.status[c] != 0:
            assert E.failed_outputs_ok(got, c), (what, c, name)
        if name == 'bound_active' and not cols.constrained(n):
            x = cols.pos[-1]
            at = ref.params_out[r, x] == ref.high[r, x]
            assert got.status[c] == 0 and (at.all() or not every_bound) and at.any(), (what, c, at)
            assert got.params_out[r, x][at].tobytes() == got.high[r, x][at].tobytes(), (what, c, got.params_out[r, x] - got.high[r, x])
    # the clusters that fit, by whether the oracle gives their params_std
    sizes = np.diff(got.feat_offset)
    for with_std in (True, False):
        idx = [c for c in range(got.n_clusters) if oracle_gives_std(problem, int(sizes[c])) == with_std]
        if idx:
            assert_engine_matches_oracle(E.subset(got, idx, True), E.subset(ref, idx, True), cols.nd, with_std, what)
    free = [(c, names[c], int(got.n_iter[c]), int(ref.n_iter[c])) for c in range(got.n_clusters)
            if names[c] not in E.FAILS and got.n_iter[c] != ref.n_iter[c]]
    dp, dc = figures(got, ref, cols)
    print('endings %s: max |dpos| %.3g px, max rel dcost %.3g%s' % (
        what, dp, dc, '; n_iter (cluster, ending, engine, oracle) %s' % free[:6] if free else ''))


# ---- every cell ------------------------------------------------------------------------------------

@pytest.mark.parametrize('cid', sorted(E.CELLS))
def test_cell_endings_engine_vs_oracle(engine, oracle, cid):
    for k, calls in enumerate(E.calls_of(oracle, cid)):
        problem, cols, names = calls.problem, calls.cols, calls.names
        what = '%s case %d' % (cid, k)
        got = E.clone(calls.per_cluster)
        engine.refine_batch(problem, got)
        check_against_oracle(got, calls.per_cluster, problem, cols, names, what + ' per-cluster', every_bound=True)
        alone = E.clone(calls.alone)
        engine.refine_batch(problem, alone)
        assert alone.status[0] == 0
        for c, name in enumerate(names):    # nothing of a failed neighbour shows
            if name is None or name == 'empty_interval_const':
                assert E.same_bytes(got, c, alone, 0), (what, c, name)
        assert E.same_bytes(alone, 0, alone, alone.n_clusters - 1), what
        for name in E.PER_CALL:
            p, ref = calls.per_call[name]
            hb = E.clone(ref)
            engine.refine_batch(p, hb)
            check_against_oracle(hb, ref, p, cols, [None] * hb.n_clusters, '%s %s' % (what, name),
                                 n_iter_of=2 if name == 'solver_limit' else None)
            assert E.same_bytes(hb, 0, hb, hb.n_clusters - 1), (what, name)
            want = {'solver_limit': (_abi.STATUS_NO_CONVERGENCE, 1), 'rms': (_abi.STATUS_RMS_DEV, int(calls.alone.n_rounds[0])),
                    'round_cap': (0, 1), 'two_rounds': (0, 2)}[name]
            assert all((s, r) == want for s, r in zip(hb.status, hb.n_rounds)), (what, name, hb.status, hb.n_rounds)


# ---- clusters that share execution state --------------------------------------------------------------

def edited_against_plain(engine, oracle, problem, hb, what):
    """hb twice: with every third cluster edited and as it is"""
    run = lambda b: engine.refine_batch(problem, b)
    cols = E.Columns(problem)
    plain = E.clone(hb)
    run(plain)
    edited, names = E.edit_every_third(hb, cols, problem)
    run(edited)
    done = [c for c, n in enumerate(names) if n is not None]
    assert len(set(names[c] for c in done)) >= min(len(done), 5), names
    for c, name in enumerate(names):
        if name is None:
            assert E.same_bytes(edited, c, plain, c), (what, c, 'beside', names[max(c - 2, 0):c + 3])
    ref = E.subset(edited, done)
    oracle.run_batch(problem, ref)
    check_against_oracle(E.subset(edited, done, True), ref, problem, cols, [names[c] for c in done], what)
    return plain, edited, names


SHARED_SMALL = [('single', 8, 40), ('single', 64, 6), ('pair', 16, 70), ('pair', 64, 6)]


@pytest.mark.parametrize('kind, lanes, count', SHARED_SMALL, ids=['%s-%dlanes' % s[:2] for s in SHARED_SMALL])
@pytest.mark.parametrize('nd, iso', D.GEOMS, ids=['%dd-%s' % (nd, 'iso' if iso else 'aniso') for nd, iso in D.GEOMS])
def test_lane_groups_beside_a_failed_cluster(engine, oracle, nd, iso, kind, lanes, count):
    """small kernels: 8 (4) clusters share a wavefront and a lane group pulls its next cluster when
    one ends; more clusters than one wavefront holds at 8 and 16 lanes"""
    cell = D.Cell('small', nd, iso, 'small1' if kind == 'single' else 'small2', 0, lanes)
    case, = D.build_case(cell)
    prep = case.prepare(compute_error=True)
    b = prep.batch
    hb = E.subset(b, [k % b.n_clusters for k in range(count)])
    assert (case.flags == _abi.FLAG_THROUGHPUT) == (kind == 'pair' and lanes == 16)
    edited_against_plain(engine, oracle, prep.problem, hb, D.cell_id(cell) + ' x%d' % count)


def tail_specs(cap):
    n = cap + 7
    close = {0, 1, 5, n - 2, n - 1}
    return {
        # more entries than workgroups in an absorbed 3-4-feature bin: the loop
        'absorbed-nt1-loop': ([(3 + k % 2, k in close) for k in range(n)] + [(2, k % 3 == 0) for k in range(6)] +
                              [(1, False)] * 3, n + 10, NT1),
        'absorbed-nt2-dozen': ([(5 + k % 3, k % 4 == 0) for k in range(12)] + [(2, k % 3 == 0) for k in range(6)] +
                               [(1, False)] * 3, 13, NT2),
        'close-pairs-beyond-cap': ([(2, True)] * (cap + 9) + [(2, False)] * 70 + [(3, True), (3, False)] +
                                   [(1, False)] * 3, 0, None),
    }


@pytest.mark.parametrize('name', ['absorbed-nt1-loop', 'absorbed-nt2-dozen', 'close-pairs-beyond-cap'])
def test_tail_launch_beside_a_failed_cluster(engine, oracle, name):
    """the tail launch: a workgroup fits one entry after the other in the same LDS and registers"""
    cap = _cap(engine)
    assert 1 <= cap and cap + 100 <= 4 * 256, cap     # (the clusters fit the four frames of draw)
    spec, max_count, whole = tail_specs(cap)[name]
    frames, f0 = draw(spec)
    prep = cta.prepare_batch(f0, cta.ArrayReader(frames), DIAMETER)
    prep.problem.flags |= _abi.FLAG_THROUGHPUT
    with absorb(engine, max_count):
        # (the plan is decided by the problem and the sizes of the clusters: the same for both calls)
        plan = engine.plan(prep.problem, prep.batch.feat_offset)
        fused, absorbed = plan.tail()[0], plan.tail_bins()[0]
        plan.close()
        assert fused
        assert whole is None or absorbed[whole]
        assert whole is not None or not absorbed[PAIRS]
        plain, edited, names = edited_against_plain(engine, oracle, prep.problem, prep.batch, name)
    sizes = np.diff(prep.batch.feat_offset)
    for lo, hi in ((2, 2), (3, 4), (5, 10)):     # every bin of the launch with six clusters holds edited ones
        if ((sizes >= lo) & (sizes <= hi)).sum() >= 6:
            assert any(n is not None and lo <= sizes[c] <= hi for c, n in enumerate(names)), (lo, hi)


GAUSSIAN_TYPES = [t for t in D.problem_types() if t.family in ('gauss', 'gauss_tp', 'lowpass')]


@pytest.mark.parametrize('t', GAUSSIAN_TYPES, ids=lambda t: t.name)
def test_bins_of_one_call_beside_failed_clusters(engine, oracle, t):
    """every cell a gaussian problem type reaches, in one call: the bins launched together"""
    prep = D.build_type_case(t).prepare(compute_error=True)
    edited_against_plain(engine, oracle, prep.problem, prep.batch, 'type ' + t.name)
