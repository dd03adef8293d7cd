"""What the tail launch of a throughput plan takes beyond the likely slow clusters (include/ctrefine.h:
ctr_plan_tail_bins, ctr_set_tail_absorb): a 3-4- or 5-10-feature bin of at most
`max_count` clusters is fitted whole by the workgroups of the tail launch, which pull the bin's
entries from a counter, and has no launch of its own; of a larger bin the tail launch takes every
close cluster; the pairs of the 64-lane tier are all fitted there.  None of it may show in a single
bit of a result.

As in test_gpu_tail_fusion.py, whose inputs and helpers these tests use, a fused call is compared
table by table and per `uid` with the unfused calls of its parts; `max_count` is set to a handful
of clusters, so that both sides of the rule are reached with a dozen clusters.
"""
import contextlib

import numpy as np
import pytest
from numpy.testing import assert_equal

import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib
from clustertracking_amd.device import DeviceBatch
from test_gpu_tail_fusion import DIAMETER, SEED, TABLES, Run, check, draw, _cap

pytestmark = pytest.mark.gpu

PAIRS, NT1, NT2 = 0, 1, 2


@contextlib.contextmanager
def absorb(engine, max_count):
    """plans made inside fit a block bin of at most max_count clusters whole"""
    before = engine.set_tail_absorb(max_count)
    try:
        assert engine.set_tail_absorb(-1) == max_count
        yield before
    finally:
        engine.set_tail_absorb(before)


def bins(engine, run):
    """ctr_plan_tail_bins of a plan like the run's, made with the engine's setting of now"""
    plan = engine.plan(run.prep.problem, run.prep.batch.feat_offset)
    out = plan.tail_bins()
    plan.close()
    return out


def same(a, b):
    assert_equal(a.by_uid.index.values, b.by_uid.index.values)
    for col in a.by_uid.columns:
        assert_equal(a.by_uid[col].values, b.by_uid[col].values, err_msg=col)


def checked(engine, spec, max_count, seed=SEED):
    """the fused call of spec under max_count against its unfused parts: (Run, absorbed, own_launch)"""
    with absorb(engine, max_count):
        run = check(engine, spec, seed)
        absorbed, own = bins(engine, run)
    return run, absorbed, own


def test_default_and_setter(engine):
    cap = _cap(engine)
    default = engine.set_tail_absorb(-1)
    assert default == 32 * cap
    with absorb(engine, 3) as before:
        assert before == default
    assert engine.set_tail_absorb(-1) == default


@pytest.mark.parametrize('n, whole', [(5, True), (6, False)])
def test_rule_edges(engine, n, whole):
    """max_count = 5: a bin of 5 three-feature clusters is absorbed, one of 6 is not"""
    spec = [(2, k % 4 == 0) for k in range(8)] + [(3, k == 1) for k in range(n)] + [(1, False)] * 3
    run, absorbed, own = checked(engine, spec, 5)
    assert absorbed[NT1] == whole and own[NT1] == (not whole)
    assert absorbed[PAIRS] and not own[PAIRS]          # (one tier: every pair)
    assert not absorbed[NT2] and not own[NT2]          # (empty)
    off, absorbed0, own0 = checked(engine, spec, 0)
    assert not absorbed0[NT1] and own0[NT1]
    same(run, off)


def test_the_loop(engine):
    """more entries than workgroups: cap + 7 clusters of three and four features in a bin that is
    absorbed, close ones at the front and at the very end of the spec; twice on one plan"""
    import torch
    cap = _cap(engine)
    n = cap + 7
    assert n + 12 <= 4 * 256
    close = {0, 1, 5, n - 2, n - 1}
    spec = [(3 + k % 2, k in close) for k in range(n)] + [(2, k % 3 == 0) for k in range(6)] + [(1, False)] * 3
    run, absorbed, own = checked(engine, spec, n + 10)
    assert run.grid == cap + 6
    assert absorbed[NT1] and not own[NT1]
    assert_equal(run.tables['status'], 0)
    with absorb(engine, n + 10):
        db = DeviceBatch(run.prep.problem, run.prep.batch, device=0, engine=engine)
    try:
        assert db.plan.tail_bins()[0][NT1]
        for _ in range(2):     # (the counters of the segments start from zero in every call)
            db.t['status'].fill_(-1)
            db.t['n_iter'].fill_(-1)
            db.t['params_out'].fill_(float('nan'))
            torch.cuda.synchronize()
            engine.refine_batch_device(db.plan, db.struct, 0)
            torch.cuda.synchronize()
            for k in TABLES:   # (an entry that was skipped keeps the fill)
                assert_equal(db.t[k].cpu().numpy(), run.tables[k], err_msg=k)
    finally:
        db.plan.close()


@pytest.mark.parametrize('n1, n2', [(6, 3), (3, 6)])
def test_one_block_bin_absorbed_and_not_the_other(engine, n1, n2):
    spec = [(2, k % 4 == 0) for k in range(8)] + [(3 + k % 2, k % 3 == 0) for k in range(n1)]
    spec += [(5 + k % 3, k % 2 == 0) for k in range(n2)] + [(1, False)] * 3
    run, absorbed, own = checked(engine, spec, 4)
    assert absorbed[NT1] == (n1 <= 4) and own[NT1] == (n1 > 4)
    assert absorbed[NT2] == (n2 <= 4) and own[NT2] == (n2 > 4)
    same(run, checked(engine, spec, 0)[0])


def test_pairs_two_tiers_beyond_the_cap(engine):
    """more close pairs than the segment has workgroups: they take the overflow, no 64-lane launch"""
    cap = _cap(engine)
    spec = [(2, True)] * (cap + 9) + [(2, False)] * 70 + [(3, True), (3, False)] + [(1, False)] * 3
    run, absorbed, own = checked(engine, spec, 0)
    assert not own[PAIRS] and not absorbed[PAIRS]      # (two tiers: the far pairs at 16 lanes)
    assert run.grid == cap + 2


def test_pairs_one_tier(engine):
    spec = [(2, k % 3 == 0) for k in range(12)] + [(3, True), (3, False), (4, False)] + [(1, False)] * 4
    run, absorbed, own = checked(engine, spec, 0)
    assert absorbed[PAIRS] and not own[PAIRS]
    assert not absorbed[NT1] and own[NT1]


def test_absorbed_bin_without_a_close_cluster(engine):
    spec = [(2, k % 4 == 0) for k in range(8)] + [(3 + k % 2, False) for k in range(5)] + [(1, False)] * 3
    run, absorbed, own = checked(engine, spec, 5)
    assert absorbed[NT1] and not own[NT1]
    same(run, checked(engine, spec, 0)[0])


def absorbed_mix():
    spec = [(2, k % 5 == 0) for k in range(70)]              # 14 close pairs, 56 far: two tiers
    spec += [(3, k % 3 == 0) for k in range(9)] + [(4, k % 2 == 1) for k in range(4)]
    spec += [(5, True), (5, False), (6, True), (6, False), (7, True), (7, False)]
    spec += [(1, False)] * 12
    return spec


def test_absorbed_batch_against_the_oracle(engine, oracle):
    run, absorbed, own = checked(engine, absorbed_mix(), 13)
    assert absorbed == (False, True, True) and own == (False, False, False)
    b = run.prep.batch
    ref = _abi.HostBatch(b.frames, b.frame_index, b.feat_offset, b.params, b.low, b.high)
    oracle.run_batch(run.prep.problem, ref)
    t = run.tables
    assert_equal(t['status'], ref.status)
    ok = np.repeat(t['status'] == 0, np.diff(b.feat_offset))
    d = np.abs(t['params_out'][:, 2:4] - ref.params_out[:, 2:4])[ok]
    print('absorbed call vs oracle: %d of %d clusters ok, max |dpos| %.3g px' % ((t['status'] == 0).sum(), len(t['status']), d.max()))
    assert ok.sum() >= len(ok) // 2
    assert d.max() < 1e-6


def test_two_handles_in_flight(engine):
    """absorbed bins on two handles, 4 interleaved calls each, nothing waited for in between: every
    table equals that of a call alone"""
    import torch
    frames, f0 = draw(absorbed_mix(), SEED + 2)
    with absorb(engine, 0):
        alone = Run(engine, frames, f0)
    prep = cta.prepare_batch(f0, cta.ArrayReader(frames), DIAMETER)
    prep.problem.flags |= _abi.FLAG_THROUGHPUT
    engines = [_lib.Engine(0), _lib.Engine(0)]
    calls = []
    try:
        for e in engines:
            e.set_tail_absorb(13)
        calls = [[DeviceBatch(prep.problem, prep.batch, device=0, engine=e) for _ in range(4)] for e in engines]
        for per in calls:
            assert per[0].plan.tail_bins() == ((False, True, True), (False, False, False))
            for d in per:
                d.t['status'].fill_(-1)
        torch.cuda.synchronize()
        for k in range(4):
            for per in calls:     # (every call of a handle on the handle's first plan)
                per[k].engine.refine_batch_device(per[0].plan, per[k].struct, 0)
        torch.cuda.synchronize()
        for per in calls:
            for d in per:
                for k in TABLES:
                    assert_equal(d.t[k].cpu().numpy(), alone.tables[k], err_msg=k)
    finally:
        for per in calls:
            for d in per:
                d.plan.close()
        for e in engines:
            e.close()


def test_the_decision_table(engine):
    """(bin count, max_count) -> (absorbed, own launch), from the problem and the sizes of the
    clusters alone; and the plans that do not fuse"""
    import pandas as pd

    def problem(diameter=DIAMETER, **kw):
        f0 = pd.DataFrame(np.array([[10. + 9 * k] * 2 for k in range(4)]), columns=['y', 'x'])
        f0['frame'] = 0
        f0['signal'], f0['size'], f0['background'] = 72., 3., 2.
        return cta.prepare_batch(f0, cta.ArrayReader(np.zeros((1, 48, 48), np.uint8)), diameter, **kw).problem

    def tail_bins(sizes, max_count, flags=_abi.FLAG_THROUGHPUT, **kw):
        p = problem(**kw)
        p.flags |= flags
        with absorb(engine, max_count):
            plan = engine.plan(p, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
        out = plan.tail_bins()
        plan.close()
        return out

    cap = _cap(engine)
    for count, max_count, whole in [(1, 0, False), (1, 1, True), (5, 4, False), (5, 5, True), (5, 6, True),
                                    (cap, cap, True), (cap + 1, cap, False), (cap + 1, cap + 1, True),
                                    (8 * cap, 8 * cap, True), (8 * cap + 1, 8 * cap, False)]:
        for size, sgm in ((3, NT1), (4, NT1), (6, NT2), (10, NT2)):
            absorbed, own = tail_bins([2] * 5 + [size] * count + [1] * 7, max_count)
            assert absorbed[sgm] == whole and own[sgm] == (not whole), (count, max_count, size)
            assert absorbed[PAIRS] and not own[PAIRS]
            other = NT2 if sgm == NT1 else NT1
            assert not absorbed[other] and not own[other]
    # pairs: one tier below 64 pairs, two from there on; neither queues the 64-lane launch
    for pairs, whole in ((63, True), (64, False), (cap + 9, False)):
        absorbed, own = tail_bins([2] * pairs + [3] * 2, 0)
        assert absorbed[PAIRS] == whole and not own[PAIRS], pairs
    # windows of more than 600 pixels: one tier however many pairs; beyond 8 * cap of them the tail
    # launch takes the close ones only and the 64-lane launch stays
    for pairs, whole in ((64, True), (8 * cap, True), (8 * cap + 1, False)):
        absorbed, own = tail_bins([2] * pairs + [3] * 2, 0, diameter=27)
        assert absorbed[PAIRS] == whole and own[PAIRS] == (not whole), pairs
    # an empty bin among the three
    assert tail_bins([3] * 4 + [6] * 2 + [1], 8) == ((False, True, True), (False, False, False))
    # plans that do not fuse launch what they launched: nothing absorbed, every bin its own launch
    sizes = [2] * 5 + [3] * 4 + [6] * 2 + [1] * 7
    assert tail_bins(sizes, 8) == ((True, True, True), (False, False, False))
    assert tail_bins(sizes, 8, flags=0) == ((False,) * 3, (True,) * 3)
    # (with a lowpass or another profile the pairs are clusters of the 3-4-feature bin's kernel)
    assert tail_bins(sizes, 8, noise_size=1.) == ((False,) * 3, (False, True, True))
    assert tail_bins(sizes, 8, fit_function='ring') == ((False,) * 3, (False, True, True))
    assert tail_bins([3] * 5 + [1] * 7, 8) == ((False,) * 3, (False, True, False))
    assert tail_bins([2] * 5 + [12] * 3 + [1] * 7, 8) == ((False,) * 3, (True, False, False))
