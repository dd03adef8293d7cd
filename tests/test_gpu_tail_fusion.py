"""The tail launch of a throughput plan (include/ctrefine.h: ctr_plan_tail): with
CTR_FLAG_THROUGHPUT the likely slow clusters of the pairs, the 3-4-feature and the 5-10-feature
bins -- two starts closer than a quarter of the mask radius -- are fitted by one launch of
refine_tail_kernel, the rest of each bin by the bin's own launch.  Which launch carries a cluster
must not show in a single bit of its result.

The comparison needs no second build: a call that holds one of the three bins alone (plus singles)
does not fuse, and which kernel fits a cluster depends on the cluster alone.  So every case runs
its clusters once in one fused call and once as three unfused calls, and the tables are equal.

Inputs: uint8 frames of 512 x 512 (at most 4), gaussians of size 3 fitted with diameter 13 and the
default modes.  Clusters sit on a grid of 30 px; inside a cluster the starts are 5 px apart (far:
5 / 6 of the mask radius) except, in a close cluster, the second one, 1 px from the first (1 / 6).
The feature behind that start lies 3 px from the first one: the fit takes several re-window
rounds -- a slow fit, what the tail launch is for -- and ends in a well-conditioned minimum, where
the bound against the oracle (1e-6 px, tests/test_gpu_parity.py) is about summation order alone.
"""
import numpy as np
import pandas as pd
import pytest
from numpy.testing import assert_equal

import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib, artificial
from clustertracking_amd.device import DeviceBatch

pytestmark = pytest.mark.gpu

TABLES = ('params_out', 'cost', 'status', 'n_iter', 'n_rounds')
SHAPE = (512, 512)
DIAMETER = 13
RADIUS = DIAMETER // 2
SIZE = 3.
SIGNAL = 80
GRID = 30            # px between the first features of neighbouring clusters
PER_SIDE = 16        # clusters per row and column of a frame
SEED = 20261021
# starts of the features of a cluster relative to its first one, (y, x): 5 px apart
OFFSETS = np.array([(0, 0), (0, 5), (5, 0), (5, 5), (0, 10), (5, 10), (10, 0)], dtype=float)
CLOSE_START, CLOSE_TRUTH = 1., 3.   # x of the second feature of a close cluster: its start, where it is drawn
KIND = {1: 'single', 2: 'pair', 3: 'nt1', 4: 'nt1', 5: 'nt2', 6: 'nt2', 7: 'nt2'}
TAIL_KINDS = ('pair', 'nt1', 'nt2')


def draw(spec, seed=SEED):
    """spec: [(features, close), ...], one entry per cluster.  (frames, start table); the table
    carries `uid` (the feature), `cl` (the entry of spec) and `kind`."""
    rng = np.random.RandomState(seed)
    per_frame = PER_SIDE * PER_SIDE
    n_frames = (len(spec) + per_frame - 1) // per_frame
    assert 1 <= n_frames <= 4
    frames = np.zeros((n_frames,) + SHAPE, np.uint8)
    rows = []
    for j, (n, close) in enumerate(spec):
        t, cell = divmod(j, per_frame)
        gy, gx = divmod(cell, PER_SIDE)
        first = np.array([25. + GRID * gy, 25. + GRID * gx])
        start = first + OFFSETS[:n]
        truth = start.copy()
        if close:
            assert n >= 2
            start[1] = first + (0., CLOSE_START)
            truth[1] = first + (0., CLOSE_TRUTH)
        truth += rng.uniform(-0.3, 0.3, truth.shape)
        for p in truth:
            artificial.draw_gaussian(frames[t], p, SIZE, SIGNAL)
        for y, x in start:
            rows.append(dict(y=y, x=x, frame=t, cl=j, kind=KIND[n]))
    for t in range(n_frames):
        frames[t] = artificial.add_poisson_noise(frames[t], 4, rng)
    f0 = pd.DataFrame(rows)
    f0['uid'] = np.arange(len(f0))
    f0['signal'] = 0.9 * SIGNAL
    f0['size'] = SIZE
    f0['background'] = 2.
    return frames, f0


def is_close(batch, c):
    """front_load_kernel's rule on cluster c of a host batch"""
    p = batch.params[batch.feat_offset[c]:batch.feat_offset[c + 1], 2:4] / float(RADIUS)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    return bool((d2[np.triu_indices(len(p), 1)] < 0.0625).any()) or len(p) > 8


def populations(problem, batch):
    """{kind: (clusters, close ones)} by the plan's own dispatch (ctr_cluster_kernel)"""
    out = {}
    for c, n in enumerate(np.diff(batch.feat_offset)):
        kc = _lib.cluster_kernel(problem, int(n))
        kind = {_abi.KBIN_SMALL1: 'single', _abi.KBIN_SMALL2: 'pair'}.get(kc.bin)
        if kind is None:
            assert kc.bin == _abi.KBIN_BLOCK and kc.family == _abi.KFAM_GAUSS_TP and kc.nt in (1, 2), (kc.bin, kc.family, kc.nt)
            kind = 'nt%d' % kc.nt
        a, b = out.get(kind, (0, 0))
        out[kind] = (a + 1, b + (is_close(batch, c) if kind != 'single' else 0))
    return out


def intended(spec):
    out = {}
    for n, close in spec:
        a, b = out.get(KIND[n], (0, 0))
        out[KIND[n]] = (a + 1, b + (1 if close and n > 1 else 0))
    return out


class Run(object):
    """one call of a start table on the lanes; the tables per feature, keyed by uid"""

    def __init__(self, engine, frames, f0, flags=_abi.FLAG_THROUGHPUT):
        import torch
        self.prep = cta.prepare_batch(f0.reset_index(drop=True), cta.ArrayReader(frames), DIAMETER)
        self.prep.problem.flags |= flags
        self.db = DeviceBatch(self.prep.problem, self.prep.batch, device=0, engine=engine)
        self.fused, self.cap, self.grid = self.db.plan.tail()
        engine.refine_batch_device(self.db.plan, self.db.struct, 0)
        torch.cuda.synchronize()
        t = {k: self.db.t[k].cpu().numpy() for k in TABLES}
        self.tables = t
        uid = self.prep.f['uid'].values[self.prep.order]
        cl = self.prep.cluster_of_row
        self.by_uid = pd.DataFrame(dict(uid=uid, cost=t['cost'][cl], status=t['status'][cl], n_iter=t['n_iter'][cl],
                                        n_rounds=t['n_rounds'][cl])).set_index('uid')
        for q in range(t['params_out'].shape[1]):
            self.by_uid['p%d' % q] = t['params_out'][:, q]
        self.db.plan.close()


def check(engine, spec, seed=SEED):
    """the fused call against the three unfused ones; returns the fused Run"""
    frames, f0 = draw(spec, seed)
    fused = Run(engine, frames, f0)
    want = intended(spec)
    assert populations(fused.prep.problem, fused.prep.batch) == want
    assert fused.fused, 'the plan with %r does not fuse' % (want,)
    assert fused.grid == sum(min(want[k][0], fused.cap) for k in TAIL_KINDS if k in want)
    assert len(fused.by_uid) == len(f0)
    for kind in TAIL_KINDS:
        if kind not in want:
            continue
        part = f0[f0['kind'].isin((kind, 'single'))]
        alone = Run(engine, frames, part)
        assert not alone.fused and alone.grid == 0, kind
        got = fused.by_uid.loc[alone.by_uid.index]
        for col in alone.by_uid.columns:
            assert_equal(got[col].values, alone.by_uid[col].values, err_msg='%s: %s' % (kind, col))
    return fused


def mixed():
    spec = [(2, k % 5 == 0) for k in range(70)]              # 14 close pairs, 56 far: two tiers
    spec += [(3, k % 2 == 0) for k in range(6)] + [(4, k % 2 == 1) for k in range(4)]
    spec += [(5, True), (5, False), (6, True), (6, False), (7, True), (7, False)]
    spec += [(1, False)] * 12
    return spec


def test_fused_equals_unfused_and_the_oracle(engine, oracle):
    spec = mixed()
    run = check(engine, spec)
    assert run.cap >= 14 and run.grid == 70 + 10 + 6
    b = run.prep.batch
    ref = _abi.HostBatch(b.frames, b.frame_index, b.feat_offset, b.params, b.low, b.high)
    oracle.run_batch(run.prep.problem, ref)
    t = run.tables
    assert_equal(t['status'], ref.status)
    ok = np.repeat(t['status'] == 0, np.diff(b.feat_offset))
    d = np.abs(t['params_out'][:, 2:4] - ref.params_out[:, 2:4])[ok]
    print('fused call vs oracle: %d of %d clusters ok, max |dpos| %.3g px' % ((t['status'] == 0).sum(), len(t['status']), d.max()))
    assert ok.sum() >= len(ok) // 2     # (the comparison is about fits, not failures)
    assert d.max() < 1e-6


def _cap(engine):
    frames, f0 = draw([(2, False), (3, False)])
    prep = cta.prepare_batch(f0, cta.ArrayReader(frames), DIAMETER)
    plan = engine.plan(prep.problem, prep.batch.feat_offset)
    cap = plan.tail()[1]
    plan.close()
    return cap


EDGES = {
    # (a) a bin without a close cluster: every tail workgroup of its segment returns
    'no-close-pairs': lambda cap: [(2, False)] * 66 + [(3, True), (3, False), (4, True)] + [(1, False)] * 3,
    # (b) a bin of close clusters only: nothing for its own launch
    'all-close-nt1': lambda cap: [(2, k % 4 == 0) for k in range(66)] + [(3, True)] * 5 + [(1, False)] * 3,
    # (c) exactly cap close pairs; (d) one more, for the 64-lane launch of the pairs
    'cap-close-pairs': lambda cap: [(2, True)] * cap + [(2, False)] * 6 + [(3, True), (3, False)] + [(1, False)] * 3,
    'cap+1-close-pairs': lambda cap: [(2, True)] * (cap + 1) + [(2, False)] * 6 + [(3, True), (3, False)] + [(1, False)] * 3,
    # (e) cap + 1 close 3-feature clusters: the last one is fitted by the bin's own launch
    'cap+1-close-nt1': lambda cap: [(3, True)] * (cap + 1) + [(3, False)] * 2 + [(2, True), (2, False)] + [(1, False)] * 3,
}


@pytest.mark.parametrize('name', sorted(EDGES))
def test_edges_of_the_split(engine, name):
    cap = _cap(engine)
    assert 1 <= cap <= 600, cap     # (cap + 1 clusters of 30 px fit the four frames)
    run = check(engine, EDGES[name](cap))
    assert run.cap == cap


def test_fewer_than_64_pairs(engine):
    """one tier of pairs (no 16-lane launch): the far pairs run at 64 lanes in their own launch"""
    spec = [(2, k % 3 == 0) for k in range(12)] + [(3, True), (3, False), (4, False)] + [(1, False)] * 4
    run = check(engine, spec)
    assert run.grid == 12 + 3


def test_the_decision(engine):
    """ctr_plan_tail of plans that must not fuse, and of one that must; a plan needs the problem
    and the sizes of the clusters alone"""
    def tail(problem, sizes, flags=_abi.FLAG_THROUGHPUT):
        problem.flags |= flags
        plan = engine.plan(problem, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
        out = plan.tail()
        plan.close()
        return out

    def problem(ndim=2, **kw):
        cols = ['z', 'y', 'x'][-ndim:]
        f0 = pd.DataFrame(np.array([[10. + 9 * k] * ndim for k in range(4)]), columns=cols)
        f0['frame'] = 0
        f0['signal'], f0['size'], f0['background'] = 0.9 * SIGNAL, SIZE, 2.
        return cta.prepare_batch(f0, cta.ArrayReader(np.zeros((1,) + (48,) * ndim, np.uint8)),
                                 DIAMETER if ndim == 2 else (7, 7, 7), **kw).problem

    sizes = [2] * 5 + [3] * 4 + [6] * 2 + [1] * 7
    fused, cap, grid = tail(problem(), sizes)
    assert fused and grid == 5 + 4 + 2
    assert tail(problem(), [2] * (cap + 9) + [3])[2] == cap + 1
    assert tail(problem(), sizes, flags=0) == (False, cap, 0)
    assert tail(problem(3), sizes) == (False, cap, 0)
    assert tail(problem(noise_size=1.), sizes) == (False, cap, 0)
    assert tail(problem(fit_function='ring'), sizes) == (False, cap, 0)
    for one in (2, 3, 6):
        assert tail(problem(), [one] * 5 + [1] * 7) == (False, cap, 0), one
    # (a bin of more than 10 features is none of the three)
    assert tail(problem(), [2] * 5 + [12] * 3 + [1] * 7) == (False, cap, 0)


def test_two_handles_in_flight(engine):
    """4 calls on each of two handles, nothing waited for in between: a work counter or a count of
    front_load_kernel that a call left behind would change the next call's tables"""
    import torch
    frames, f0 = draw(mixed(), SEED + 1)
    prep = cta.prepare_batch(f0, cta.ArrayReader(frames), DIAMETER)
    prep.problem.flags |= _abi.FLAG_THROUGHPUT
    engines = [_lib.Engine(0), _lib.Engine(0)]
    calls = []
    try:
        calls = [[DeviceBatch(prep.problem, prep.batch, device=0, engine=e) for _ in range(4)] for e in engines]
        for per in calls:
            assert per[0].plan.tail()[0]
            for d in per:
                d.t['status'].fill_(-1)
        torch.cuda.synchronize()
        for k in range(4):
            for per in calls:     # (every call of a handle on the handle's first plan)
                per[k].engine.refine_batch_device(per[0].plan, per[k].struct, 0)
        torch.cuda.synchronize()
        first = {k: calls[0][0].t[k].cpu().numpy() for k in TABLES}
        assert (first['status'] >= 0).all()
        for per in calls:
            for d in per:
                for k in TABLES:
                    assert_equal(d.t[k].cpu().numpy(), first[k], err_msg=k)
    finally:
        for per in calls:
            for d in per:
                d.plan.close()
        for e in engines:
            e.close()
