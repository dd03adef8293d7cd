"""Refine calls on the lanes of the device (include/ctrefine.h "Lanes"): wherever the
chains of a call are queued -- one lane, two, all; several handles in flight on their own streams
-- the tables are those of the same plan run alone on a caller's stream, bit for bit (no kernel
knows where it runs), and every way of waiting for a call on the handle's own stream sees the
call finished (the stream is joined with the call lazily, ctrefine.hip: own_stream).
"""
import time

import numpy as np
import pytest
from numpy.testing import assert_equal

import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib, workloads
from clustertracking_amd.device import DeviceBatch

pytestmark = pytest.mark.gpu

TABLES = ('params_out', 'cost', 'status', 'n_iter', 'n_rounds')


def _bins(problem, feat_offset):
    """clusters per (bin, nt) of the plan's dispatch (ctr_cluster_kernel)"""
    out = {}
    for n in np.diff(feat_offset):
        kc = _lib.cluster_kernel(problem, int(n))
        key = (kc.bin, kc.nt) if kc.bin in (_abi.KBIN_BLOCK, _abi.KBIN_CONS) else (kc.bin, 0)
        out[key] = out.get(key, 0) + 1
    return out


def _tables(db):
    """the output tables as they are on the device (the legacy default stream's copies; the caller
    has waited for the call)"""
    return {k: db.t[k].cpu().numpy() for k in TABLES}


def _reference(problem, batch):
    """the plan on a handle of its own, on a caller's stream, read after that stream's synchronise"""
    import torch
    eng = _lib.Engine(0)
    db = DeviceBatch(problem, batch, device=0, engine=eng)
    s = torch.cuda.Stream()
    db.run(stream=s.cuda_stream)
    s.synchronize()
    ref = _tables(db)
    db.plan.close()
    eng.close()
    return ref


class Work(object):
    def __init__(self, name):
        if name == 'cfg2':
            frames, f0, truth, opts = workloads.cfg2(4)
            extra = {}
        else:
            frames, f0, truth, opts = workloads.cfg5(1)
            extra = dict(constraints=cta.constraints.dimer(6., 2))
        prep = cta.prepare_batch(f0, cta.ArrayReader(frames), opts['diameter'], **extra)
        prep.problem.flags |= _abi.FLAG_THROUGHPUT
        self.name, self.problem, self.batch = name, prep.problem, prep.batch
        self.bins = _bins(self.problem, self.batch.feat_offset)
        self.ref = _reference(self.problem, self.batch)


@pytest.fixture(scope='module', params=['cfg2', 'cfg5'])
def work(request):
    return Work(request.param)


@pytest.fixture(scope='module')
def cfg2():
    return Work('cfg2')


@pytest.fixture(scope='module')
def trio():
    """three handles besides the default engine's"""
    engines = [_lib.Engine(0) for _ in range(3)]
    yield engines
    for e in engines:
        e.close()


@pytest.fixture(autouse=True)
def all_lanes(engine):
    yield
    assert engine.set_lane_limit(0) >= 1


def assert_tables(got, ref):
    for k in TABLES:
        assert_equal(got[k], ref[k], err_msg=k)


def test_bin_populations(work):
    """the workloads fill the bins that the cases below are about"""
    b = work.bins
    if work.name == 'cfg2':
        assert work.batch.n_clusters == 653
        assert b == {(_abi.KBIN_SMALL1, 0): 537, (_abi.KBIN_SMALL2, 0): 95,
                     (_abi.KBIN_BLOCK, 1): 19, (_abi.KBIN_BLOCK, 2): 2}
    else:
        n = np.diff(work.batch.feat_offset)
        assert work.batch.n_clusters == 36
        assert b.get((_abi.KBIN_CONS, 1), 0) + b.get((_abi.KBIN_CONS, 2), 0) == 8 and int((n == 2).sum()) == 8
        block = {k: v for k, v in b.items() if k[0] == _abi.KBIN_BLOCK}
        assert sum(block.values()) == 28 and int(((n >= 8) & (n <= 16)).sum()) == 28
        # four bin chains besides head and finish: more chains than the 1, 2 or 4 lanes they run on
        assert len(b) == 4, b


@pytest.mark.parametrize('limit', [1, 2, 0])
def test_handles_in_flight_equal_the_reference(engine, trio, work, limit):
    import torch
    dbs = [DeviceBatch(work.problem, work.batch, device=0, engine=e) for e in trio]
    assert engine.set_lane_limit(limit) >= 1
    for k in range(12):
        d = dbs[k % 3]
        d.engine.refine_batch_device(d.plan, d.struct, 0)
    torch.cuda.synchronize()
    for d in dbs:
        assert_tables(_tables(d), work.ref)


def test_result_rows_and_done_flags_in_flight(trio, cfg2):
    import torch
    n, width = cfg2.batch.n_features, cfg2.batch.params.shape[1] + 1
    inbox = torch.zeros((3, n + 3, width), dtype=torch.float64, device='cuda')
    seq = torch.zeros(3, dtype=torch.int64, device='cuda')
    dbs = [DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=e, result_rows=inbox[i], done_flag=seq[i:i + 1])
           for i, e in enumerate(trio)]
    torch.cuda.synchronize()
    for i, d in enumerate(dbs):
        d.struct.done_value = 100 + i
        d.engine.refine_batch_device(d.plan, d.struct, 0)
    torch.cuda.synchronize()
    assert seq.tolist() == [100, 101, 102]
    got = inbox.cpu().numpy()
    for i in range(3):
        assert_equal(got[i, :n, :-1], cfg2.ref['params_out'])
        assert_equal(got[i, :n, -1], np.repeat(cfg2.ref['cost'], np.diff(cfg2.batch.feat_offset)))
        assert_equal(got[i, n:], 0.)


def test_lazy_join_stream_wait_engine(trio, cfg2):
    import torch
    d = DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=trio[0])
    s = torch.cuda.Stream()
    d.engine.refine_batch_device(d.plan, d.struct, 0)
    d.engine.stream_wait_engine(s.cuda_stream)
    with torch.cuda.stream(s):
        copy = {k: d.t[k].clone() for k in TABLES}
    s.synchronize()
    assert_tables({k: v.cpu().numpy() for k, v in copy.items()}, cfg2.ref)


def test_lazy_join_synchronize(trio, cfg2):
    d = DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=trio[1])
    d.engine.refine_batch_device(d.plan, d.struct, 0)
    d.engine.synchronize()
    assert_tables(_tables(d), cfg2.ref)


def test_lazy_join_query_done(trio, cfg2):
    d = DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=trio[2])
    d.engine.refine_batch_device(d.plan, d.struct, 0)
    deadline = time.monotonic() + 30.
    while not d.engine.query_done():
        assert time.monotonic() < deadline, "the call has not finished within 30 s"
    assert_tables(_tables(d), cfg2.ref)


def test_lazy_join_own_stream_work_lands_after_the_call(trio, cfg2):
    import torch
    flag = torch.zeros(1, dtype=torch.int64, device='cuda')
    d = DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=trio[0], done_flag=flag)
    torch.cuda.synchronize()
    d.struct.done_value = 41
    d.engine.refine_batch_device(d.plan, d.struct, 0)
    d.engine.ipc_probe(flag.data_ptr(), -5)      # on the engine's own stream; waits for it
    assert flag.tolist() == [-5]
    assert_tables(_tables(d), cfg2.ref)


def test_engine_wait_stream_orders_the_inputs(trio, cfg2):
    import copy
    import torch
    moved = copy.copy(cfg2.batch)
    moved.params = cfg2.batch.params.copy()
    moved.params[:, 2:4] += np.random.RandomState(5).uniform(-0.3, 0.3, size=(len(moved.params), 2))
    ref = _reference(cfg2.problem, moved)
    assert not np.array_equal(ref['params_out'], cfg2.ref['params_out'])   # (the inputs matter to the last bit)
    d = DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=trio[1])
    new_params = torch.from_numpy(moved.params).to('cuda')
    a = torch.ones((4096, 4096), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(4):
            a = (a @ a) * (1. / 4096.)
        d.t['params'].copy_(new_params, non_blocking=True)
    d.engine.engine_wait_stream(side.cuda_stream)
    d.engine.refine_batch_device(d.plan, d.struct, 0)
    d.engine.synchronize()
    assert_tables(_tables(d), ref)
    side.synchronize()


def test_engine_wait_stream_twice_orders_both_streams(trio, cfg2):
    """Two ctr_engine_wait_stream calls before one refine call: the start parameters come from one
    stream (the slower, and named first: a call that honoured the last wait alone would miss it),
    the frames from another.  Before, the batch holds other parameters and empty frames."""
    import copy
    import torch
    moved = copy.copy(cfg2.batch)
    moved.params = cfg2.batch.params.copy()
    moved.params[:, 2:4] += np.random.RandomState(6).uniform(-0.3, 0.3, size=(len(moved.params), 2))
    ref = _reference(cfg2.problem, moved)
    assert not np.array_equal(ref['params_out'], cfg2.ref['params_out'])
    d = DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=trio[2])
    new_params = torch.from_numpy(moved.params).to('cuda')
    frames = d.t['frames'].clone()
    d.t['frames'].zero_()
    a = torch.ones((4096, 4096), dtype=torch.float32, device='cuda')
    b = torch.ones((4096, 4096), dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    slow, fast = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(slow):
        for _ in range(8):
            a = (a @ a) * (1. / 4096.)
        d.t['params'].copy_(new_params, non_blocking=True)
    with torch.cuda.stream(fast):
        b = (b @ b) * (1. / 4096.)
        d.t['frames'].copy_(frames, non_blocking=True)
    d.engine.engine_wait_stream(slow.cuda_stream)
    d.engine.engine_wait_stream(fast.cuda_stream)
    d.engine.refine_batch_device(d.plan, d.struct, 0)
    d.engine.synchronize()
    assert_tables(_tables(d), ref)
    slow.synchronize()
    fast.synchronize()


def test_last_kernel_ms_of_an_own_stream_call(trio, cfg2):
    d = DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=trio[2])
    d.engine.refine_batch_device(d.plan, d.struct, 0)
    fm, rf = d.engine.last_kernel_ms()
    assert np.isfinite(fm) and np.isfinite(rf) and fm >= 0. and rf > 0.


def test_engine_deleted_with_its_call_in_flight(trio, cfg2):
    import torch
    gone = _lib.Engine(0)
    d_gone = DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=gone)
    d = DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=trio[0])
    d_gone.engine.refine_batch_device(d_gone.plan, d_gone.struct, 0)
    d.engine.refine_batch_device(d.plan, d.struct, 0)
    gone.close()
    d_gone.plan.close()
    d.engine.refine_batch_device(d.plan, d.struct, 0)
    torch.cuda.synchronize()
    assert_tables(_tables(d), cfg2.ref)
    assert_tables(_tables(d_gone), cfg2.ref)


def test_set_lane_limit(engine, trio, cfg2):
    import torch
    assert engine.set_lane_limit(0) >= 1
    lanes = engine.set_lane_limit(0)          # the number in use before: all of them
    assert 1 <= lanes <= 32
    assert engine.set_lane_limit(1) == lanes
    assert engine.set_lane_limit(lanes) == 1
    assert engine.set_lane_limit(1) == lanes
    assert engine.set_lane_limit(lanes + 1) == -1
    assert engine.set_lane_limit(-1) == -1
    assert engine.set_lane_limit(1) == 1      # (the refused calls changed nothing)
    assert _lib.load().ctr_set_lane_limit(63, 1) == -1   # a device without a handle
    d = DeviceBatch(cfg2.problem, cfg2.batch, device=0, engine=trio[1])
    d.engine.refine_batch_device(d.plan, d.struct, 0)
    torch.cuda.synchronize()
    assert_tables(_tables(d), cfg2.ref)
    assert engine.set_lane_limit(0) == 1
