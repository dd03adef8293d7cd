"""``ctr_refine_prepare_device`` on the MI355X against the yardstick ``tests/_refine_arrays.py``:
integers, copies of doubles and single rounded operations, so ``assert_array_equal`` on every
output, doubles included.

Launch geometry under test: one workgroup of 256 threads per frame, the rows of a frame through LDS
in tiles of 256 (frames of 0, 1, 255, 256 and 257 rows; a cluster on both sides of the tile's edge
and one thread stride apart), sweeps until nothing changes (a shuffled chain of 40), the scan of the
clusters per frame (an empty frame between populated ones, no frame at all; 255, 256, 257 and 513
frames: one short of a chunk of the scan's workgroup, a chunk, one over, two and one over)."""
import functools

import numpy as np
import pytest

import _refine_arrays as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, refine

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _want(name):
    return yard.yardstick(yard.cases()[name])


def _device(case):
    ff, radius, separation = yard.model(case)
    return ff, refine.prepare_arrays(case.pos, case.off, yard.start_values(case), separation, ff,
                                     case.kw.get('bounds'), radius)


def _equal(got, want, n_params):
    n, c = len(want.label), len(want.frame_index)
    assert got.n_clusters == c and got.status == (_abi.PREPARE_OK, n_params)
    for name in ('label', 'cluster_size', 'order', 'feat_offset', 'frame_index'):
        t = getattr(got, name)
        assert t.dtype.is_floating_point is False and t.element_size() == 4
        np.testing.assert_array_equal(t.cpu().numpy(), getattr(want, name), err_msg=name)
    for name in ('params', 'low', 'high'):
        t = getattr(got, name)
        assert tuple(t.shape) == (n, n_params) and t.element_size() == 8
        np.testing.assert_array_equal(t.cpu().numpy(), getattr(want, name), err_msg=name)


@pytest.mark.parametrize('name', yard.PREPARE + yard.MANY_FRAMES + yard.REFINE)
def test_equals_the_yardstick(engine, name):
    case = yard.cases()[name]
    ff, got = _device(case)
    _equal(got, _want(name), ff.n_params)


def test_the_cases_are_the_edges(engine):
    """what the cases are there for is in them"""
    c = yard.cases()
    np.testing.assert_array_equal(np.diff(c['tile_edges'].off), [255, 0, 256, 1, 257])
    assert len(c['no_frame'].off) == 1 and len(c['no_row'].pos) == 0
    w = _want('tile_edges')
    assert w.cluster_size.max() >= 3 and (w.cluster_size == 1).sum() > 100
    assert (_want('chain').cluster_size[3:] == 40).all()
    np.testing.assert_array_equal(np.flatnonzero(_want('straddle').cluster_size == 4), [10, 255, 256, 299])
    np.testing.assert_array_equal(_want('exact_tie').label, [0, 0, 2, 3, 4])
    w = _want('aniso_3d')
    assert w.params.shape[1] == 8 and w.cluster_size.max() >= 2
    w = _want('bounds_all')
    assert np.isfinite(w.low).all() and np.isfinite(w.high).all()
    w = _want('nan_start')
    assert np.isnan(w.params).sum() == 3 and not np.isnan(w.low).any() and not np.isnan(w.high).any()


@pytest.mark.parametrize('name', sorted(yard.INFEASIBLE))
def test_infeasible_box(engine, name):
    """status names the first parameter whose box is empty, refine_arrays raises prepare_batch's error"""
    case = yard.cases()[name]
    ff, got = _device(case)
    assert got.status == (_abi.PREPARE_INFEASIBLE, ff.params.index(yard.INFEASIBLE[name]))
    with pytest.raises(ValueError, match=r"SLSQP Error: the lower bound exceeds the upper bound \(parameter '%s'\)"
                       % yard.INFEASIBLE[name]):
        ct.refine_arrays(case.frames, case.pos, case.off, signal=case.signal, size=case.size,
                         background=case.background, **yard.refine_kwargs(case))


def test_refused_offsets_of_a_tensor(engine):
    """a tensor's offsets are checked by the first kernel: nothing is followed, no cluster"""
    import torch
    case = yard.cases()['gauss_2d']
    ff, radius, separation = yard.model(case)
    for off in ([0, 30, 24], [0, 12, 23], [1, 12, 24], [0, -1, 24]):
        off_t = torch.tensor(off, dtype=torch.int64, device='cuda:0')
        got = refine.prepare_arrays(case.pos, off_t, yard.start_values(case), separation, ff, None, radius)
        assert got.status[0] == _abi.PREPARE_BAD_TABLE and got.n_clusters == 0
        with pytest.raises(ValueError, match='frame_offset'):
            ct.refine_arrays(torch.from_numpy(case.frames).cuda(), torch.from_numpy(case.pos).cuda(), off_t, 9,
                             signal=90., size=2.)


def test_same_bytes_on_another_stream_and_again(engine):
    import torch
    case = yard.cases()['tile_edges']
    ff, first = _device(case)
    with torch.cuda.stream(torch.cuda.Stream()):
        _, second = _device(case)
    _equal(second, _want('tile_edges'), ff.n_params)
    for a, b in zip(first[:8], second[:8]):
        assert torch.equal(a, b)
