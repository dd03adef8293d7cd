"""``ct.refine_arrays`` on the MI355X against ``refine_leastsq(cluster_labels='device')``: the same
kernels on the same batch bytes in the same plan order, so ``assert_array_equal`` on every column;
tensors against ndarrays, another stream, the chain from frames to orientations on the device
against the chain of DataFrames, and a cluster outside the frame."""
import functools

import numpy as np
import pytest

import _refine_arrays as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, motion

pytestmark = pytest.mark.gpu


def _arrays(case, compute_error=False, tensors=False):
    frames, pos, off, signal, size = case.frames, case.pos, case.off, case.signal, case.size
    if tensors:
        import torch
        frames, pos, off = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (frames, pos, off))
        size = torch.from_numpy(np.asarray(size)).cuda() if np.ndim(size) else size
    return ct.refine_arrays(frames, pos, off, signal=signal, size=size, background=case.background,
                            compute_error=compute_error, **yard.refine_kwargs(case))


@functools.lru_cache(maxsize=None)
def _table_path(name, compute_error=False):
    case = yard.cases()[name]
    return ct.refine_leastsq(yard.table(case), ct.ArrayReader(case.frames), cluster_labels='device',
                             compute_error=compute_error, **yard.refine_kwargs(case))


def _same(res, f, ff, compute_error):
    assert res.columns == ff.params and res.params.dtype == np.float64 and res.cluster.dtype == np.int64
    for k, col in enumerate(ff.params):
        np.testing.assert_array_equal(res.params[:, k], f[col].values, err_msg=col)
    np.testing.assert_array_equal(res.cost, f['cost'].values)
    np.testing.assert_array_equal(res.cluster, f['cluster'].values)
    np.testing.assert_array_equal(res.cluster_size, f['cluster_size'].values)
    if not compute_error:
        assert res.params_std is None
        return
    for k, col in enumerate(ff.params):
        if ff.modes[k] > 0:
            np.testing.assert_array_equal(res.params_std[:, k], f[col + '_std'].values, err_msg=col + '_std')
        else:
            assert np.isnan(res.params_std[:, k]).all()


@pytest.mark.parametrize('compute_error', [False, True], ids=['fit', 'std'])
@pytest.mark.parametrize('name', [n for n in yard.REFINE if n != 'outside'])
def test_equals_refine_leastsq(engine, name, compute_error):
    case = yard.cases()[name]
    ff, _, _ = yard.model(case)
    f = _table_path(name, compute_error)
    res = _arrays(case, compute_error)
    _same(res, f, ff, compute_error)
    want = yard.yardstick(case)
    np.testing.assert_array_equal(res.feat_offset, want.feat_offset)
    assert res.status.shape == res.n_rounds.shape == res.n_iter.shape == (len(want.frame_index),)
    # the fits did something
    assert (res.status == _abi.STATUS_OK).any() and np.isfinite(res.cost).any() and (res.n_iter > 0).any()
    assert (np.abs(res.params[:, 2:2 + case.pos.shape[1]] - case.pos) > 0).any()


def test_the_large_cluster_takes_the_large_kernel(engine):
    from clustertracking_amd import _lib
    case = yard.cases()['large_70']
    ff, radius, _ = yard.model(case)
    problem = _abi.make_problem(2, True, ff.modes, radius)
    assert _lib.cluster_kernel(problem, 70).bin == _abi.KBIN_LARGE
    assert (yard.yardstick(case).cluster_size == 70).all()


def test_tensors_in_tensors_out_and_another_stream(engine):
    import torch
    case = yard.cases()['gauss_2d']
    host = _arrays(case, compute_error=True)
    dev = _arrays(case, compute_error=True, tensors=True)
    with torch.cuda.stream(torch.cuda.Stream()):
        other = _arrays(case, compute_error=True, tensors=True)
        torch.cuda.current_stream().synchronize()
    for name, h, d, o in zip(host._fields, host, dev, other):
        if name == 'columns':
            assert h == d == o
            continue
        assert isinstance(h, np.ndarray) and torch.is_tensor(d) and d.is_cuda and torch.is_tensor(o)
        assert d.cpu().numpy().dtype == h.dtype
        assert d.cpu().numpy().tobytes() == h.tobytes() == o.cpu().numpy().tobytes(), name


def test_a_cluster_outside_the_frame(engine):
    """cost NaN and the parameters unchanged, as in refine_leastsq"""
    case = yard.cases()['outside']
    ff, _, _ = yard.model(case)
    res = _arrays(case)
    _same(res, _table_path('outside'), ff, False)
    assert np.isnan(res.cost[1:3]).all() and np.isfinite(res.cost[[0, 3, 4]]).all()
    np.testing.assert_array_equal(res.params[1:3], yard.start_values(case)[1:3])
    np.testing.assert_array_equal(res.cluster, [0, 1, 1, 3, 3])
    assert sorted(res.status.tolist()) == [0, 0, _abi.STATUS_OUT_OF_BOUNDS]


def test_empty_tables(engine):
    for name in ('no_frame', 'no_row'):
        case = yard.cases()[name]
        res = _arrays(case)
        assert res.params.shape == (0, 5) and res.cost.shape == (0,) and res.feat_offset.tolist() == [0]
        assert res.status.shape == (0,) and res.cluster.dtype == np.int64


@functools.lru_cache(maxsize=None)
def _dimer_video():
    """8 frames of 64 x 64 with 6 dimers that drift and turn"""
    rng = np.random.RandomState(5)
    centres = np.array([[12., 12.], [12., 34.], [12., 54.], [40., 14.], [42., 38.], [52., 54.]])
    angle = rng.uniform(0, np.pi, 6)
    frames = np.zeros((8, 64, 64), dtype=np.uint8)
    for t in range(8):
        centres = centres + rng.uniform(-0.4, 0.4, centres.shape)
        angle = angle + rng.uniform(-0.15, 0.15, 6)
        arm = 2.5 * np.stack([np.sin(angle), np.cos(angle)], 1)
        for p in np.r_[centres - arm, centres + arm]:
            ct.artificial.draw_feature(frames[t], p, 2., 150)
    return frames


def test_the_chain_on_the_device_equals_the_chain_of_tables(engine):
    """find_link_arrays -> refine_arrays -> cluster_tracks_arrays -> track_positions_arrays ->
    orientation_arrays, tensors all the way, against find_link -> refine_leastsq -> cluster_tracks ->
    orientation_df"""
    import torch
    frames = _dimer_video()
    link = dict(search_range=3, separation=4, diameter=7)
    fit = dict(diameter=7, separation=8, constraints=ct.constraints.dimer(5.))
    # tables
    f = ct.find_link(frames, **link)
    assert len(f) >= 8 * 6
    f = ct.refine_leastsq(f, ct.ArrayReader(frames), cluster_labels='device', **fit)
    f = ct.cluster_tracks(f, 2)
    assert f.attrs['n_tracks'] >= 1
    com, bases, ids = motion.orientation_df(f[f['cluster_track'] >= 0], 2, ndim=2, track_column='cluster_track')
    # tensors
    t_frames = torch.from_numpy(frames).cuda()
    r = ct.find_link_arrays(t_frames, _on_device=True, **link)
    res = ct.refine_arrays(t_frames, r.pos, r.frame_offset, signal=r.signal, size=r.size, **fit)
    assert all(torch.is_tensor(x) and x.is_cuda for x in (res.params, res.cost, res.cluster, res.cluster_size))
    for k, col in enumerate(res.columns):
        np.testing.assert_array_equal(res.params[:, k].cpu().numpy(), f[col].values, err_msg=col)
    np.testing.assert_array_equal(res.cost.cpu().numpy(), f['cost'].values)
    np.testing.assert_array_equal(res.cluster.cpu().numpy(), f['cluster'].values)
    tracks = ct.cluster_tracks_arrays(r.frame_offset, r.particle, res.cluster, 2, n_particles=int(r.n_tracks.item()))
    assert tracks.n_tracks == f.attrs['n_tracks'] and tracks.status == _abi.TRACKS_OK
    np.testing.assert_array_equal(tracks.track_of_particle.cpu().numpy()[f['particle'].values], f['cluster_track'].values)
    block = ct.track_positions_arrays(res.params[:, 2:4].contiguous(), r.frame_offset, r.particle,
                                      tracks.track_of_particle, tracks.n_tracks, 2)
    t_com, t_bases = motion.orientation_arrays(block.pos, 2, 2)
    assert torch.is_tensor(t_com) and t_com.is_cuda
    np.testing.assert_array_equal(ids, np.arange(tracks.n_tracks))
    np.testing.assert_array_equal(t_com.cpu().numpy(), com)
    np.testing.assert_array_equal(t_bases.cpu().numpy(), bases)
    assert np.isfinite(com).any()
