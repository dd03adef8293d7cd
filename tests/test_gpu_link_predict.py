"""Linking with prediction on the device (``ctr_link_predict_device``): ids, velocities
and ``adaptive_round`` against the host restatement of ``link.link_levels``, exactly, on the inputs of
tests/_link_predict.py.  Every velocity has one owner lane or the stated sum order, so the
comparison is ``assert_array_equal``."""
import numpy as np
import pandas as pd
import pytest
from numpy.testing import assert_array_equal

import _link_predict as ref
import clustertracking_amd as cta
from _link_adaptive import blob40, six_blobs
from _link_predict import FLOW, FLOW_3D, SEARCH_RANGE, SEARCH_RANGE_3D, n_ids
from clustertracking_amd import link as lk

pytestmark = pytest.mark.gpu

PREDICTORS = ('velocity', 'drift')


def assert_device_equals_host(levels, sr, memory, predictor, v0, stop=None, step=.95):
    kw = dict(adaptive_stop=stop, adaptive_step=step, diag=True, predictor=predictor, initial_velocity=v0,
              want_velocity=True)
    want_ids, want_rounds, want_vel = lk.link_levels(levels, sr, memory, **kw)
    ids, rounds, vel = lk.link_levels(levels, sr, memory, engine='device', **kw)
    assert [len(i) for i in ids] == [len(l) for l in levels] == [len(r) for r in rounds] == [len(v) for v in vel]
    for t in range(len(levels)):
        assert_array_equal(ids[t], want_ids[t], err_msg='ids of level %d' % t)
        assert_array_equal(rounds[t], want_rounds[t], err_msg='rounds of level %d' % t)
        assert_array_equal(vel[t], want_vel[t], err_msg='velocities of level %d' % t)
        assert ids[t].dtype == np.int64 and rounds[t].dtype == np.int32 and vel[t].dtype == np.float64
    return ids, rounds, vel


@pytest.mark.parametrize('memory', (0, 2))
@pytest.mark.parametrize('predictor', PREDICTORS)
def test_flow(predictor, memory):
    levels = ref.flow()
    ids, _, vel = assert_device_equals_host(levels, SEARCH_RANGE, memory, predictor, FLOW)
    assert n_ids(ids) == 30 and np.abs(vel[5] - FLOW).max() < .25
    # without an initial velocity nothing links (with memory: but for a row remembered until its
    # neighbour arrives where it was, three levels later)
    ids, _, vel = assert_device_equals_host(levels, SEARCH_RANGE, memory, predictor, None)
    if memory == 0:
        assert n_ids(ids) == 180 and not np.concatenate(vel).any()
        assert n_ids(lk.link_levels(levels, SEARCH_RANGE, engine='device')) == 180        # more ids, no failure


@pytest.mark.parametrize('memory', (0, 2))
@pytest.mark.parametrize('predictor', PREDICTORS)
def test_ramp(predictor, memory):
    ids, _, _ = assert_device_equals_host(ref.ramp(), SEARCH_RANGE, memory, predictor, None)
    assert n_ids(ids) == 30


@pytest.mark.parametrize('memory', (0, 2))
def test_shear(memory):
    levels = ref.shear()
    ids, _, _ = assert_device_equals_host(levels, SEARCH_RANGE, memory, 'velocity', None)
    assert n_ids(ids) == 31
    ids, _, _ = assert_device_equals_host(levels, SEARCH_RANGE, memory, 'drift', None)
    assert n_ids(ids) > 31


@pytest.mark.parametrize('predictor', PREDICTORS)
def test_dropout_is_predicted_forward_by_its_age(predictor):
    levels, row0 = ref.dropout()
    ids, _, _ = assert_device_equals_host(levels, SEARCH_RANGE, 2, predictor, (0., 3.))
    assert n_ids(ids) == 30 and all(ids[t][0] == 0 for t in range(7) if row0[t] is not None)
    for memory in (0, 1):
        ids, _, _ = assert_device_equals_host(levels, SEARCH_RANGE, memory, predictor, (0., 3.))
        assert n_ids(ids) == 31


@pytest.mark.parametrize('predictor', PREDICTORS)
def test_empty_level(predictor):
    levels = ref.empty_level()
    for memory, n in ((0, 60), (1, 30), (2, 30)):
        ids, _, _ = assert_device_equals_host(levels, SEARCH_RANGE, memory, predictor, FLOW)
        assert n_ids(ids) == n
    # the video ends, or begins, with a level without rows
    assert_device_equals_host(levels[:3], SEARCH_RANGE, 1, predictor, FLOW)
    assert_device_equals_host(levels[2:], SEARCH_RANGE, 1, predictor, FLOW)


@pytest.mark.parametrize('memory', (0, 2))
@pytest.mark.parametrize('predictor', PREDICTORS)
def test_wide_level(predictor, memory):
    """more rows than a workgroup has threads: the second trip of the drift sum, births beyond row 256"""
    ids, _, _ = assert_device_equals_host(ref.wide_level(), SEARCH_RANGE, memory, predictor, FLOW)
    assert n_ids(ids) == 340 and np.flatnonzero(ids[1] >= 300).max() >= 256


def test_window_beyond_the_grid_of_the_velocity_kernel():
    """two levels of 8372 rows with memory 1: the source window that link_velocity_kernel strides over
    (16744 rows) is more than its 64 workgroups of 256 lanes"""
    rng = np.random.default_rng(12)
    g = np.stack(np.meshgrid(np.arange(92.), np.arange(91.), indexing='ij'), -1).reshape(-1, 2) * 10. + 20.
    born = g[rng.permutation(len(g))[:60]] + 5.
    second = np.concatenate([(g + FLOW)[rng.permutation(len(g))[:-50]], born])
    levels = [g, second[rng.permutation(len(second))] + ref.noise(rng, second.shape)]
    ids, _, vel = assert_device_equals_host(levels, SEARCH_RANGE, 1, 'velocity', FLOW)
    assert n_ids(ids) == len(g) + 60 and np.abs(vel[1] - FLOW).max() < .15


@pytest.mark.parametrize('memory', (0, 2))
@pytest.mark.parametrize('predictor', PREDICTORS)
def test_three_dimensions_with_an_anisotropic_range(predictor, memory):
    ids, _, _ = assert_device_equals_host(ref.flow3d(), SEARCH_RANGE_3D, memory, predictor, FLOW_3D)
    assert n_ids(ids) == 36


@pytest.mark.parametrize('memory', (0, 2))
@pytest.mark.parametrize('predictor', PREDICTORS)
def test_adaptive_range_works_on_the_predicted_positions(predictor, memory):
    levels, perm = ref.shifted_blob()
    ids, rounds, _ = assert_device_equals_host(levels, 5., memory, predictor, 3., .25, .9)
    assert rounds[1].max() > 0 and (ids[1] == perm).sum() == 38
    with pytest.raises(lk.SubnetOversizeException):           # without the adaptive range: the plain rule's failure
        lk.link_levels(levels, 5., memory, engine='device', predictor=predictor, initial_velocity=3.)


def _table(levels):
    offs = np.r_[0, np.cumsum([len(l) for l in levels])].astype(np.int64)
    return np.concatenate(levels), offs


def test_same_call_twice_gives_the_same_bytes():
    for levels, memory in ((ref.shear(), 0), (ref.wide_level(), 2)):
        pos, offs = _table(levels)
        for predictor in PREDICTORS:
            kw = dict(predictor=predictor, initial_velocity=FLOW, want_velocity=True)
            first = cta.link_arrays(pos, offs, SEARCH_RANGE, memory, **kw)
            again = cta.link_arrays(pos, offs, SEARCH_RANGE, memory, **kw)
            assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
            only_ids = cta.link_arrays(pos, offs, SEARCH_RANGE, memory, predictor=predictor, initial_velocity=FLOW)
            assert only_ids.tobytes() == first[0].tobytes()      # the velocities in the handle's scratch


def test_tensors_in_tensors_out(monkeypatch):
    import torch
    levels = ref.shear()
    pos, offs = _table(levels)
    want = cta.link_arrays(pos, offs, SEARCH_RANGE, 1, predictor='velocity', want_velocity=True)
    pt, ot = torch.from_numpy(pos).cuda(), torch.from_numpy(offs).cuda()
    read_back = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (read_back.append(tuple(self.shape)), cpu(self, *a, **k))[1])
    ids, rounds, vel = lk.link_arrays(pt, ot, SEARCH_RANGE, 1, predictor='velocity', want_velocity=True, diag=True,
                                      _on_device=True)
    monkeypatch.undo()
    assert read_back == [(4,)]                                   # nothing but the status
    assert ids.is_cuda and ids.dtype == torch.int64 and vel.is_cuda and vel.dtype == torch.float64
    assert rounds.is_cuda and rounds.dtype == torch.int32 and tuple(vel.shape) == (len(pos), 2)
    assert_array_equal(ids.cpu().numpy(), want[0])
    assert_array_equal(vel.cpu().numpy(), want[1])
    with pytest.raises(ValueError):
        cta.link_arrays(pt, ot, SEARCH_RANGE, predictor='channel')
    with pytest.raises(ValueError):
        cta.link_arrays(pt, ot, SEARCH_RANGE, predictor='drift', initial_velocity=(0., 1., 2.))


@pytest.mark.parametrize('predictor', PREDICTORS)
def test_table_form_equals_the_host(predictor):
    levels = ref.dropout()[0]
    pos, _ = _table(levels)
    f = pd.DataFrame(pos, columns=['y', 'x'])
    f['frame'] = np.repeat(3 * np.arange(len(levels)), [len(l) for l in levels])
    kw = dict(predictor=predictor, initial_velocity=(0., 3.), want_velocity=True)
    host = lk.link(f, SEARCH_RANGE, 2, **kw)
    dev = lk.link(f, SEARCH_RANGE, 2, engine='device', **kw)
    assert list(dev.columns) == list(host.columns) == ['y', 'x', 'frame', 'particle', 'vy', 'vx']
    for column in ('particle', 'vy', 'vx'):
        assert_array_equal(dev[column].values, host[column].values)
    assert dev['particle'].nunique() == 30


def test_plain_and_adaptive_calls_after_a_predictive_one_return_their_bytes():
    """the predictive call's scratch shares the handle's link block"""
    rng = np.random.default_rng(17)
    pos = rng.uniform(0, 100, (150, 2))
    levels = []
    for t in range(8):
        pos = pos + rng.normal(0, 1.5, pos.shape)
        levels.append(pos[rng.permutation(150)[:140]])
    table, offs = _table(levels)
    blobs, boffs = _table(six_blobs())
    before = [cta.link_arrays(table, offs, 5., memory) for memory in (0, 2)]
    before_ad = cta.link_arrays(blobs, boffs, 5., adaptive_stop=.25, adaptive_step=.9, diag=True)
    wide, woffs = _table(ref.wide_level())
    for predictor in PREDICTORS:
        cta.link_arrays(wide, woffs, SEARCH_RANGE, 2, predictor=predictor, initial_velocity=FLOW, want_velocity=True)
        cta.link_arrays(table, offs, 5., 2, predictor=predictor, adaptive_stop=.5)
        after = [cta.link_arrays(table, offs, 5., memory) for memory in (0, 2)]
        after_ad = cta.link_arrays(blobs, boffs, 5., adaptive_stop=.25, adaptive_step=.9, diag=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        assert before_ad[0].tobytes() == after_ad[0].tobytes() and before_ad[1].tobytes() == after_ad[1].tobytes()
    (a, b), _ = blob40()
    with pytest.raises(lk.SubnetOversizeException):
        cta.link_arrays(np.concatenate([a, b]), [0, 40, 80], 5.)
