"""Linking with the adaptive search range on the device (``ctr_link_adaptive_device``, DESIGN.md
7b): ids and ``adaptive_round`` against the host restatement of ``link.link_levels``, exactly, on
the inputs of tests/_link_adaptive.py."""
import numpy as np
import pandas as pd
import pytest
from numpy.testing import assert_equal

import clustertracking_amd as cta
from _link_adaptive import blob3d, blob40, blob100, eight_levels, lattice, memory_case, six_blobs
from clustertracking_amd import link as lk

pytestmark = pytest.mark.gpu


def assert_device_equals_host(levels, sr, memory, stop, step):
    want_ids, want_rounds = lk.link_levels(levels, sr, memory, adaptive_stop=stop, adaptive_step=step, diag=True)
    ids, rounds = lk.link_levels(levels, sr, memory, engine='device', adaptive_stop=stop, adaptive_step=step,
                                 diag=True)
    assert [len(i) for i in ids] == [len(l) for l in levels] == [len(r) for r in rounds]
    for t in range(len(levels)):
        differ = np.flatnonzero((ids[t] != want_ids[t]) | (rounds[t] != want_rounds[t]))
        assert len(differ) == 0, ("level %d: rows %r: device ids %r rounds %r, host ids %r rounds %r"
                                  % (t, differ[:8], ids[t][differ[:8]], rounds[t][differ[:8]],
                                     want_ids[t][differ[:8]], want_rounds[t][differ[:8]]))
        assert ids[t].dtype == np.int64 and rounds[t].dtype == np.int32
    return ids, rounds


def test_blob_of_40():
    levels, perm = blob40()
    with pytest.raises(lk.SubnetOversizeException):
        lk.link_levels(levels, 5., engine='device')
    ids, rounds = assert_device_equals_host(levels, 5., 0, .25, .9)
    assert (ids[1] == perm).sum() == 38 and rounds[1].max() == 8


def test_blob_of_100_with_too_many_destinations():
    ids, rounds = assert_device_equals_host(blob100(), 5., 0, .25, .9)
    assert rounds[1].max() > 0


def test_lattice():
    ids, rounds = assert_device_equals_host(lattice(), 2., 0, .4, .5)
    assert_equal(ids[1], np.arange(36))
    assert_equal(rounds[1], np.full(36, 2))


def test_blob_in_3d_with_an_anisotropic_range():
    ids, rounds = assert_device_equals_host(blob3d(), (2.5, 5., 5.), 0, (.125, .25, .25), .9)
    assert rounds[1].max() > 0


def test_eight_levels_in_one_launch():
    ids, rounds = assert_device_equals_host(eight_levels(), 5., 0, .25, .9)
    assert [t for t in range(8) if rounds[t].any()] == [3, 6]


def test_five_levels_with_memory():
    """the level-by-level path; the sources that level 2 leaves come back at levels 3 and 4"""
    levels, lost = memory_case()
    ids, rounds = assert_device_equals_host(levels, 5., 2, .25, .9)
    assert rounds[2].any() and len(lost(ids)) == 3
    assert all(p in ids[3] or p in ids[4] for p in lost(ids))


def test_six_blobs_in_600_rows():
    ids, rounds = assert_device_equals_host(six_blobs(), 5., 0, .25, .9)
    assert (rounds[1] > 0).sum() == 420 and (rounds[1] == 0).sum() == 180


def test_give_up_names_the_level_and_the_engine_recovers():
    (a, b), _ = blob40()
    far = np.array([[100., 100.], [120., 100.]])
    levels = [far, np.concatenate([a, far]), np.concatenate([b, far])]
    for memory in (0, 1):
        with pytest.raises(lk.SubnetOversizeException) as info:
            lk.link_levels(levels, 5., memory, engine='device', adaptive_stop=3., adaptive_step=.95)
        assert 'level 2' in str(info.value) and '40' in str(info.value)
    with pytest.raises(lk.SubnetOversizeException):
        lk.link_levels(levels, 5., 0, adaptive_stop=3., adaptive_step=.95)
    rng = np.random.RandomState(5)                                # 1 x 70: destinations, the same exception
    crowd = [np.array([[50., 50.]]), 50. + rng.uniform(-1, 1, (70, 2))]
    for engine in ('host', 'device'):
        with pytest.raises(lk.SubnetOversizeException) as info:
            lk.link_levels(crowd, 5., engine=engine, adaptive_stop=4., adaptive_step=.9)
        assert 'level 1' in str(info.value) and '70 destinations' in str(info.value)
    assert_device_equals_host(levels, 5., 0, .25, .9)


def _table(levels):
    offs = np.r_[0, np.cumsum([len(l) for l in levels])].astype(np.int64)
    return np.concatenate(levels), offs


def test_same_call_twice_gives_the_same_bytes():
    pos, offs = _table(six_blobs())
    first = cta.link_arrays(pos, offs, 5., adaptive_stop=.25, adaptive_step=.9, diag=True)
    again = cta.link_arrays(pos, offs, 5., adaptive_stop=.25, adaptive_step=.9, diag=True)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    levels, _ = memory_case()
    pos, offs = _table(levels)
    first = cta.link_arrays(pos, offs, 5., 2, adaptive_stop=.25, adaptive_step=.9, diag=True)
    again = cta.link_arrays(pos, offs, 5., 2, adaptive_stop=.25, adaptive_step=.9, diag=True)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


def test_where_the_plain_call_succeeds_the_ids_are_its_bytes():
    rng = np.random.default_rng(17)
    pos = rng.uniform(0, 100, (150, 2))       # dense: sub-networks of 10 x 10 and more, none oversize
    levels = []
    for t in range(8):
        pos = pos + rng.normal(0, 1.5, pos.shape)
        levels.append(pos[rng.permutation(150)[:140]])
    table, offs = _table(levels)
    for memory in (0, 2):
        plain = cta.link_arrays(table, offs, 5., memory)
        ids, rounds = cta.link_arrays(table, offs, 5., memory, adaptive_stop=.5, adaptive_step=.9, diag=True)
        assert ids.tobytes() == plain.tobytes() and ids.dtype == plain.dtype
        assert not rounds.any()
        assert cta.link_arrays(table, offs, 5., memory, adaptive_stop=.5).tobytes() == plain.tobytes()
        ids0, rounds0 = cta.link_arrays(table, offs, 5., memory, diag=True)
        assert ids0.tobytes() == plain.tobytes() and rounds0.dtype == np.int32 and not rounds0.any()


def test_tensors_in_and_the_dataframe_call():
    import torch
    levels = eight_levels()
    pos, offs = _table(levels)
    want = cta.link_arrays(pos, offs, 5., adaptive_stop=.25, adaptive_step=.9, diag=True)
    pt, ot = torch.from_numpy(pos).cuda(), torch.from_numpy(offs).cuda()
    got = cta.link_arrays(pt, ot, 5., adaptive_stop=.25, adaptive_step=.9, diag=True)
    assert_equal(got[0], want[0])
    assert_equal(got[1], want[1])
    t_ids, t_rounds = lk.link_arrays(pt, ot, 5., adaptive_stop=.25, adaptive_step=.9, diag=True, _on_device=True)
    assert t_ids.is_cuda and t_ids.dtype == torch.int64 and t_rounds.is_cuda and t_rounds.dtype == torch.int32
    assert_equal(t_ids.cpu().numpy(), want[0])
    assert_equal(t_rounds.cpu().numpy(), want[1])
    with pytest.raises(ValueError):
        cta.link_arrays(pt, ot, 5., adaptive_stop=5.)
    f = pd.DataFrame(pos, columns=['y', 'x'])
    f['frame'] = np.repeat(np.arange(len(levels)), [len(l) for l in levels])
    host = lk.link(f, 5., adaptive_stop=.25, adaptive_step=.9, diag=True)
    dev = lk.link(f, 5., engine='device', adaptive_stop=.25, adaptive_step=.9, diag=True)
    assert list(dev.columns) == list(host.columns)
    assert_equal(dev['particle'].values, host['particle'].values)
    assert_equal(dev['adaptive_round'].values, host['adaptive_round'].values)
