"""``ctr_find_link_device`` / ``clustertracking_amd.find_link`` on the MI355X against the NumPy
restatement of its rule (tests/_find_link.py): seeded videos, the constructed edge cases, the
refusals, and the ways in (tensors, streams, preprocessing)."""
import numpy as np
import pytest

import _find_link as F
import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib
from clustertracking_amd import link as lk

pytestmark = pytest.mark.gpu

RANDOM = F.random_cases()
EDGE = F.edge_cases()
BRIGHT = F.bright_cases()
FIXTURES = F.fixtures()


@pytest.mark.parametrize('index', range(len(FIXTURES)), ids=[c[0] for c in FIXTURES])
def test_device_equals_the_reference(engine, index):
    name, frames, kw, want = FIXTURES[index]
    ndim, iso = frames.ndim - 1, F.is_isotropic(kw)
    got = cta.find_link_arrays(frames, **kw)
    F.assert_equals_fixture(F.from_arrays(got, ndim, iso), want, ndim, iso, frames.dtype.kind in 'ui')


def check(frames, kw, **extra):
    """device == restatement: bit for bit on integer frames, 1e-12 on float64 ones"""
    ndim = frames.ndim - 1
    iso = F.is_isotropic(kw)
    want = F.find_link(frames, **kw)
    got = cta.find_link_arrays(frames, **dict(kw, **extra))
    assert not got.status.any()
    F.assert_same(F.from_arrays(got, ndim, iso), want, ndim, iso, exact=frames.dtype.kind in 'ui')
    return got, want


@pytest.mark.parametrize('index', range(len(RANDOM)), ids=[c[0] for c in RANDOM])
def test_seeded_videos(engine, index):
    name, frames, kw = RANDOM[index]
    check(frames, kw)


def test_many_levels(engine):
    """257 frames of 24 x 24 pixels with two features, one of them in and out of the margin: the
    offsets of the frames' live rows and the first ids of the levels are scanned by one workgroup in
    chunks of 256 levels"""
    frames = F.video((24, 24), 257, 2, 257, drift=0.2, size=1.2, margin=3, centres=[[8., 9.], [15., 16.]])
    got, want = check(frames, dict(diameter=5, separation=6, search_range=3, minmass=100))
    assert len(got.frame_offset) == 258 and got.frame_offset[-1] >= 257


@pytest.mark.parametrize('name', sorted(EDGE))
def test_edge_cases(engine, name):
    frames, kw = EDGE[name]
    got, want = check(frames, kw)
    if name == 'coupled':
        assert got.coupled.tolist() == [False, True]
    if name == 'all_relocated':     # the relocated rows of a frame in C order of position
        assert got.pos[2:].tolist() == [[1., 30.], [20., 1.]] and got.relocated.tolist() == [False, False, True, True]


def test_dataframe(engine):
    name, frames, kw = RANDOM[6]
    want = F.find_link(frames, **kw)
    f = cta.find_link(frames, **kw)
    assert list(f.columns) == ['y', 'x', 'frame', 'particle', 'mass', 'signal', 'size', 'relocated']
    assert np.array_equal(f[['y', 'x']].values, want['pos']) and np.array_equal(f['frame'].values, want['frame'])
    assert np.array_equal(f['particle'].values, want['particle']) and f['relocated'].sum() == want['relocated'].sum() > 0
    assert f.attrs['coupled_levels'] == int(want['coupled'].sum()) and f.attrs['n_tracks'] == want['n_tracks']
    name, frames, kw = RANDOM[3]
    f = cta.find_link(frames, **kw)
    assert list(f.columns) == ['y', 'x', 'frame', 'particle', 'mass', 'signal', 'size_y', 'size_x', 'relocated']


def test_tensors_in_equal_arrays_in(engine):
    import torch
    for index in (1, 6, 9):     # uint16 (travels as int16), uint8, 3D
        name, frames, kw = RANDOM[index]
        a = cta.find_link_arrays(frames, **kw)
        host = frames.view(np.int16) if frames.dtype == np.uint16 else frames
        b = cta.find_link_arrays(torch.from_numpy(host).cuda(), dtype=frames.dtype, **kw)
        for x, y in zip(a[:7], b[:7]):
            assert np.array_equal(x, y, equal_nan=True)
        assert a.n_tracks == b.n_tracks and np.array_equal(a.coupled, b.coupled)


def test_non_default_stream_gives_the_same_bytes(engine):
    import torch
    name, frames, kw = RANDOM[2]
    a = cta.find_link_arrays(frames, **kw)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = cta.find_link_arrays(frames, **kw)
    s.synchronize()
    for x, y in zip(a[:7], b[:7]):
        assert x.tobytes() == y.tobytes()


def test_noise_size_is_preprocess_then_the_plain_path(engine):
    """maxima and relocation look at the preprocessed frames; mass, signal and size of the located
    rows come from the raw frames, those of the relocated rows from the preprocessed ones"""
    from clustertracking_amd import preprocessing
    name, frames, kw = RANDOM[12]
    a = cta.find_link_arrays(frames, noise_size=1, **kw)
    proc, _ = preprocessing.preprocess_arrays(frames, 1, F._relocate.as_tuple(kw['separation'], 2))
    # (the raw masses decide which located rows pass minmass: the processed block alone cannot
    # say, so the plain path is compared where it has the same rows)
    b = cta.find_link_arrays(proc, **dict(kw, minmass=0))
    assert a.relocated.any()
    key = lambda r: {(int(f), tuple(p)): i for i, (f, p) in enumerate(zip(np.repeat(np.arange(len(r.frame_offset) - 1), np.diff(r.frame_offset)), r.pos.tolist()))}   # noqa: E731
    ka, kb = key(a), key(b)
    n = 0
    for k, i in ka.items():
        if a.relocated[i] and k in kb and b.relocated[kb[k]]:
            assert a.mass[i] == b.mass[kb[k]] and a.signal[i] == b.signal[kb[k]] and a.size[i] == b.size[kb[k]]
            n += 1
    assert n > 0


@pytest.mark.parametrize('index', range(len(BRIGHT)), ids=[c[0] for c in BRIGHT])
def test_nothing_to_find_is_locate_and_link(engine, index):
    name, frames, kw = BRIGHT[index]
    got = cta.find_link_arrays(frames, **kw)
    f = cta.locate(frames, kw['separation'], kw['diameter'], kw['minmass'])
    off = np.r_[0, np.cumsum(np.bincount(f['frame'].values, minlength=len(frames)))]
    ids = cta.link_arrays(f[['y', 'x']].values, off, kw['search_range'], kw['memory'])
    assert not got.relocated.any() and not got.coupled.any()
    assert np.array_equal(got.pos, f[['y', 'x']].values) and np.array_equal(got.frame_offset, off)
    assert np.array_equal(got.particle, ids) and got.n_tracks == ids.max() + 1
    assert got.mass.tobytes() == f['mass'].values.tobytes() and got.signal.tobytes() == f['signal'].values.tobytes()
    sizes = f[[c for c in f.columns if c.startswith('size')]].values
    assert got.size.reshape(len(sizes), -1).tobytes() == np.ascontiguousarray(sizes).tobytes()


def small_correct_call():
    frames, kw = EDGE['lost_pair_1_5']
    check(frames, kw)


def test_refusals_where_the_restatement_refuses(engine):
    frames, kw = EDGE['lost_pair_2_5']
    with pytest.raises(F.Refused):
        F.find_link(frames, max_queries=1, **kw)
    with pytest.raises(_lib.EngineError, match='level 1.*max_queries is 1'):
        cta.find_link_arrays(frames, max_queries=1, **kw)
    small_correct_call()
    frames, kw = EDGE['lost_pair_1_5']
    with pytest.raises(F.Refused):
        F.find_link(frames, max_relocated=1, **kw)
    with pytest.raises(_lib.EngineError, match='level 1.*max_relocated is 1'):
        cta.find_link_arrays(frames, max_relocated=1, **kw)
    small_correct_call()
    frames, kw = F.oversize_case()
    with pytest.raises(lk.SubnetOversizeException):
        F.find_link(frames, **kw)
    with pytest.raises(lk.SubnetOversizeException, match=r'31 points \(level 1\)'):
        cta.find_link_arrays(frames, **kw)
    small_correct_call()
    frames, kw = F.relocate_capacity_case()
    with pytest.raises(F.Refused, match='relocate at level 1'):
        F.find_link(frames, **kw)
    with pytest.raises(_lib.EngineError, match='level 1: a relocation query is beyond'):
        cta.find_link_arrays(frames, **kw)
    small_correct_call()
    frames, kw = F.destinations_case()
    with pytest.raises(F.Refused, match='destinations at level 1'):
        F.find_link(frames, **kw)
    with pytest.raises(_lib.EngineError, match='level 1: a sub-network has 69 destinations'):
        cta.find_link_arrays(frames, **kw)
    small_correct_call()


def test_callbacks_are_refused(engine):
    frames, kw = EDGE['lost_pair_1_5']
    for name in ('before_link', 'after_link', 'refine'):
        with pytest.raises(NotImplementedError):
            cta.find_link(frames, **dict(kw, **{name: lambda **k: None}))


def test_relocate_query_without_sources_finds_nothing(engine):
    """what the loop relies on: a query with an empty source range answers n_found = 0, status 0,
    and leaves the queries next to it alone"""
    frames, kw = EDGE['lost_pair_1_5']
    args = dict(diameter=5, separation=5, search_range=4)
    thr = np.array([F._locate.percentile_threshold(frames[1], 64)])
    known = np.zeros((0, 2))
    one = cta.relocate_arrays(frames[1:], thr, known, [0, 0], [[3., 30.]], [0, 1], [0], **args)
    got = cta.relocate_arrays(frames[1:], thr, known, [0, 0], [[3., 30.]], [0, 0, 1, 1], [0, 0, 0], **args)
    n_found, pos, mass, signal, size, status = got
    assert n_found.tolist() == [0, one[0][0], 0] and one[0][0] >= 1 and status.tolist() == [0, 0, 0]
    assert (pos[[0, 2]] == -1).all() and np.isnan(mass[[0, 2]]).all()
    for x, y in zip(got[1:5], one[1:5]):
        assert np.array_equal(x[1], y[0], equal_nan=True)
