"""Feature location on the MI355X (ctr_locate_maxima_device): equal to the
reference's grey_dilation on every fixture, to the SciPy composition on seeded random frames,
frame by frame inside a batch, and good enough to start refine_leastsq from."""
import functools
import zlib

import numpy as np
import pandas as pd
import pytest
from scipy.spatial import cKDTree

import _locate
import clustertracking_amd as cta
from clustertracking_amd import find

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16, np.int16, np.int32, np.float32, np.float64)


def _same(got, expect):
    assert got.dtype == expect.dtype and got.shape == expect.shape
    np.testing.assert_array_equal(got, expect)


def _frame(rng, shape, dt, n_blobs=None):
    ndim = len(shape)
    im = np.zeros(shape)
    grid = np.indices(shape).astype(np.float64)
    for _ in range(n_blobs if n_blobs is not None else rng.randint(0, 8)):
        c = [rng.uniform(0, s) for s in shape]
        im += rng.uniform(20, 100) * np.exp(-sum(((g - ci) / 2.) ** 2 for g, ci in zip(grid, c)) * ndim / 2)
    im += rng.uniform(0, 8, shape)
    if np.dtype(dt).kind == 'f':
        im = im - rng.uniform(0, 20) * (rng.rand() < 0.3)
    im[rng.rand(*shape) < 0.2] = 0
    if np.dtype(dt).kind in 'ui':
        im = np.round(im * (1 if dt == np.uint8 else 37))
        if np.dtype(dt).kind == 'i':
            im -= 200
    return im.astype(dt)


@pytest.mark.parametrize('case', _locate.fixtures(), ids=lambda c: c[0])
def test_fixture(case):
    name, frame, kw, expect, thr = case
    _same(find.grey_dilation(frame, **kw), expect)
    pos, off, t = find.locate_arrays(frame[None], **kw)
    assert off.tolist() == [0, len(expect)]
    assert t[0].tobytes() == np.float64(thr).tobytes() or (np.isnan(t[0]) and np.isnan(thr))


@pytest.mark.parametrize('dt', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('geom', [((40, 52), 6, True), ((33, 47), (5, 8), True), ((40, 40), 5, False),
                                  ((10, 16, 18), (3, 5, 6), True)], ids=['2d', '2d_aniso', '2d_loose', '3d'])
def test_random_frames_equal_composition(dt, geom):
    shape, sep, precise = geom
    rng = np.random.RandomState(zlib.crc32(repr((np.dtype(dt).name, shape)).encode()))
    n = 200 if len(shape) == 2 else 60
    frames = np.stack([_frame(rng, shape, dt) for _ in range(n)])
    pct = [64, 30, 90][len(shape) % 3]
    pos, off, thr = find.locate_arrays(frames, sep, percentile=pct, precise=precise)
    for t in range(n):
        expect = _locate.compose(frames[t], sep, pct, precise=precise)
        got = pos[off[t]:off[t + 1]].astype(np.int64)
        if len(expect) == 0:
            assert len(got) == 0, t
        else:
            _same(got, expect)
        ref_thr = np.float64(find.percentile_threshold(frames[t], pct))
        assert thr[t].tobytes() == ref_thr.tobytes() or (np.isnan(thr[t]) and np.isnan(ref_thr)), t


def test_batch_equals_single_frames():
    rng = np.random.RandomState(5)
    frames = np.stack([_frame(rng, (48, 70), np.uint16, 6) for _ in range(7)])
    frames[3] = 0
    f = find.locate_maxima(frames, (5, 7), percentile=50)
    assert list(f.columns) == ['y', 'x', 'frame'] and f['y'].dtype == np.float64
    for t in range(len(frames)):
        one = find.grey_dilation(frames[t], (5, 7), percentile=50)
        rows = f[f['frame'] == t][['y', 'x']].values
        np.testing.assert_array_equal(rows, one.reshape(-1, 2).astype(np.float64))
    assert not (f['frame'] == 3).any()


@functools.lru_cache(maxsize=None)
def _tiny_frames():
    """2049 frames of 16 x 16 pixels (one chunk of mask words each) and the composition frame by frame"""
    rng = np.random.RandomState(16)
    frames = np.stack([_frame(rng, (16, 16), np.uint8, rng.randint(0, 3)) for _ in range(2049)])
    frames[[5, 1023, 1024]] = 0
    return frames, [_locate.compose(f, 4, 50).reshape(-1, 2) for f in frames]


@pytest.mark.parametrize('n_frames', [1023, 1024, 1025, 2049])
def test_batch_equals_single_frames_at_the_chunk_of_the_scan(n_frames):
    """the chunk counts are scanned by one workgroup of 1024, one chunk per frame here: one frame
    short of its width, the width, one over, two and one over"""
    frames, single = _tiny_frames()
    pos, off, _ = find.locate_arrays(frames[:n_frames], 4, percentile=50)
    want = np.concatenate(single[:n_frames])
    assert off.tolist() == np.r_[0, np.cumsum([len(s) for s in single[:n_frames]])].tolist()
    np.testing.assert_array_equal(pos.astype(np.int64), want.astype(np.int64))
    assert len(want) > n_frames // 2 and any(len(s) == 0 for s in single[:n_frames])


def test_torch_frames_from_draw_frames():
    import torch
    from clustertracking_amd import device
    rng = np.random.RandomState(6)
    pos = rng.uniform(10, 118, (60, 2))
    frame_of = np.repeat(np.arange(3), 20)
    for dt in (np.uint8, np.uint16):
        t = device.draw_frames((128, 128), frame_of, pos, 3., 200 if dt == np.uint8 else 3000, n_frames=3,
                               noise=10., seed=1, dtype=dt)
        host = t.cpu().numpy()
        if dt == np.uint16:
            host = host.view(np.uint16)
        a = find.locate_maxima(t, 9, dtype=dt)
        b = find.locate_maxima(host, 9)
        pd.testing.assert_frame_equal(a, b)
        assert len(a) > 30
    with pytest.raises(ValueError):
        find.locate_maxima(torch.zeros((1, 8, 8), dtype=torch.uint8, device='cuda:0'), 3, dtype=np.uint16)


def test_capacity_overflow_retries():
    im = np.full((64, 64), 7, np.uint8)
    im[::5, ::3] = 0
    im[20:40, 10:50] = 200            # a plateau: every pixel of it is a maximum
    expect = _locate.compose(im, 3, precise=False)
    assert len(expect) > 100
    pos, off, _ = find.locate_arrays(im[None], 3, precise=False, capacity=10)
    _same(pos.astype(np.int64), expect)
    assert off.tolist() == [0, len(expect)]
    _same(find.grey_dilation(im, 3), _locate.compose(im, 3))


def test_invalid_arguments_raise():
    im = np.ones((2, 16, 16), np.uint8)
    with pytest.raises(ValueError):
        find.locate_arrays(im, 3, percentile=101)
    with pytest.raises(ValueError):
        find.locate_arrays(im, 3, percentile=-1)
    with pytest.raises(ValueError):
        find.locate_arrays(im, 3, margin=-1)
    with pytest.raises(ValueError):
        find.locate_arrays(im, -2)
    with pytest.raises(ValueError):
        find.locate_arrays(np.ones((2, 16), np.uint8), 3)
    with pytest.raises(ValueError):
        find.locate_arrays(np.ones((2, 16, 16), np.int64), 3)


def test_cfg2_end_to_end():
    """Located maxima find every isolated true feature (the maximum is the pixel of the truth or
    one of its neighbours), and refine_leastsq from them reaches the reference's accuracy bar
    (RMS < 0.05 px at S/N 10; BASELINE 1) on the isolated features.  Isolated: no other true
    feature within the separation + 2 px, since each integer maximum may sit a pixel off its
    feature; closer pairs can merge into one maximum or lose one to suppression, by design."""
    from clustertracking_amd import workloads
    frames, _, truth, opts = workloads.cfg2(n_frames=4)
    sep = opts['diameter']
    f = find.locate_maxima(frames, sep)
    truth = truth.reshape(len(frames), -1, 2)
    f0 = f.copy()
    f0['signal'] = 90.
    f0['size'] = 3.
    f0['background'] = 5.
    res = cta.refine_leastsq(f0, cta.ArrayReader(frames), diameter=sep, separation=sep)
    errs = []
    for t in range(len(frames)):
        tr = truth[t]
        d, _ = cKDTree(tr).query(tr, 2)
        isolated = tr[d[:, 1] > sep + 2]
        mine = f[f['frame'] == t][['y', 'x']].values
        d1, _ = cKDTree(mine).query(np.round(isolated), p=np.inf)
        assert len(isolated) > 50 and np.all(d1 <= 1.0), (t, d1.max())
        fitted = res[res['frame'] == t][['y', 'x']].values
        d2, _ = cKDTree(fitted).query(isolated)
        errs.append(d2)
    rms = np.sqrt(np.mean(np.concatenate(errs) ** 2))
    assert rms < 0.05, rms
