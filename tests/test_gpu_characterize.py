"""Characterisation on the MI355X (ctr_characterize_device): equal to the
reference's characterize on every fixture, to the NumPy yardstick on seeded random cases, frame
by frame inside a batch, and -- chained behind the feature location in ``cta.locate`` -- enough
to start refine_leastsq from without a hand-set value.

Tolerances.  Integer frames: the sums are exact integers on both sides, so ``mass`` and
``signal`` are equal and ``size`` (one division, one square root) agrees to rtol 1e-14.  Float
frames: ``signal`` is equal; ``mass`` and ``size`` agree to the bound of plain summation of the
window in the frame's own precision, n_window * 2^-24 (float32: the reference's mass IS a float32
sum) or n_window * 2^-53 (float64).  That bound is relative to sum(|pixel|), which is |sum(pixel)|
only where the pixels of a window have one sign: the random float frames are therefore
non-negative or non-positive, never mixed."""
import zlib

import numpy as np
import pandas as pd
import pytest
from scipy.spatial import cKDTree

import _characterize
import _locate
import clustertracking_amd as cta
from clustertracking_amd import find

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16, np.int16, np.int32, np.float32, np.float64)


def _compare(got, expect, dtype, radius, isotropic, ndim):
    keys = ['mass', 'signal'] + _characterize.size_keys(ndim, isotropic)
    assert list(got) == keys and list(expect) == keys
    for k in keys:
        assert got[k].dtype == np.float64 and got[k].shape == expect[k].shape, k
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(expect[k]), err_msg=k)
    np.testing.assert_array_equal(got['signal'], expect['signal'])
    if np.dtype(dtype).kind in 'ui':
        np.testing.assert_array_equal(got['mass'], expect['mass'])
        rtol = 1e-14
    else:
        rtol = _characterize.float_rtol(dtype, radius)
        np.testing.assert_allclose(got['mass'], expect['mass'], rtol=rtol, atol=0)
    for k in keys[2:]:
        np.testing.assert_allclose(got[k], expect[k], rtol=rtol, atol=0, err_msg=k)


@pytest.mark.parametrize('case', _characterize.fixtures(), ids=lambda c: c[0])
def test_fixture(case):
    name, image, coords, kw, expect = case
    got = cta.characterize(coords, image, **kw)
    _compare(got, expect, image.dtype, kw['radius'], kw['isotropic'], image.ndim)


def _frame(rng, shape, dt):
    ndim = len(shape)
    im = np.zeros(shape)
    grid = np.indices(shape).astype(np.float64)
    for _ in range(rng.randint(1, 6)):
        c = [rng.uniform(0, s) for s in shape]
        im += rng.uniform(20, 100) * np.exp(-sum(((g - ci) / 2.5) ** 2 for g, ci in zip(grid, c)) * ndim / 2)
    im += rng.uniform(0, 8, shape)
    im[rng.rand(*shape) < 0.1] = 0
    if np.dtype(dt).kind == 'f':
        if rng.rand() < 0.3:
            im = -im           # one sign per frame (module docstring)
    else:
        im = np.round(im * (1 if dt == np.uint8 else 37))
        if np.dtype(dt).kind == 'i':
            im -= 600          # mixed signs: exact in integers
    return im.astype(dt)


GEOMETRIES = [((28, 33), (4, 4), True), ((28, 33), (6, 6), True), ((30, 26), (3, 7), False), ((31, 37), (9, 9), True),
              ((27, 29), (11, 8), False), ((9, 13, 15), (2, 3, 3), False), ((10, 12, 14), (3, 3, 3), True),
              ((8, 16, 16), (1, 5, 4), False)]


@pytest.mark.parametrize('dt', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('geom', GEOMETRIES, ids=lambda g: '%dd_r%s_%s' % (len(g[0]), '_'.join(map(str, g[1])), 'iso' if g[2] else 'aniso'))
def test_random_cases_equal_yardstick(dt, geom):
    """6 types x 8 geometries x 80 centres = 3840 cases, every one compared: centres uniform over
    the frame and up to a radius beyond it, a quarter of them on integers, a quarter on halves."""
    shape, radius, isotropic = geom
    rng = np.random.RandomState(zlib.crc32(repr((np.dtype(dt).name, shape, radius)).encode()))
    n_frames, per_frame = 4, 20
    frames = np.stack([_frame(rng, shape, dt) for _ in range(n_frames)])
    pos = np.stack([rng.uniform(-r, n - 1 + r, n_frames * per_frame) for n, r in zip(shape, radius)], 1)
    pos[::4] = np.round(pos[::4])
    pos[1::4] = np.floor(pos[1::4]) + 0.5
    offset = np.arange(n_frames + 1) * per_frame
    mass, signal, size = find.characterize_arrays(frames, pos, offset, radius, isotropic)
    keys = _characterize.size_keys(len(shape), isotropic)
    for t in range(n_frames):
        rows = slice(offset[t], offset[t + 1])
        got = dict(mass=mass[rows], signal=signal[rows])
        for a, k in enumerate(keys):
            got[k] = size[rows] if isotropic else size[rows, a]
        expect = _characterize.compose(pos[rows], frames[t], radius, isotropic)
        _compare(got, expect, dt, radius, isotropic, len(shape))


def _batch(dt=np.uint16, seed=5, n_frames=5, shape=(40, 56)):
    rng = np.random.RandomState(seed)
    frames = np.stack([_frame(rng, shape, dt) for _ in range(n_frames)])
    counts = np.array([7, 0, 12, 1, 9][:n_frames])
    offset = np.r_[0, np.cumsum(counts)].astype(np.int64)
    pos = np.stack([rng.uniform(-3, n + 2, offset[-1]) for n in shape], 1)
    return frames, pos, offset


def test_batch_equals_single_frames():
    frames, pos, offset = _batch()
    for isotropic, radius in ((True, (5, 5)), (False, (4, 6))):
        mass, signal, size = find.characterize_arrays(frames, pos, offset, radius, isotropic)
        assert size.shape == ((len(pos),) if isotropic else (len(pos), 2))
        for t in range(len(frames)):
            rows = slice(offset[t], offset[t + 1])
            one = cta.characterize(pos[rows], frames[t], radius, isotropic)
            np.testing.assert_array_equal(mass[rows], one['mass'])
            np.testing.assert_array_equal(signal[rows], one['signal'])
            one_size = one['size'] if isotropic else np.stack([one['size_y'], one['size_x']], 1)
            np.testing.assert_array_equal(size[rows], one_size)


def test_empty_table():
    frames, _, _ = _batch()
    mass, signal, size = find.characterize_arrays(frames, np.empty((0, 2)), np.zeros(len(frames) + 1, np.int64), (3, 3), False)
    assert mass.shape == (0,) and signal.shape == (0,) and size.shape == (0, 2)
    res = cta.characterize(np.empty((0, 2)), frames[0], (3, 3))
    assert list(res) == ['mass', 'signal', 'size'] and len(res['size']) == 0


def test_tensor_inputs_and_integer_positions_and_stream():
    """torch tensors on the device = ndarrays; int32 positions = the same positions as float64, bit
    for bit; a call on a non-default torch stream."""
    import torch
    for dt in (np.uint8, np.uint16, np.float32):
        frames, pos, offset = _batch(dt, seed=8)
        pos = np.round(pos)
        ref = find.characterize_arrays(frames, pos, offset, (5, 5), True)
        got = find.characterize_arrays(frames, pos.astype(np.int32), offset, (5, 5), True)
        for a, b in zip(got, ref):
            assert a.tobytes() == b.tobytes()
        host = frames.view(np.int16) if dt == np.uint16 else frames
        t = torch.from_numpy(host).cuda()
        args = (torch.from_numpy(pos.astype(np.int32)).cuda(), torch.from_numpy(offset).cuda(), (5, 5), True)
        got = find.characterize_arrays(t, *args, dtype=dt)
        for a, b in zip(got, ref):
            assert a.tobytes() == b.tobytes()
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            got = find.characterize_arrays(t, torch.from_numpy(pos).cuda(), offset, (5, 5), True, dtype=dt)
        stream.synchronize()
        for a, b in zip(got, ref):
            assert a.tobytes() == b.tobytes()


def test_scale_factor_from_metadata():
    class Frame(np.ndarray):
        pass
    frames, pos, offset = _batch(np.uint8)
    image = frames[0].view(Frame)
    image.metadata = {'scale_factor': 4.}
    plain = cta.characterize(pos[:7], frames[0], (4, 4))
    scaled = cta.characterize(pos[:7], image, (4, 4))
    np.testing.assert_array_equal(scaled['mass'], plain['mass'] / 4.)
    np.testing.assert_array_equal(scaled['signal'], plain['signal'] / 4.)
    np.testing.assert_array_equal(scaled['size'], plain['size'])
    np.testing.assert_array_equal(cta.characterize(pos[:7], image, (4, 4), scale_factor=1.)['mass'], plain['mass'])


def test_invalid_arguments_raise():
    frames, pos, offset = _batch()
    with pytest.raises(ValueError):
        find.characterize_arrays(frames, pos, offset, (-1, 3))
    with pytest.raises(ValueError):
        find.characterize_arrays(frames, pos, offset, (2.5, 3))
    with pytest.raises(ValueError):
        find.characterize_arrays(frames, pos, offset[:-1], (3, 3))
    with pytest.raises(ValueError):
        find.characterize_arrays(frames, pos[:, :1], offset, (3, 3))
    with pytest.raises(ValueError):
        find.characterize_arrays(frames.astype(np.int64), pos, offset, (3, 3))
    with pytest.raises(ValueError):
        find.characterize_arrays(frames, pos, offset, (3, 3), scale_factor=0.)


def _expected_locate(frames, separation, diameter, minmass, margin):
    f = find.locate_maxima(frames, separation, margin=margin)
    ndim = frames.ndim - 1
    cols = ['z', 'y', 'x'][3 - ndim:]
    radius = tuple(int(d // 2) for d in diameter)
    isotropic = len(set(diameter)) == 1
    parts = []
    for t in range(len(frames)):
        rows = f[f['frame'] == t]
        ch = _characterize.compose(rows[cols].values, frames[t], radius, isotropic)
        part = rows[cols].copy()
        for k, v in ch.items():
            part[k] = v
        part['frame'] = rows['frame']
        parts.append(part)
    out = pd.concat(parts)
    return out[out['mass'] >= minmass].reset_index(drop=True)


@pytest.mark.parametrize('geom', [((6, 64, 72), 9, (9, 9), np.uint8), ((5, 60, 60), (7, 9), (5, 9), np.uint16),
                                  ((4, 16, 48, 48), (3, 7, 7), (5, 7, 7), np.uint8),
                                  ((4, 16, 40, 40), 5, (5, 5, 5), np.int16)], ids=['2d', '2d_aniso', '3d_aniso', '3d_iso'])
def test_locate_equals_maxima_plus_yardstick(geom):
    shape, sep, diameter, dt = geom
    rng = np.random.RandomState(zlib.crc32(repr(shape).encode()))
    frames = np.stack([_frame(rng, shape[1:], dt) for _ in range(shape[0])])
    sep_t = (sep,) * (len(shape) - 1) if not isinstance(sep, tuple) else sep
    margin = tuple(int(max(d // 2, s // 2 - 1)) for d, s in zip(diameter, sep_t))
    everything = _expected_locate(frames, sep, diameter, -np.inf, margin)
    assert len(everything) > 10
    cut = float(np.median(everything['mass']))     # (the int16 frames have negative masses too)
    for minmass in (0, cut, abs(everything['mass'].max()) * 2 + 1):
        expect = _expected_locate(frames, sep, diameter, minmass, margin)
        got = cta.locate(frames, sep, diameter=diameter, minmass=minmass)
        if minmass == cut:
            assert 3 <= len(expect) < len(everything)
        assert list(got.columns) == list(expect.columns)
        assert [got[c].dtype for c in got] == [expect[c].dtype for c in expect]
        assert len(got) == len(expect) and list(got.index) == list(expect.index)
        for c in got:
            if c.startswith('size'):
                np.testing.assert_array_equal(np.isnan(got[c]), np.isnan(expect[c]))
                np.testing.assert_allclose(got[c].values, expect[c].values, rtol=1e-14, atol=0)
            else:
                np.testing.assert_array_equal(got[c].values, expect[c].values)
    assert list(got.columns) == ['z', 'y', 'x'][4 - len(shape):] + ['mass', 'signal'] + \
        _characterize.size_keys(len(shape) - 1, len(set(diameter)) == 1) + ['frame']
    assert len(got) == 0       # the last minmass is above every mass: an empty table with the columns


def test_locate_default_diameter_is_the_separation():
    rng = np.random.RandomState(11)
    frames = np.stack([_frame(rng, (50, 50), np.uint8) for _ in range(3)])
    pd.testing.assert_frame_equal(cta.locate(frames, 9), cta.locate(frames, 9, diameter=9))
    pd.testing.assert_frame_equal(cta.locate(frames, 9), cta.locate(frames, 9, diameter=(9, 9), margin=4))


def test_cfg2_end_to_end_without_hand_set_start_values():
    """locate -> refine_leastsq with characterize's signal and size as the start values: every row
    lies within 2 px of a true feature (minmass has dropped the noise maxima), every isolated
    true feature (tests/test_gpu_locate.py's definition) has a row within one pixel, no cluster
    fails, and the RMS error on the isolated features is below the reference's bar of 0.05 px.
    Host composition of the same chain on these two frames: 1091 maxima, 342 rows for every
    minmass in 1500 .. 3000 (noise maxima have mass <= 1237, true features >= 3739)."""
    from clustertracking_amd import workloads
    frames, _, truth, opts = workloads.cfg2(n_frames=2)
    sep = opts['diameter']
    assert sep == 13
    f = cta.locate(frames, 13, minmass=2000)
    assert len(f) == 342
    assert list(f.columns) == ['y', 'x', 'mass', 'signal', 'size', 'frame']
    start = f.copy()
    start['background'] = 5.
    res = cta.refine_leastsq(start, cta.ArrayReader(frames), diameter=13, separation=13)
    assert len(res) == len(f) and not res['cost'].isnull().any()      # cost NaN: a failed cluster
    truth = truth.reshape(len(frames), -1, 2)
    errs = []
    for t in range(len(frames)):
        tr = truth[t]
        mine = f[f['frame'] == t][['y', 'x']].values
        d0, _ = cKDTree(tr).query(mine)
        print('frame %d: %d rows, farthest from a true feature %.3f px' % (t, len(mine), d0.max()))
        assert np.all(d0 < 2.0), (t, d0.max())
        d, _ = cKDTree(tr).query(tr, 2)
        isolated = tr[d[:, 1] > sep + 2]
        d1, _ = cKDTree(mine).query(np.round(isolated), p=np.inf)
        assert len(isolated) > 50 and np.all(d1 <= 1.0), (t, d1.max())
        fitted = res[res['frame'] == t][['y', 'x']].values
        d2, _ = cKDTree(fitted).query(isolated)
        errs.append(d2)
    rms = np.sqrt(np.mean(np.concatenate(errs) ** 2))
    print('RMS on %d isolated features: %.4f px' % (len(np.concatenate(errs)), rms))
    assert rms < 0.05, rms
