"""Preprocessing on the MI355X (ctr_preprocess_device): equal to the reference's
fixtures and to the NumPy / SciPy yardstick (tests/_preprocess.py) bit for bit on integer frames,
within the stated rounding bounds on float frames, and -- in front of the feature location in
``cta.locate`` -- equal to the host composition row for row.

Float bounds.  The Gaussian chain is the same float64 operations in the same order on both
sides: ``lowpass`` is equal.  The background of a float frame is summed in a different order
(SciPy keeps a running sum): float32 frames round the background once per axis pass,
|d| <= ndim * 2^-22 * max|pixel|; float64 frames sum llong[a] terms per pass,
|d| <= sum(llong) * 2^-51 * max|pixel|.  The uint8 output differs by at most one level in at most
3 * p_ref of the pixels (floor: 2 per frame), p_ref being the share of pixels where the
yardstick itself changes when its box sums are taken in np.longdouble."""
import zlib

import numpy as np
import pandas as pd
import pytest
from scipy.spatial import cKDTree

import _characterize
import _locate
import _preprocess
import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib, find

pytestmark = pytest.mark.gpu

preprocessing = cta.preprocessing      # (AttributeError before the feature)
FIXTURES = _preprocess.fixtures()
INT_TYPES = (np.uint8, np.uint16, np.int16, np.int32)


def _is_int(a):
    return np.issubdtype(a.dtype, np.integer)


def _band_bound(raw, llong):
    llong = _preprocess.validate_tuple(llong, raw.ndim)
    peak = float(np.abs(raw).max())
    if raw.dtype == np.float32:
        return raw.ndim * 2. ** -22 * peak
    return sum(llong) * 2. ** -51 * peak


def _check_band(band, raw, lshort, llong, thr, label=''):
    """float ``bandpass`` against the yardstick: every pixel within the bound of the module
    docstring.  The bound is on the band BEFORE the threshold; a pixel whose yardstick band lies
    within the bound of the threshold may legally fall on either side of it, so there the device's
    value is 0 or within the bound of the unthresholded band -- nothing else.  Such pixels are
    rare (the bound is some 1e-7 or 1e-15 of a grey level): at most 1 in 1000, floor 1."""
    bound = _band_bound(raw, llong)
    if thr is None:
        thr = 1 / 255.
    expect = _preprocess.bandpass(raw, lshort, llong, thr)
    unthresholded = _preprocess._gaussian_chain(raw, _preprocess.validate_tuple(lshort, raw.ndim)) - \
        _preprocess.boxcar(raw, llong)
    sure = np.abs(unthresholded - thr) > bound
    assert (~sure).sum() <= max(1e-3 * raw.size, 1)
    worst = np.abs(band - expect)[sure].max() if sure.any() else 0.
    print('%s max |band - yardstick| %.3e, bound %.3e, %d pixels at the threshold' % (label, worst, bound, (~sure).sum()))
    assert worst <= bound
    edge = band[~sure]
    assert np.all((edge == 0) | (np.abs(edge - unthresholded[~sure]) <= bound))
    return bound, float(expect.max())


def _scale_rtol(bound, band_max):
    """scale_factor = 255 / max(band): a band within `bound` moves it by bound / max(band)
    relatively (first order; doubled for the second order and the division's own rounding)"""
    return 2 * bound / band_max


def _check_u8(got, raw, noise, smooth, thr, label='', chosen=True):
    """the uint8 output of float frames against SciPy's, by the p_ref rule of the module docstring"""
    expect, _ = _preprocess.preprocess(raw, noise, smooth, thr)
    other, _ = _preprocess.preprocess(raw, noise, smooth, thr, bandpass=_preprocess.bandpass_longdouble)
    p_ref = np.mean(expect != other)
    diff = np.abs(got.astype(np.int64) - expect.astype(np.int64))
    share = np.mean(diff != 0)
    print('%s p_ref %.3e device share %.3e (%d of %d pixels)' % (label, p_ref, share, (diff != 0).sum(), diff.size))
    if chosen:      # frames this file generates are chosen so; a fixture of 300 pixels has p_ref 0 or >= 3e-3
        assert p_ref < 1e-3
    assert diff.max() <= 1
    assert (diff != 0).sum() <= max(3 * p_ref * diff.size, 2)
    return p_ref, share


@pytest.mark.parametrize('case', FIXTURES, ids=lambda c: c[0])
def test_fixture(case, engine):
    name, raw, kw, expect = case
    image, scale = cta.preprocess(raw, **kw)
    assert image.dtype == expect['image'].dtype and image.shape == raw.shape and isinstance(scale, float)
    dark = not np.isfinite(expect['scale_factor'])
    if dark:                    # the reference casts NaN here: zeros and inf are this project's rule
        assert scale == np.inf and not image.any()
    elif _is_int(raw):
        assert scale == float(expect['scale_factor'])
        np.testing.assert_array_equal(image, expect['image'])
    elif kw['noise_size'] is None:      # a float frame only rescaled: no sum, no order
        assert scale == float(expect['scale_factor'])
        np.testing.assert_array_equal(image, expect['image'])
    else:
        _check_u8(image, raw, kw['noise_size'], kw['smoothing_size'], kw['threshold'], name, chosen=False)
    if kw['noise_size'] is None:
        return
    low = cta.lowpass(raw, kw['noise_size'])
    assert low.dtype == np.float64
    np.testing.assert_array_equal(low, expect['lowpass'])
    band = cta.bandpass(raw, kw['noise_size'], kw['smoothing_size'], kw['threshold'])
    assert band.dtype == np.float64
    if _is_int(raw):
        np.testing.assert_array_equal(band, expect['bandpass'])
    else:
        bound, band_max = _check_band(band, raw, kw['noise_size'], kw['smoothing_size'], kw['threshold'], name)
        if not dark:
            np.testing.assert_allclose(scale, float(expect['scale_factor']), rtol=_scale_rtol(bound, band_max), atol=0)


def _random_frame(rng, shape, dt):
    ndim = len(shape)
    im = np.zeros(shape)
    grid = np.indices(shape).astype(np.float64)
    for _ in range(rng.randint(1, 5)):
        c = [rng.uniform(0, s) for s in shape]
        im += rng.uniform(30, 100) * np.exp(-sum(((g - ci) / 2.5) ** 2 for g, ci in zip(grid, c)) * ndim / 2)
    im += rng.uniform(0, 10, shape) + rng.uniform(0, 1) * grid[-1]
    dt = np.dtype(dt)
    if dt.kind == 'f':
        return (im / 256.).astype(dt)
    # im < 4 * 100 + 10 + 200: scaled to fill most of the type, signed types shifted below zero
    im = np.round(im / 610. * {'u1': 250, 'u2': 60000, 'i2': 40000, 'i4': 2.3e9}[dt.str[1:]])
    if dt.kind == 'i':
        im -= {2: 9000, 4: 3e8}[dt.itemsize]
    return im.astype(dt)


# odd shapes, none a multiple of the 16 x 64 tile; 2D and 3D; per-axis sizes
GEOMETRIES = [((5, 37, 71), 1, 7), ((3, 67, 133), (0.8, 1.6), (9, 5)), ((4, 21, 200), (1, 0), (3, 15)),
              ((6, 18, 65), 2, 13), ((3, 7, 19, 70), 1, (3, 5, 7)), ((2, 9, 33, 35), (0.5, 1, 1.5), (5, 7, 9)),
              ((3, 5, 17, 129), (0, 1, 1), (1, 9, 9)), ((2, 11, 16, 64), (1, 0, 1), (5, 1, 3))]


@pytest.mark.parametrize('dt', INT_TYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('geom', GEOMETRIES, ids=lambda g: 'x'.join(map(str, g[0])))
def test_random_integer_frames_equal_yardstick(dt, geom, engine):
    """4 types x 8 geometries x 3 rounds of 2-6 frames (over 300 frames in all): preprocess,
    bandpass and lowpass of the block equal the yardstick frame by frame, bit for bit"""
    shape, noise, smooth = geom
    rng = np.random.RandomState(zlib.crc32(repr((np.dtype(dt).name, geom)).encode()))
    for _ in range(3):
        frames = np.stack([_random_frame(rng, shape[1:], dt) for _ in range(shape[0])])
        thr = [None, 0, float(rng.uniform(-30, 2))][rng.randint(3)]
        images, scales = preprocessing.preprocess_arrays(frames, noise, smooth, thr)
        bands = preprocessing.bandpass_arrays(frames, noise, smooth, thr)
        lows = preprocessing.lowpass_arrays(frames, noise, thr)
        assert images.dtype == np.dtype(dt) and scales.dtype == np.float64 and scales.shape == (len(frames),)
        for t, raw in enumerate(frames):
            expect, scale = _preprocess.preprocess(raw, noise, smooth, thr)
            assert np.isfinite(scale)
            assert scales[t] == scale
            np.testing.assert_array_equal(images[t], expect)
            np.testing.assert_array_equal(bands[t], _preprocess.bandpass(raw, noise, smooth, thr))
            np.testing.assert_array_equal(lows[t], _preprocess.lowpass(raw, noise, thr))


FLOAT_GEOMETRIES = [((3, 128, 192), 1, 7), ((2, 96, 150), (1, 1.5), (9, 13)), ((2, 12, 64, 80), 1, (3, 7, 7))]


@pytest.mark.parametrize('dt', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('geom', FLOAT_GEOMETRIES, ids=lambda g: 'x'.join(map(str, g[0])))
def test_float_frames_within_the_bounds(dt, geom, engine):
    shape, noise, smooth = geom
    rng = np.random.RandomState(zlib.crc32(repr((np.dtype(dt).name, geom)).encode()))
    frames = np.stack([_random_frame(rng, shape[1:], dt) for _ in range(shape[0])])
    lows = preprocessing.lowpass_arrays(frames, noise)
    bands = preprocessing.bandpass_arrays(frames, noise, smooth)
    images, scales = preprocessing.preprocess_arrays(frames, noise, smooth)
    assert images.dtype == np.uint8
    for t, raw in enumerate(frames):
        np.testing.assert_array_equal(lows[t], _preprocess.lowpass(raw, noise))
        bound, band_max = _check_band(bands[t], raw, noise, smooth, None, '%s frame %d:' % (np.dtype(dt).name, t))
        _, scale = _preprocess.preprocess(raw, noise, smooth)
        np.testing.assert_allclose(scales[t], scale, rtol=_scale_rtol(bound, band_max), atol=0)
        _check_u8(images[t], raw, noise, smooth, None, '%s frame %d:' % (np.dtype(dt).name, t))


def _u16_batch(seed=3, n=5, shape=(45, 83)):
    rng = np.random.RandomState(seed)
    return np.stack([_random_frame(rng, shape, np.uint16) for _ in range(n)])


def test_batch_equals_frame_by_frame(engine):
    frames = _u16_batch()
    images, scales = preprocessing.preprocess_arrays(frames, 1, 9)
    bands = preprocessing.bandpass_arrays(frames, 1, 9)
    for t in range(len(frames)):
        one, scale = cta.preprocess(frames[t], 1, 9)
        assert one.tobytes() == images[t].tobytes() and scale == scales[t]
        assert cta.bandpass(frames[t], 1, 9).tobytes() == bands[t].tobytes()


def test_both_scaling_strategies_agree(engine):
    for frames in (_u16_batch(), np.stack([_u16_batch(4, 3, (9, 20, 33))[0]] * 2).astype(np.uint8)):
        a = preprocessing.preprocess_arrays(frames, 1, 7, _strategy=_abi.PRE_BAND_PLANE)
        b = preprocessing.preprocess_arrays(frames, 1, 7, _strategy=_abi.PRE_TWICE)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_tensor_input_stream_and_uint16_view(engine):
    import torch
    frames = _u16_batch(5)
    ref_images, ref_scales = preprocessing.preprocess_arrays(frames, 1, 9)
    ref_band = preprocessing.bandpass_arrays(frames, 1, 9)
    t = torch.from_numpy(frames.view(np.int16)).cuda()
    images, scales = preprocessing.preprocess_arrays(t, 1, 9, dtype=np.uint16)    # int16 tensor read as uint16
    assert images.dtype == np.uint16 and images.tobytes() == ref_images.tobytes()
    assert scales.tobytes() == ref_scales.tobytes()
    signed = preprocessing.preprocess_arrays(t, 1, 9)[0]                          # ... and as what it is
    assert signed.dtype == np.int16
    np.testing.assert_array_equal(signed[0], _preprocess.preprocess(frames[0].view(np.int16), 1, 9)[0])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        band = preprocessing.bandpass_arrays(t, 1, 9, dtype=np.uint16)
        dev_images, dev_scales, pix = preprocessing.preprocess_arrays(t, 1, 9, dtype=np.uint16, _on_device=True)
    stream.synchronize()
    assert band.tobytes() == ref_band.tobytes()
    assert pix == np.uint16 and dev_images.is_cuda and dev_images.dtype == torch.int16
    assert dev_images.cpu().numpy().view(np.uint16).tobytes() == ref_images.tobytes()
    assert dev_scales.cpu().numpy().tobytes() == ref_scales.tobytes()
    for dt in (np.uint8, np.float32):
        fr = np.stack([_random_frame(np.random.RandomState(6), (40, 70), dt)] * 2)
        a = preprocessing.preprocess_arrays(fr, 1, 7)
        b = preprocessing.preprocess_arrays(torch.from_numpy(fr).cuda(), 1, 7)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_without_noise_size(engine):
    frames = _u16_batch(7)
    images, scales = preprocessing.preprocess_arrays(frames)
    assert images.dtype == np.uint16 and images.tobytes() == frames.tobytes()
    np.testing.assert_array_equal(scales, np.ones(len(frames)))
    for dt in (np.float32, np.float64):
        fr = np.stack([_random_frame(np.random.RandomState(8 + k), (33, 70), dt) - 0.02 for k in range(3)])
        images, scales = preprocessing.preprocess_arrays(fr)
        for t in range(3):
            expect, scale = _preprocess.preprocess(fr[t])
            assert scales[t] == scale
            np.testing.assert_array_equal(images[t], expect)


def test_dark_frame_gives_zeros_and_inf(engine):
    frames = _u16_batch(9, 3).astype(np.uint8)
    frames[1] = 0
    images, scales = preprocessing.preprocess_arrays(frames, 1, 7)
    assert scales[1] == np.inf and not images[1].any()
    assert np.isfinite(scales[[0, 2]]).all() and images[0].max() >= 254 and images[2].max() >= 254
    flat = np.full((2, 30, 40), 77, np.uint8)                  # no band at all, 3D and float too
    assert not preprocessing.preprocess_arrays(flat, 1, 5)[0].any()
    images, scales = preprocessing.preprocess_arrays(np.zeros((2, 4, 20, 30), np.float32), 1, 5)
    assert images.dtype == np.uint8 and not images.any() and np.all(scales == np.inf)
    f = cta.locate(frames, 7, noise_size=1)
    assert 1 not in set(f['frame']) and {0, 2} <= set(f['frame'])          # locate finds nothing in the dark frame
    nan = np.full((1, 20, 30), np.nan, np.float32)             # no defined result; must not fault
    preprocessing.preprocess_arrays(nan, 1, 5)
    preprocessing.preprocess_arrays(nan)


def test_unsupported_halo_raises_and_the_next_call_works(engine):
    """a tile above 64 KiB of LDS: float64 frames of 2100 columns with a box of
    2001 need (1 + 2000) x (64 + 2000) x 8 bytes"""
    big = np.zeros((1, 2100, 2100), np.float64)
    with pytest.raises(_lib.EngineError):
        preprocessing.bandpass_arrays(big, 1, 2001)
    frames = _u16_batch(10, 2)
    np.testing.assert_array_equal(cta.bandpass(frames[0], 1, 9), _preprocess.bandpass(frames[0], 1, 9))


def _host_locate(frames, separation, diameter, minmass, noise_size, smoothing_size=None, threshold=None):
    """yardstick preprocess -> tests/_locate.py maxima -> tests/_characterize.py on the RAW frame
    -> minmass"""
    ndim = frames.ndim - 1
    sep = _preprocess.validate_tuple(separation, ndim)
    diameter = _preprocess.validate_tuple(diameter, ndim)
    radius = tuple(int(d // 2) for d in diameter)
    margin = tuple(int(max(d // 2, s // 2 - 1)) for d, s in zip(diameter, sep))
    isotropic = len(set(diameter)) == 1
    cols = ['z', 'y', 'x'][3 - ndim:]
    parts = []
    for t, raw in enumerate(frames):
        image = raw if noise_size is None else \
            _preprocess.preprocess(raw, noise_size, sep if smoothing_size is None else smoothing_size, threshold)[0]
        pos = np.asarray(_locate.compose(image, sep, margin=margin), dtype=np.float64).reshape(-1, ndim)
        part = pd.DataFrame(pos, columns=cols)
        for k, v in _characterize.compose(pos, raw, radius, isotropic).items():
            part[k] = v
        part['frame'] = np.int64(t)
        parts.append(part)
    out = pd.concat(parts)
    return out[out['mass'] >= minmass].reset_index(drop=True)


def _assert_tables_equal(got, expect):
    assert list(got.columns) == list(expect.columns) and len(got) == len(expect)
    for c in got:
        if c.startswith('size'):
            np.testing.assert_allclose(got[c].values, expect[c].values, rtol=1e-14, atol=0, equal_nan=True)
        else:
            np.testing.assert_array_equal(got[c].values, expect[c].values)


@pytest.mark.parametrize('geom', [((4, 70, 90), 9, (9, 9), np.uint8, 1, None), ((3, 64, 75), (7, 9), (5, 9), np.uint16, (1, 0.5), (9, 11)),
                                  ((2, 14, 40, 44), (3, 7, 7), (5, 7, 7), np.uint8, 1, None),
                                  ((3, 60, 60), 9, (9, 9), np.int16, 1, 13)], ids=['2d', '2d_aniso', '3d', 'i16'])
def test_locate_with_noise_size_equals_host_composition(geom, engine):
    shape, sep, diameter, dt, noise, smooth = geom
    rng = np.random.RandomState(zlib.crc32(repr(geom[:3]).encode()))
    frames = np.stack([_random_frame(rng, shape[1:], dt) for _ in range(shape[0])])
    everything = _host_locate(frames, sep, diameter, -np.inf, noise, smooth)
    assert len(everything) > 5
    for minmass in (-np.inf, float(np.median(everything['mass']))):
        expect = _host_locate(frames, sep, diameter, minmass, noise, smooth)
        got = cta.locate(frames, sep, diameter=diameter, minmass=minmass, noise_size=noise, smoothing_size=smooth)
        _assert_tables_equal(got, expect)
    maxima = cta.locate_maxima(frames, sep, margin=tuple(int(max(d // 2, s // 2 - 1)) for d, s in
                                                         zip(diameter, _preprocess.validate_tuple(sep, len(shape) - 1))),
                               noise_size=noise, smoothing_size=smooth)
    cols = [c for c in maxima.columns if c != 'frame']
    np.testing.assert_array_equal(maxima[cols].values, everything[cols].values)
    # without noise_size: today's path, the raw maxima
    plain = cta.locate(frames, sep, diameter=diameter, noise_size=None)
    _assert_tables_equal(plain, _host_locate(frames, sep, diameter, 0, None))
    pd.testing.assert_frame_equal(plain, cta.locate(frames, sep, diameter=diameter))


RAMP_OFFSET, RAMP_SLOPE, MINMASS = 10, 0.109, 7000


def _recovered(table, truth, n_frames):
    n = 0
    for t in range(n_frames):
        rows = table[table['frame'] == t][['y', 'x']].values
        if len(rows):
            d, _ = cKDTree(rows).query(truth[t])
            n += int((d < 2).sum())
    return n


def test_cfg2_under_an_illumination_ramp(engine):
    """The two noisy cfg-2 frames (frame 0 is tests/golden/cfg2_frame_noisy.npz) with the offset
    and ramp uint8(10 + 0.109 x) added in uint8 (10 grey levels on the left, 65 on the right: the
    headroom the brightest pixel, 189, leaves), separation = diameter = 13.  Host composition,
    frames 0 + 1 (offset, slope and minmass picked from a scan of the host composition, where the
    gap was between -4 and +3 features for every pair tried):
      maxima without preprocessing 350 + 332 = 682, with noise_size=1  589 + 575 = 1164;
      true features (of 400) with a row within 2 px at minmass 7000: raw path 122 + 127 = 249,
      with preprocessing 122 + 130 = 252.
    The gap is small by construction of the rule: as in the reference's find_link, the masses come
    from the RAW frames in both paths, so under uneven illumination one minmass cuts the dark side
    of both; what preprocessing changes is which maxima are found.  The device must give these
    figures exactly."""
    from clustertracking_amd import workloads
    frames, _, truth, _ = workloads.cfg2(n_frames=2)
    np.testing.assert_array_equal(frames[0], np.load(_preprocess.GOLDEN.replace('preprocess/preprocess_cases', 'cfg2_frame_noisy'))['frames'][0])
    ramp = (RAMP_OFFSET + RAMP_SLOPE * np.arange(frames.shape[2])).astype(np.uint8)
    assert int(frames.max()) + int(ramp.max()) <= 255
    frames = frames + ramp[None, None, :]
    assert frames.dtype == np.uint8
    truth = truth.reshape(2, -1, 2)
    figures = {}
    for label, noise in (('raw', None), ('pre', 1)):
        host_all = _host_locate(frames, 13, (13, 13), -np.inf, noise)
        host = host_all[host_all['mass'] >= MINMASS]
        dev_all = cta.locate(frames, 13, minmass=-np.inf, noise_size=noise)
        dev = cta.locate(frames, 13, minmass=MINMASS, noise_size=noise)
        figures[label] = (len(dev_all), _recovered(dev, truth, 2))
        print(label, 'maxima', len(dev_all), 'rows at minmass', len(dev), 'recovered', figures[label][1])
        assert len(dev_all) == len(host_all)
        assert len(dev) == len(host)
        assert figures[label][1] == _recovered(host, truth, 2)
    assert figures['raw'] == (682, 249) and figures['pre'] == (1164, 252)
    assert figures['pre'][1] > figures['raw'][1]
