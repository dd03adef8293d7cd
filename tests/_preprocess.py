"""The yardstick of the preprocessing: NumPy / SciPy only, no GPU.

``lowpass`` and ``preprocess`` restate the reference (preprocessing.py:13-75; pinned by
tests/golden/preprocess/preprocess_cases.npz, which the reference's own functions wrote).
``bandpass``, ``boxcar``, ``scalefactor_to_gamut`` and ``scale_to_gamut`` restate trackpy 0.3
(``trackpy/preprocessing.py``), ``gaussian_kernel`` trackpy's masks: trackpy is not installed,
so these are PARITY UNPINNED; the filters themselves are SciPy's.

``box_exact`` is the rule the device implements for integer pixels, stated without SciPy: per
axis trunc(S / size) with S the exact window sum over edge-clamped indices.
"""
import json
import os

import numpy as np
from scipy.ndimage import correlate1d, uniform_filter1d

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'preprocess', 'preprocess_cases.npz')


def validate_tuple(value, ndim):
    if not hasattr(value, '__iter__'):
        return (value,) * ndim
    if len(value) == ndim:
        return tuple(value)
    raise ValueError("List length should have same length as image dimensions.")


def gaussian_kernel(sigma, truncate=4.0):
    lw = int(truncate * sigma + 0.5)
    x = np.arange(-lw, lw + 1)
    result = np.exp(x ** 2 / (-2 * sigma ** 2))
    return result / np.sum(result)


def lowpass(image, lshort, threshold=None):
    """reference preprocessing.py:13-49"""
    lshort = validate_tuple(lshort, image.ndim)
    if threshold is None:
        if np.issubdtype(image.dtype, np.integer):
            threshold = 1
        else:
            threshold = 1 / 256.
    result = np.array(image, dtype=np.float64)
    for (axis, size) in enumerate(lshort):
        if size > 0:
            correlate1d(result, gaussian_kernel(size, 4), axis, output=result, mode='constant', cval=0.0)
    return np.where(result > threshold, result, 0)


def _gaussian_chain(image, lshort, truncate=4):
    result = np.array(image, dtype=np.float64)
    for axis, sigma in enumerate(lshort):
        if sigma > 0:
            correlate1d(result, gaussian_kernel(sigma, truncate), axis, output=result, mode='constant', cval=0.0)
    return result


def boxcar(image, size):
    """trackpy 0.3 ``boxcar``: the rolling average IN THE PIXEL TYPE, axis after axis in place."""
    size = validate_tuple(size, image.ndim)
    if not np.all([x & 1 for x in size]):
        raise ValueError("Smoothing size must be an odd integer. Round up.")
    result = image.copy()
    for axis, _size in enumerate(size):
        if _size > 1:
            uniform_filter1d(result, _size, axis, output=result, mode='nearest', cval=0)
    return result


def bandpass(image, lshort, llong, threshold=None, truncate=4):
    """trackpy 0.3 ``bandpass``"""
    lshort = validate_tuple(lshort, image.ndim)
    llong = validate_tuple(llong, image.ndim)
    if np.any([x >= y for (x, y) in zip(lshort, llong)]):
        raise ValueError("The smoothing length scale must be larger than the noise length scale.")
    if threshold is None:
        if np.issubdtype(image.dtype, np.integer):
            threshold = 1
        else:
            threshold = 1 / 255.
    background = boxcar(image, llong)
    result = _gaussian_chain(image, lshort, truncate)
    result -= background
    return np.where(result >= threshold, result, 0)


def scalefactor_to_gamut(image, dtype):
    """trackpy 0.3; the maximum widened first so that the division is one float64 division for
    float32 images too, whatever NumPy's scalar promotion rules"""
    return np.iinfo(dtype).max / np.float64(image.max())


def scale_to_gamut(image, dtype, scale_factor):
    """trackpy 0.3"""
    scaled = (scale_factor * image.clip(min=0.)).astype(dtype)
    return scaled


def preprocess(raw_image, noise_size=None, smoothing_size=None, threshold=None, bandpass=bandpass):
    """reference preprocessing.py:52-75: (image, scale_factor)"""
    if noise_size is not None:
        image = bandpass(raw_image, noise_size, smoothing_size, threshold)
        if np.issubdtype(raw_image.dtype, np.integer):
            dtype = raw_image.dtype
        else:
            dtype = np.uint8
        scale_factor = scalefactor_to_gamut(image, dtype)
        image = scale_to_gamut(image, dtype, scale_factor)
    elif np.issubdtype(raw_image.dtype, np.integer):
        scale_factor = 1.
        image = raw_image
    else:
        scale_factor = scalefactor_to_gamut(raw_image, np.uint8)
        image = scale_to_gamut(raw_image, np.uint8, scale_factor)
    return image, scale_factor


def box_exact(image, size):
    """The integer rule with exact sums (Python integers of any width would do: int64 holds
    size * 2^32): per axis trunc(S / size), S over indices clamped to the frame, truncation
    towards zero as a C cast does; the next axis works on the truncated integers."""
    assert np.issubdtype(image.dtype, np.integer)
    size = validate_tuple(size, image.ndim)
    result = image.astype(np.int64)
    for axis, s in enumerate(size):
        if s > 1:
            n = result.shape[axis]
            idx = np.clip(np.arange(n)[:, None] + np.arange(-(s // 2), s // 2 + 1)[None, :], 0, n - 1)
            total = np.take(result, idx, axis=axis).sum(axis=axis + 1)
            result = np.sign(total) * (np.abs(total) // s)
    return result.astype(image.dtype)


def boxcar_longdouble(image, size):
    """``boxcar`` of a float image with every window summed directly in ``np.longdouble``: a
    second summation order beside SciPy's running float64 sum, for the sensitivity ``p_ref``."""
    size = validate_tuple(size, image.ndim)
    result = image.copy()
    for axis, s in enumerate(size):
        if s > 1:
            n = result.shape[axis]
            idx = np.clip(np.arange(n)[:, None] + np.arange(-(s // 2), s // 2 + 1)[None, :], 0, n - 1)
            total = np.take(result.astype(np.longdouble), idx, axis=axis).sum(axis=axis + 1)
            result = (total / np.longdouble(s)).astype(image.dtype)
    return result


def bandpass_longdouble(image, lshort, llong, threshold=None):
    """``bandpass`` with ``boxcar_longdouble`` as the background."""
    lshort = validate_tuple(lshort, image.ndim)
    llong = validate_tuple(llong, image.ndim)
    if threshold is None:
        threshold = 1 if np.issubdtype(image.dtype, np.integer) else 1 / 255.
    result = _gaussian_chain(image, lshort)
    result -= boxcar_longdouble(image, llong)
    return np.where(result >= threshold, result, 0)


def fixtures():
    """[(name, image, kwargs, expected dict)] of the golden file: kwargs of ``preprocess``
    (noise_size, smoothing_size, threshold); expected: ``image``, ``scale_factor`` and, where
    noise_size is given, ``lowpass`` (the reference's lowpass with that noise size and its own
    default threshold) and ``bandpass`` (float64)."""
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(json.loads(str(z['names']))):
        kw = json.loads(str(z['args_%d' % i]))
        for k in ('noise_size', 'smoothing_size'):
            if isinstance(kw[k], list):
                kw[k] = tuple(kw[k])
        expect = {k: z['%s_%d' % (k, i)] for k in ('image', 'scale_factor', 'lowpass', 'bandpass') if '%s_%d' % (k, i) in z}
        out.append((name, z['raw_%d' % i], kw, expect))
    return out
