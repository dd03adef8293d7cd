"""Preprocessing of raw frames on the MI355X: what the reference's ``find_link`` runs in front
of the maxima search (find_link.py:468,957-959; preprocessing.py:52-75).

``lowpass`` follows reference preprocessing.py:13-49, ``preprocess`` preprocessing.py:52-75;
``bandpass``, ``scalefactor_to_gamut`` and ``scale_to_gamut`` are trackpy's (restated from its
published 0.3 source: PARITY UNPINNED), as is ``gaussian_kernel``.  The pixels are
filtered by ``ctr_preprocess_device`` (csrc/preprocess_kernels.h); only the Gaussian taps are
computed here, with NumPy, so that they are the reference's to the last bit.  Integer frames come
out equal to NumPy / SciPy's result bit for bit, float frames to rounding.

``lowpass``, ``bandpass`` and ``preprocess`` take one image, as the reference's do; the
``*_arrays`` functions take a block of frames ``[T, (z,) y, x]``.  There is no CPU fallback.
"""
import numpy as np

from . import _abi, _lib
from .utils import validate_tuple


def gaussian_kernel(sigma, truncate=4.0):
    """1D discretised Gaussian, ``trackpy.masks.gaussian_kernel`` (restated; parity unpinned)."""
    lw = int(truncate * sigma + 0.5)
    x = np.arange(-lw, lw + 1)
    result = np.exp(x ** 2 / (-2 * sigma ** 2))
    return result / np.sum(result)


def _taps(lshort, ndim):
    """Taps per axis; an axis that is not filtered (``lshort <= 0``) gets the single tap 1."""
    lshort = validate_tuple(lshort, ndim)
    taps = []
    for size in lshort:
        if not np.isfinite(size):
            raise ValueError("the noise size must be finite")
        taps.append(np.ascontiguousarray(gaussian_kernel(size, 4), dtype=np.float64) if size > 0 else np.ones(1))
    return lshort, taps


def _box(lshort, llong, ndim):
    """trackpy's argument checks of ``bandpass`` / ``boxcar``; the box size per axis."""
    llong = validate_tuple(llong, ndim)
    if any(x is None for x in llong):
        raise ValueError("bandpass needs a smoothing size")
    if np.any([x >= y for (x, y) in zip(lshort, llong)]):
        raise ValueError("The smoothing length scale must be larger than the noise length scale.")
    if not all(int(x) == x and int(x) & 1 for x in llong):
        raise ValueError("Smoothing size must be an odd integer. Round up.")
    return [max(int(x), 1) for x in llong]     # `_size > 1`: a box of 1 or less is skipped


def check_sizes(noise_size, smoothing_size, ndim):
    """The ``ValueError`` s of ``bandpass(image, noise_size, smoothing_size)``, without an image."""
    lshort, _ = _taps(noise_size, ndim)
    _box(lshort, smoothing_size, ndim)


_DEVICE_TAPS = {}


def _device_taps(torch, lshort, taps, dev):
    """The taps as tensors on the device, uploaded once per (sizes, device) and kept: a call
    queues no upload and needs no synchronisation to keep them alive."""
    key = (tuple(float(x) for x in lshort), str(dev))
    held = _DEVICE_TAPS.get(key)
    if held is None:
        if len(_DEVICE_TAPS) >= 64:
            _DEVICE_TAPS.clear()
        held = _DEVICE_TAPS[key] = [torch.from_numpy(w).to(dev) for w in taps]
        torch.cuda.synchronize(dev)
    return held


def _is_integer(pix):
    return np.issubdtype(pix, np.integer)


def _out_tensor(torch, shape, np_dtype, dev):
    """An output tensor of a NumPy type (uint16 travels as int16, as the frames do)."""
    kinds = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16, np.dtype(np.int16): torch.int16,
             np.dtype(np.int32): torch.int32, np.dtype(np.float64): torch.float64}
    return torch.empty(shape, dtype=kinds[np.dtype(np_dtype)], device=dev)


def _to_numpy(t, np_dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if np.dtype(np_dtype) == np.uint16 else a


def _run(frames, mode, lshort, llong, threshold, device, dtype, strategy=_abi.PRE_AUTO):
    """One ``ctr_preprocess_device`` call on a block: (out tensor, its NumPy type, scale_factor
    tensor or None, frames tensor, pixel type).  The arguments are checked before any GPU call."""
    ndim = len(frames.shape) - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]")
    taps = box = None
    if mode != _abi.PRE_SCALE:
        lshort, taps = _taps(lshort, ndim)
        if mode != _abi.PRE_LOWPASS:
            box = _box(lshort, llong, ndim)
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    from .find import _device_frames
    t, pix = _device_frames(frames, device, dtype)
    pix = np.dtype(pix)
    if threshold is None:       # preprocessing.py:35-39 (lowpass), trackpy bandpass
        threshold = 1 if _is_integer(pix) else (1 / 256. if mode == _abi.PRE_LOWPASS else 1 / 255.)
    scaled = mode in (_abi.PRE_PREPROCESS, _abi.PRE_SCALE)
    out_type = np.dtype(np.float64) if not scaled else (pix if _is_integer(pix) else np.dtype(np.uint8))
    dev = t.device
    n_frames = int(t.shape[0])
    d = _abi.Preprocess()
    d.ndim = ndim
    d.frame_dtype = _abi.DTYPE_CODES[pix]
    d.n_frames = n_frames
    d.mode = mode
    d.strategy = strategy
    d.threshold = float(threshold)
    with torch.cuda.device(dev):
        held = _device_taps(torch, lshort, taps, dev) if taps is not None else None
        for a in range(ndim):
            d.shape[a] = int(t.shape[1 + a])
            if held is not None:
                d.n_taps[a] = int(held[a].numel())
                d.taps[a] = held[a].data_ptr()
            d.box[a] = box[a] if box is not None else 1
        out = _out_tensor(torch, tuple(t.shape), out_type, dev)
        scale = torch.empty(max(n_frames, 1), dtype=torch.float64, device=dev) if scaled else None
        d.frames = t.data_ptr()
        d.out = out.data_ptr()
        d.scale_factor = scale.data_ptr() if scaled else None
        eng.on_current_stream(eng.preprocess_device, d, dev=dev)
        # no synchronisation, as for ctr_locate_maxima_device: the call is ordered on the caller's
        # stream, where whatever reads `out` (a copy to the host, the maxima search) is queued too
    return out, out_type, (scale[:n_frames] if scaled else None), t, pix


def lowpass_arrays(frames, lshort, threshold=None, device=0, dtype=None):
    """:func:`lowpass` of every frame of a block ``[T, (z,) y, x]``: float64 ndarray."""
    out, _, _, _, _ = _run(frames, _abi.PRE_LOWPASS, lshort, None, threshold, device, dtype)
    return out.cpu().numpy()


def bandpass_arrays(frames, lshort, llong, threshold=None, device=0, dtype=None):
    """:func:`bandpass` of every frame of a block ``[T, (z,) y, x]``: float64 ndarray."""
    out, _, _, _, _ = _run(frames, _abi.PRE_BANDPASS, lshort, llong, threshold, device, dtype)
    return out.cpu().numpy()


def preprocess_arrays(frames, noise_size=None, smoothing_size=None, threshold=None, device=0, dtype=None,
                      _on_device=False, _strategy=_abi.PRE_AUTO):
    """:func:`preprocess` of every frame of a block ``[T, (z,) y, x]`` (ndarray, or a torch tensor
    on cuda:``device`` as :func:`find.locate_arrays` takes it): (integer frames, scale_factor [T]).
    Without ``noise_size`` integer frames come back as they are with scale factors of 1.
    (``_on_device``, internal: the two as torch tensors on the device followed by the frames'
    NumPy type -- what :func:`find.locate_arrays` goes on with.)"""
    if noise_size is not None:
        mode = _abi.PRE_PREPROCESS
    else:
        if not hasattr(frames, 'shape'):
            frames = np.asarray(frames)
        _lib.default_engine(device)     # EngineError without a library or a GPU
        from .find import _device_frames
        t, pix = _device_frames(frames, device, dtype)
        if _is_integer(pix):            # preprocessing.py:62-65: nothing to do
            if _on_device:
                import torch
                return t, torch.ones(int(t.shape[0]), dtype=torch.float64, device=t.device), np.dtype(pix)
            return _to_numpy(t, pix), np.ones(int(t.shape[0]))
        frames, dtype, mode = t, pix, _abi.PRE_SCALE
    if not hasattr(frames, 'shape'):
        frames = np.asarray(frames)
    out, out_type, scale, _, _ = _run(frames, mode, noise_size, smoothing_size, threshold, device, dtype, _strategy)
    if _on_device:
        return out, scale, out_type
    return _to_numpy(out, out_type), scale.cpu().numpy()


def _one(image):
    if not hasattr(image, 'shape'):
        image = np.asarray(image)
    return image[None]


def lowpass(image, lshort, threshold=None, device=0, dtype=None):
    """Gaussian lowpass of one image (reference preprocessing.py:13-49): float64 copy, per axis
    with ``lshort[a] > 0`` SciPy's ``correlate1d`` with ``gaussian_kernel(lshort[a], 4)`` and zeros
    beyond the image, then ``where(result > threshold, result, 0)``.  ``threshold`` defaults to 1
    for integer images, 1/256 for float images."""
    return lowpass_arrays(_one(image), lshort, threshold, device, dtype)[0]


def bandpass(image, lshort, llong, threshold=None, device=0, dtype=None):
    """trackpy's ``bandpass`` of one image: the Gaussian lowpass minus a rolling average of size
    ``llong`` (odd, larger than ``lshort``; taken in the pixel type with the edge pixel repeated),
    then ``where(result >= threshold, result, 0)`` as float64.  ``threshold`` defaults to 1 for
    integer images, 1/255 for float images."""
    return bandpass_arrays(_one(image), lshort, llong, threshold, device, dtype)[0]


def preprocess(raw_image, noise_size=None, smoothing_size=None, threshold=None, device=0, dtype=None):
    """Reference ``preprocess`` (preprocessing.py:52-75) of one image: (integer image,
    scale_factor).  With ``noise_size``: :func:`bandpass`, rescaled to fill the raw integer type
    (uint8 for float images).  Without: an integer image as it is (factor 1), a float image
    rescaled into uint8.  The reference keeps the factor in ``Frame.metadata['scale_factor']``."""
    image, scale = preprocess_arrays(_one(raw_image), noise_size, smoothing_size, threshold, device, dtype)
    return image[0], float(scale[0])
