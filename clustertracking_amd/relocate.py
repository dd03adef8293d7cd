"""Relocation candidates of lost features: the look-again step of the reference's ``find_link``
(``FindLinker.get_relocate_candidates``, find_link.py:811-867) on the MI355X
(``ctr_relocate_device``).

When a sub-network has more sources than destinations the reference masks away what it already
found around the lost features, takes the local maxima that remain in the processed frame and
offers them to the linker.  :func:`relocate_arrays` answers a batch of such queries in one call,
:func:`relocate_candidates` one query with the reference's return.  The loop around them
(shortage per sub-network, merging, the sub-network solved with the claimed candidates) is
``find_link.find_link``.  There is no CPU fallback.
"""
import numpy as np

from . import _abi, _lib
from ._lib import EngineError
from .find import _device_frames, _size_columns, locate_arrays
from .utils import validate_tuple


def derived(diameter, separation, search_range):
    """What ``FindLinker.__init__`` derives (find_link.py:754-784): dict of ``radius``,
    ``dilation_size``, ``slice_radius``, ``bg_radius`` (tuples) and ``max_dist``."""
    ndim = len(diameter)
    radius = tuple(int(d // 2) for d in diameter)
    slice_radius = tuple(int(s + r + 1) for s, r in zip(search_range, radius))
    bg_radius = tuple(sl + r + 1 for sl, r in zip(slice_radius, radius))
    return dict(radius=radius, dilation_size=tuple(int(2 * s / np.sqrt(ndim)) for s in separation),
                slice_radius=slice_radius, bg_radius=bg_radius,
                max_dist=max(a / b for a, b in zip(bg_radius, search_range)))


def descriptor(shape, dtype, n_frames, diameter, separation, search_range, minmass=0, isotropic=None,
               scale_factor=1., max_candidates=10):
    """An ``_abi.Relocate`` with the scalars filled in (no pointers): what ``_lib.relocate_plan``
    takes."""
    ndim = len(shape)
    diameter = validate_tuple(diameter, ndim)
    separation = validate_tuple(separation, ndim)
    search_range = validate_tuple(search_range, ndim)
    if isotropic is None:
        isotropic = all(d == diameter[0] for d in diameter)
    r = _abi.Relocate()
    r.ndim = ndim
    r.frame_dtype = _abi.DTYPE_CODES[np.dtype(dtype)]
    r.n_frames = int(n_frames)
    for a in range(ndim):
        r.shape[a] = int(shape[a])
        r.radius[a] = int(diameter[a] // 2)
        r.separation[a] = float(separation[a])
        r.search_range[a] = float(search_range[a])
    r.isotropic = int(bool(isotropic))
    r.max_candidates = int(max_candidates)
    r.minmass = float(minmass)
    r.scale_factor = float(scale_factor)
    return r


def _to_device(x, np_dtype, torch_dtype, dev, what, shape_tail=None):
    """``x`` (ndarray, list or tensor on ``dev``) as a contiguous tensor of ``torch_dtype``."""
    import torch
    if isinstance(x, torch.Tensor):
        if x.device != dev:
            raise ValueError("%s must be on %s (it is on %s)" % (what, dev, x.device))
        t = x.to(torch_dtype).contiguous()
    else:
        arr = np.ascontiguousarray(x, dtype=np_dtype)
        if shape_tail is not None:
            arr = arr.reshape((-1,) + shape_tail)
        t = torch.from_numpy(arr).to(dev)
    if shape_tail is not None and (t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != shape_tail):
        raise ValueError("%s must be [N, %s]" % (what, ', '.join(str(s) for s in shape_tail)))
    return t


def relocate_arrays(frames, threshold, known, known_offset, sources, source_offset, query_frame,
                    diameter, separation, search_range, minmass=0, isotropic=None, scale_factor=1.,
                    max_candidates=10, device=0, dtype=None, _on_device=False):
    """Relocation candidates of a batch of independent queries on the MI355X.

    frames: [T, (z,) y, x], ndarray or tensor on cuda:``device`` (as for ``locate_arrays``);
    threshold: [T] float64, what ``locate_arrays`` returns per frame; known: [M, ndim] positions of
    the features already found, sorted by frame, with known_offset [T + 1] -- the tensors of a
    preceding ``locate_arrays(..., _on_device=True)`` go in as they are (int32 positions are
    widened); sources: [S, ndim] float64 positions of the lost features, source_offset [Q + 1],
    query_frame [Q]: query q looks in frame ``query_frame[q]`` around ``sources[source_offset[q]:
    source_offset[q + 1]]``.  diameter, separation, search_range, minmass: as ``FindLinker`` takes
    them; isotropic defaults to that of the diameter.

    Returns NumPy arrays ``(n_found [Q] int32, pos [Q, K, ndim] int32, mass [Q, K], signal [Q, K],
    size [Q, K] or [Q, K, ndim], status [Q] int32)`` with K = ``max_candidates``: rows
    ``[0, min(n_found, K))`` of a query by mass descending (equal masses in C order of position),
    -1 / NaN behind them.  ``status`` is 0, ``_abi.RELOCATE_CAPACITY`` (more than 30 sources, more
    than 256 raw maxima or more than 512 background features in the box) or
    ``_abi.RELOCATE_BAD_FRAME``; with a non-zero status the rows are not a result.  Frames of any
    size are taken: a query whose box is too wide for the LDS tile only runs slower."""
    if not hasattr(frames, 'shape'):
        frames = np.asarray(frames)
    ndim = len(frames.shape) - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]")
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    t, pix = _device_frames(frames, device, dtype)
    dev = t.device
    n_frames = int(t.shape[0])
    r = descriptor(tuple(t.shape[1:]), pix, n_frames, diameter, separation, search_range, minmass, isotropic,
                   scale_factor, max_candidates)
    iso = bool(r.isotropic)
    with torch.cuda.device(dev):
        thr_t = _to_device(threshold, np.float64, torch.float64, dev, 'threshold')
        known_t = _to_device(known, np.float64, torch.float64, dev, 'known', (ndim,))
        koff_t = _to_device(known_offset, np.int64, torch.int64, dev, 'known_offset')
        src_t = _to_device(sources, np.float64, torch.float64, dev, 'sources', (ndim,))
        soff_t = _to_device(source_offset, np.int64, torch.int64, dev, 'source_offset')
        qf_t = _to_device(query_frame, np.int64, torch.int64, dev, 'query_frame')
        n_q = int(qf_t.numel())
        if thr_t.numel() != n_frames or koff_t.numel() != n_frames + 1:
            raise ValueError("threshold must have n_frames entries and known_offset n_frames + 1")
        if soff_t.numel() != n_q + 1:
            raise ValueError("source_offset must have one entry more than query_frame")
        K = int(max_candidates)
        n_found = torch.zeros(n_q, dtype=torch.int32, device=dev)
        status = torch.zeros(n_q, dtype=torch.int32, device=dev)
        pos = torch.empty((n_q, max(K, 0), ndim), dtype=torch.int32, device=dev)
        mass = torch.empty((n_q, max(K, 0)), dtype=torch.float64, device=dev)
        signal = torch.empty_like(mass)
        size = torch.empty((n_q, max(K, 0)) if iso else (n_q, max(K, 0), ndim), dtype=torch.float64, device=dev)
        r.frames, r.threshold = t.data_ptr(), thr_t.data_ptr()
        r.n_known, r.known_pos, r.known_offset = int(known_t.shape[0]), known_t.data_ptr(), koff_t.data_ptr()
        r.n_queries, r.query_frame, r.source_offset = n_q, qf_t.data_ptr(), soff_t.data_ptr()
        r.source_pos = src_t.data_ptr()
        r.n_found, r.cand_pos, r.status = n_found.data_ptr(), pos.data_ptr(), status.data_ptr()
        r.mass, r.signal, r.size = mass.data_ptr(), signal.data_ptr(), size.data_ptr()
        eng.on_current_stream(eng.relocate_device, r, dev=dev)
        if _on_device:      # the caller synchronises; the inputs must outlive the kernel
            return (n_found, pos, mass, signal, size, status), (t, thr_t, known_t, koff_t, src_t, soff_t, qf_t)
        torch.cuda.synchronize(dev)   # the inputs uploaded here live until the kernel has read them
    return tuple(x.cpu().numpy() for x in (n_found, pos, mass, signal, size, status))


def relocate_candidates(image, sources, known, diameter, separation, search_range, minmass=0,
                        percentile=64, scale_factor=1., device=0):
    """Reference ``FindLinker.get_relocate_candidates`` for one frame on the MI355X:
    ``(coords [n, ndim] int64, dict(mass=, signal=, size= or size_z / size_y / size_x))`` of the
    candidates around ``sources`` [S, ndim] that are not among ``known`` [M, ndim] (or None), by
    mass descending, or ``(None, None)`` when there is none.  The threshold is the ``percentile``
    of the frame's non-zero pixels, taken by the percentile pass of ``locate_arrays``.  Every
    candidate is returned (the reference's caller takes as many as the sub-network is short of).
    A query beyond the engine's per-query limits (``_abi.RELOCATE_CAPACITY``) raises
    ``EngineError``."""
    image = np.asarray(image)
    ndim = image.ndim
    diameter = validate_tuple(diameter, ndim)
    separation = validate_tuple(separation, ndim)
    search_range = validate_tuple(search_range, ndim)
    isotropic = all(d == diameter[0] for d in diameter)
    sources = np.asarray(sources, dtype=np.float64).reshape(-1, ndim)
    known = np.empty((0, ndim)) if known is None else np.asarray(known, dtype=np.float64).reshape(-1, ndim)
    _, _, thr = locate_arrays(image[None], separation, percentile, device=device)
    K = 16
    while True:
        n_found, pos, mass, signal, size, status = relocate_arrays(
            image[None], thr, known, [0, len(known)], sources, [0, len(sources)], [0], diameter, separation,
            search_range, minmass, isotropic, scale_factor, K, device)
        if status[0] != _abi.RELOCATE_OK:
            raise EngineError("relocate_candidates: the query is beyond the engine's per-query limits "
                              "(status %d: more than %d sources, %d raw maxima or %d background features)"
                              % (status[0], _abi.LINK_MAX_SOURCES, _abi.RELOCATE_MAX_MAXIMA,
                                 _abi.RELOCATE_MAX_BACKGROUND))
        if n_found[0] <= K:
            break
        K = int(n_found[0])
    n = int(n_found[0])
    if n == 0:
        return None, None
    extra = dict(mass=mass[0, :n].copy(), signal=signal[0, :n].copy())
    if isotropic:
        extra['size'] = size[0, :n].copy()
    else:
        for a, key in enumerate(_size_columns(ndim, False)):
            extra[key] = size[0, :n, a].copy()
    return pos[0, :n].astype(np.int64), extra

