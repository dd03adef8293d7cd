"""Host-side cluster labelling: which features are fitted together.

Behavioural mirror of reference ``clustertracking/find.py:12-163``
(``Clusters``, ``_find``, ``find_iter``, ``find_clusters``): features closer
than ``separation`` (per-axis scaled Euclidean distance < 1) belong to one
cluster; clusters never span frames; ids carry a running per-frame offset.

Feature location follows reference ``find.py:166-277`` (``where_close``,
``drop_close``, ``percentile_threshold``, ``grey_dilation``): the three helpers
run on the host, the local-maximum search itself on the MI355X
(``ctr_locate_maxima_device``) for one frame (``grey_dilation``)
or a block of frames (``locate_maxima``).  There is no CPU fallback.

Characterisation follows reference ``find_link.characterize`` (find_link.py:44-79) and the
``minmass`` filter of ``find_link`` (find_link.py:927-971): mass, signal and size of every located
maximum on the MI355X (``ctr_characterize_device``) -- ``characterize`` for one
frame, ``characterize_arrays`` for a block, ``locate`` for the chain locate -> characterize ->
``mass >= minmass`` with the positions staying on the device in between.

The labels themselves follow the reference's merge rule (when a pair (a, b) is
joined, b's whole cluster takes a's current label; pairs are visited in the
iteration order of the set returned by ``cKDTree.query_pairs``), so that ids
are equal to the reference's and not merely partition-equivalent.
"""
import numpy as np
import pandas as pd
from scipy.spatial import cKDTree

from . import _abi, _lib
from .utils import guess_pos_columns, validate_tuple


def label_points(pos, separation):
    """Cluster labels and sizes for one frame.

    pos : [n, ndim] array; separation : per-axis tuple.
    Returns (ids [n] int, sizes [n] int).  (reference find.py:72-93)"""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    label = list(range(n))
    if n > 1:
        pairs = cKDTree(pos / separation).query_pairs(1)
        members = {}
        for a, b in pairs:
            la, lb = label[a], label[b]
            if la == lb:
                continue
            grp_a = members.setdefault(la, [la])
            grp_b = members.pop(lb, [lb])
            for k in grp_b:
                label[k] = la
            grp_a.extend(grp_b)
    label = np.asarray(label, dtype=np.int64)
    if n == 0:
        return label, label.copy()
    sizes = np.bincount(label, minlength=n)[label]
    return label, sizes


def find_iter(f, separation, pos_columns=None, t_column='frame'):
    """Per-frame generator of ``(frame_no, DataFrame)`` with ``cluster`` and
    ``cluster_size`` columns added (reference find.py:96-129)."""
    if pos_columns is None:
        pos_columns = guess_pos_columns(f)
    next_id = 0
    for frame_no, f_frame in f.groupby(t_column):
        ids, sizes = label_points(f_frame[pos_columns].values, separation)
        result = f_frame.copy()
        result['cluster'] = ids + next_id
        result['cluster_size'] = sizes
        next_id = result['cluster'].max() + 1
        yield frame_no, result


def label_frames(pos, frames, separation):
    """Cluster ids and sizes for a whole table at once (NumPy only).

    pos [N, ndim], frames [N]; returns (order, ids, sizes) where ``order`` is
    the stable frame-sorted row order of find_clusters' output and ids/sizes
    are aligned with it.  Same labels as running :func:`label_points` frame by
    frame with the reference's running id offset (find.py:120-128)."""
    pos = np.asarray(pos, dtype=np.float64)
    frames = np.asarray(frames)
    order = np.argsort(frames, kind='stable')
    fs = frames[order]
    n = len(order)
    ids = np.empty(n, dtype=np.int64)
    sizes = np.empty(n, dtype=np.int64)
    if n == 0:
        return order, ids, sizes
    starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]])
    stops = np.r_[starts[1:], n]
    scaled = pos[order] / separation
    next_id = 0
    for a, b in zip(starts, stops):
        lab, siz = label_points(scaled[a:b], 1.)
        ids[a:b] = lab + next_id
        sizes[a:b] = siz
        next_id = ids[a:b].max() + 1
    return order, ids, sizes


def label_frames_device(pos, frames, separation, device=0):
    """Same contract as :func:`label_frames`, computed by the HIP engine
    (``ctr_find_clusters``).  The partition equals the reference's; the ids are
    canonical (smallest frame-sorted row index of the cluster) instead of the
    reference's set-order-dependent ones."""
    from . import _lib
    pos = np.asarray(pos, dtype=np.float64)
    frames = np.asarray(frames)
    order = np.argsort(frames, kind='stable')
    fs = frames[order]
    n = len(order)
    if n == 0:
        return order, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]])
    offsets = np.r_[starts, n].astype(np.int32)
    labels, sizes = _lib.default_engine(device).find_clusters(pos[order], offsets, separation)
    return order, labels.astype(np.int64), sizes.astype(np.int64)


def find_clusters(f, separation, pos_columns=None, t_column='frame', labels='reference',
                  device=0):
    """Copy of ``f`` (rows grouped by frame) with ``cluster`` and
    ``cluster_size`` columns (reference find.py:132-163).  One pass over NumPy
    arrays instead of a DataFrame copy per frame; same rows, order and labels.

    ``labels='device'`` computes the same partition on the MI355X
    (``ctr_find_clusters``) with canonical ids (smallest row of the cluster)."""
    if pos_columns is None:
        pos_columns = guess_pos_columns(f)
    separation = np.array(validate_tuple(separation, len(pos_columns)),
                          dtype=np.float64)
    if t_column in f:
        frames = f[t_column].values
    else:
        frames = np.zeros(len(f), dtype=np.int64)
    if labels == 'reference':
        order, ids, sizes = label_frames(f[pos_columns].values, frames, separation)
    elif labels == 'device':
        order, ids, sizes = label_frames_device(f[pos_columns].values, frames, separation, device)
    else:
        raise ValueError("labels must be 'reference' or 'device'")
    result = f.iloc[order].copy()
    if t_column not in f:
        result[t_column] = 0   # the reference's output carries the temporary column (find.py:149-157)
    result['cluster'] = ids
    result['cluster_size'] = sizes
    return result


# ---- feature location (reference find.py:166-277) ------------------------------------------

def where_close(pos, separation, intensity=None):
    """Sorted indices of the features that lose a pair closer than ``separation`` (scaled
    distance <= 1 - 1e-7, as ``cKDTree.query_pairs``): the dimmer one of the pair, on equal
    intensity the one with the smaller sum of ``pos / separation``, and on a tie of both the
    one listed first.  ``[]`` when there is none (reference find.py:166-198)."""
    pos = np.asarray(pos)
    if len(pos) == 0:
        return []
    separation = validate_tuple(separation, pos.shape[1])
    if any(s == 0 for s in separation):
        return []
    scaled = pos / separation
    pairs = cKDTree(scaled, 30).query_pairs(1 - 1e-7, output_type='ndarray')
    if len(pairs) == 0:
        return []
    first, second = pairs[:, 0], pairs[:, 1]
    by_sum = np.where(np.sum(scaled[first], 1) > np.sum(scaled[second], 1), second, first)
    if intensity is None:
        lose = by_sum
    else:
        intensity = np.asarray(intensity)
        a, b = intensity[first], intensity[second]
        lose = np.where(a > b, second, first)
        tie = a == b
        lose[tie] = by_sum[tie]
    return np.unique(lose)


def drop_close(pos, separation, intensity=None):
    """``pos`` without the rows :func:`where_close` names (reference find.py:201-206)."""
    return np.delete(pos, where_close(pos, separation, intensity), axis=0)


def percentile_threshold(image, percentile):
    """``np.percentile`` of the non-zero pixels; NaN when there are none
    (reference find.py:209-216)."""
    pixels = image[np.nonzero(image)]
    if pixels.size == 0:
        return np.nan
    return np.percentile(pixels, percentile)


_TORCH_DTYPES = None


def _device_frames(frames, device, dtype):
    """(contiguous torch tensor on the device, NumPy pixel type) of a block of frames."""
    import torch
    global _TORCH_DTYPES
    if _TORCH_DTYPES is None:
        _TORCH_DTYPES = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32,
                         torch.float32: np.float32, torch.float64: np.float64}
    dev = torch.device('cuda', device)
    if isinstance(frames, torch.Tensor):
        if frames.device != dev:
            raise ValueError("frames must be on cuda:%d (they are on %s)" % (device, frames.device))
        if frames.dtype not in _TORCH_DTYPES:
            raise ValueError("pixel type %s is not supported" % frames.dtype)
        pix = np.dtype(_TORCH_DTYPES[frames.dtype])
        if dtype is not None and np.dtype(dtype) != pix:
            if not (pix == np.int16 and np.dtype(dtype) == np.uint16):
                raise ValueError("dtype %s does not describe a %s tensor" % (np.dtype(dtype), frames.dtype))
            pix = np.dtype(np.uint16)   # uint16 frames travel as int16 (device.draw_frames)
        return frames.contiguous(), pix
    arr = np.ascontiguousarray(frames)
    if dtype is not None and np.dtype(dtype) != arr.dtype:
        raise ValueError("dtype %s does not describe a %s array" % (np.dtype(dtype), arr.dtype))
    if arr.dtype not in _abi.DTYPE_CODES:
        raise ValueError("pixel type %s is not supported" % arr.dtype)
    host = torch.from_numpy(arr.view(np.int16) if arr.dtype == np.uint16 else arr)
    with torch.cuda.device(dev):
        return host.to(dev), arr.dtype


def locate_arrays(frames, separation, percentile=64, margin=None, precise=True, device=0,
                  dtype=None, capacity=None, _on_device=False, noise_size=None, smoothing_size=None,
                  threshold=None):
    """The device pass behind :func:`locate_maxima`: (positions int32 [N, ndim] in frame order,
    frame_offset int64 [T + 1], per-frame threshold float64 [T]) as NumPy arrays.
    ``capacity``: rows to reserve at first; a larger buffer is taken when the frames hold more.
    ``noise_size``, ``smoothing_size``, ``threshold``: see :func:`locate_maxima`.
    ``EngineError``: a separation whose box needs an LDS tile over 64 KiB.
    (``_on_device``, internal: the three as torch tensors on the device, preceded by the RAW
    frames' tensor and pixel type -- what :func:`locate` hands to :func:`characterize_arrays`.)"""
    if not hasattr(frames, 'shape'):
        frames = np.asarray(frames)
    ndim = len(frames.shape) - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]")
    separation = validate_tuple(separation, ndim)
    if noise_size is not None:
        from . import preprocessing
        if smoothing_size is None:
            smoothing_size = separation     # find_link.py:921
        preprocessing.check_sizes(noise_size, smoothing_size, ndim)
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    raw_t, raw_pix = _device_frames(frames, device, dtype)
    if noise_size is None:
        t, pix = raw_t, raw_pix
    else:       # find_link.py:957-959: the maxima are those of the preprocessed frames
        t, _, pix = preprocessing.preprocess_arrays(raw_t, noise_size, smoothing_size, threshold, device, raw_pix,
                                                    _on_device=True)
    if margin is None:
        margin = tuple(int(s / 2) for s in separation)
    margin = validate_tuple(margin, ndim)
    if any(int(m) != m for m in margin):
        raise ValueError("margin must be integer")
    n_frames = int(t.shape[0])
    if capacity is None:
        capacity = max(1024, 512 * n_frames)
    dev = t.device
    loc = _abi.Locate()
    loc.ndim = ndim
    loc.frame_dtype = _abi.DTYPE_CODES[np.dtype(pix)]
    loc.n_frames = n_frames
    for a in range(ndim):
        loc.shape[a] = int(t.shape[1 + a])
        loc.separation[a] = float(separation[a])
        loc.margin[a] = int(margin[a])
    loc.percentile = float(percentile)
    loc.precise = int(bool(precise))
    loc.frames = t.data_ptr()
    with torch.cuda.device(dev):
        offset = torch.empty(n_frames + 1, dtype=torch.int64, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        thr = torch.empty(max(n_frames, 1), dtype=torch.float64, device=dev)
        loc.frame_offset, loc.total, loc.threshold = offset.data_ptr(), total.data_ptr(), thr.data_ptr()
        while True:
            pos = torch.empty((max(int(capacity), 1), ndim), dtype=torch.int32, device=dev)
            loc.capacity = int(capacity)
            loc.pos_out = pos.data_ptr()
            eng.on_current_stream(eng.locate_maxima_device, loc, dev=dev)
            torch.cuda.synchronize(dev)
            n = int(total.item())
            if n <= capacity:
                break
            capacity = n        # more maxima than rows: run again with room for all of them
        if _on_device:
            return raw_t, raw_pix, pos[:n], offset, thr[:n_frames]
        return (pos[:n].cpu().numpy(), offset.cpu().numpy(), thr[:n_frames].cpu().numpy())


def locate_maxima(frames, separation, percentile=64, margin=None, precise=True, device=0,
                  dtype=None, noise_size=None, smoothing_size=None, threshold=None):
    """Local maxima of every frame of a block by the rule of reference ``grey_dilation``,
    on the MI355X.

    frames: ndarray [T, (z,) y, x] or a torch tensor already on cuda:``device`` (for example
    ``device.draw_frames`` output); ``dtype=np.uint16`` reads an int16 tensor as unsigned.
    Returns a DataFrame with the position columns ((z,) y, x; float64) and ``frame``, rows in
    frame order and, within a frame, in the order :func:`grey_dilation` returns them.

    ``noise_size`` given: every frame first goes through ``preprocessing.preprocess`` on the
    device (bandpass with ``noise_size`` and ``smoothing_size``, default ``separation``, then
    rescaled into the integer type) as in the reference's ``find_link`` (find_link.py:957-959),
    and the maxima are those of the preprocessed frames.  ``noise_size=None`` (the default here)
    takes the frames as they are; the reference's default is ``noise_size=1``.
    Raises ``EngineError`` for a separation whose box needs an LDS tile over 64 KiB (2D: a box
    above 200 pixels for 1-byte, 128 for 2-byte, 79 for 4-byte, 46 for float64 pixels)."""
    pos, offset, _ = locate_arrays(frames, separation, percentile, margin, precise, device, dtype,
                                   noise_size=noise_size, smoothing_size=smoothing_size, threshold=threshold)
    ndim = pos.shape[1]
    cols = ['z', 'y', 'x'][3 - ndim:]
    result = pd.DataFrame(pos.astype(np.float64), columns=cols)
    result['frame'] = np.repeat(np.arange(len(offset) - 1, dtype=np.int64), np.diff(offset))
    return result


def grey_dilation(image, separation, percentile=64, margin=None, precise=True, device=0):
    """Positions [n, ndim] (int64) of the local maxima of one frame brighter than the
    ``percentile`` of its non-zero pixels, as reference ``find.grey_dilation``
    (find.py:219-277) returns them; ``np.empty((0, ndim))`` when there is none.  Runs on the
    MI355X (``locate_maxima`` with one frame)."""
    image = np.asarray(image)
    pos, _, _ = locate_arrays(image[None], separation, percentile, margin, precise, device)
    if len(pos) == 0:
        return np.empty((0, image.ndim))
    return pos.astype(np.int64)


# ---- characterisation (reference find_link.py:44-79, 927-971) -------------------------------

def _size_columns(ndim, isotropic):
    return ['size'] if isotropic else ['size_z', 'size_y', 'size_x'][3 - ndim:]


def _characterize_device(frames, pos, frame_offset, radius, isotropic, scale_factor, device, dtype):
    """:func:`characterize_arrays` with the results left on the device (torch tensors)."""
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    t, pix = _device_frames(frames, device, dtype)
    ndim = t.dim() - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]")
    radius = validate_tuple(radius, ndim)
    if any(int(r) != r for r in radius):
        raise ValueError("radius must be integer")
    dev = t.device
    n_frames = int(t.shape[0])
    with torch.cuda.device(dev):
        if isinstance(pos, torch.Tensor):
            if pos.device != dev:
                raise ValueError("pos must be on cuda:%d (it is on %s)" % (device, pos.device))
            if pos.dtype not in (torch.int32, torch.float64):
                raise ValueError("a position tensor is int32 or float64, not %s" % pos.dtype)
            pos_t = pos.contiguous()
        else:
            pos = np.asarray(pos)
            pos = np.ascontiguousarray(pos, dtype=np.int32 if pos.dtype == np.int32 else np.float64)
            pos_t = torch.from_numpy(pos.reshape(-1, ndim) if pos.size == 0 else pos).to(dev)
        if pos_t.dim() != 2 or pos_t.shape[1] != ndim:
            raise ValueError("pos must be [N, %d]" % ndim)
        n = int(pos_t.shape[0])
        if isinstance(frame_offset, torch.Tensor):
            if frame_offset.device != dev or frame_offset.dtype != torch.int64:
                raise ValueError("a frame_offset tensor is int64 on cuda:%d" % device)
            off_t = frame_offset.contiguous()
            if off_t.numel() != n_frames + 1:
                raise ValueError("frame_offset must have n_frames + 1 entries")
        else:
            off = np.ascontiguousarray(frame_offset, dtype=np.int64)
            if off.shape != (n_frames + 1,) or off[0] != 0 or off[-1] != n or np.any(np.diff(off) < 0):
                raise ValueError("frame_offset must be [n_frames + 1], rising from 0 to the number of features")
            off_t = torch.from_numpy(off).to(dev)
        mass = torch.empty(n, dtype=torch.float64, device=dev)
        signal = torch.empty(n, dtype=torch.float64, device=dev)
        size = torch.empty((n, 1 if isotropic else ndim), dtype=torch.float64, device=dev)
        if n == 0:      # nothing to launch (and an empty tensor has no address to pass)
            if not (float(scale_factor) != 0.):
                raise ValueError("scale_factor must be a non-zero number")
            return mass, signal, size
        ch = _abi.Characterize()
        ch.ndim = ndim
        ch.frame_dtype = _abi.DTYPE_CODES[np.dtype(pix)]
        ch.n_frames = n_frames
        for a in range(ndim):
            ch.shape[a] = int(t.shape[1 + a])
            ch.radius[a] = int(radius[a])
        ch.isotropic = int(bool(isotropic))
        ch.scale_factor = float(scale_factor)
        ch.frames = t.data_ptr()
        ch.n_features = n
        ch.frame_offset = off_t.data_ptr()
        if pos_t.dtype == torch.int32:
            ch.pos_i32 = pos_t.data_ptr()
        else:
            ch.pos = pos_t.data_ptr()
        ch.mass, ch.signal, ch.size = mass.data_ptr(), signal.data_ptr(), size.data_ptr()
        eng.on_current_stream(eng.characterize_device, ch, dev=dev)
        torch.cuda.synchronize(dev)   # the inputs uploaded here live until the kernel has read them
    return mass, signal, size


def characterize_arrays(frames, pos, frame_offset, radius, isotropic=True, scale_factor=1.,
                        device=0, dtype=None):
    """Mass, signal and size of the features of a block of frames on the MI355X, by the rule of
    reference ``find_link.characterize`` (``ctr_characterize_device``).

    frames: ndarray [T, (z,) y, x] or a torch tensor on cuda:``device`` (as for
    :func:`locate_arrays`); pos: [N, ndim] centres sorted by frame, float64 or int32, ndarray or
    tensor on the device; frame_offset: [T + 1] int64, rows ``[off[t], off[t + 1])`` belong to
    frame t -- the device tensors of a preceding locate go in as they are.
    Returns NumPy float64 arrays (mass [N], signal [N], size [N] or [N, ndim])."""
    mass, signal, size = _characterize_device(frames, pos, frame_offset, radius, isotropic, scale_factor,
                                              device, dtype)
    size = size.cpu().numpy()
    return mass.cpu().numpy(), signal.cpu().numpy(), size[:, 0] if isotropic else size


def characterize(coords, image, radius, isotropic=True, scale_factor=None, device=0):
    """Reference ``find_link.characterize`` (find_link.py:44-79) on the MI355X: dict with ``mass``,
    ``signal`` and ``size`` (isotropic) or ``size_z`` / ``size_y`` / ``size_x`` of the features at
    ``coords`` [N, ndim] of one frame.  ``scale_factor=None`` reads
    ``image.metadata['scale_factor']`` when there is one, else 1."""
    if scale_factor is None:
        try:
            scale_factor = image.metadata['scale_factor']
        except (AttributeError, KeyError):
            scale_factor = 1.
    _lib.default_engine(device)     # EngineError without a library or a GPU
    image = np.asarray(image)
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, image.ndim)
    radius = validate_tuple(radius, image.ndim)
    mass, signal, size = characterize_arrays(image[None], coords, [0, len(coords)], radius, isotropic,
                                             scale_factor, device)
    result = dict(mass=mass, signal=signal)
    if isotropic:
        result['size'] = size
    else:
        for a, key in enumerate(_size_columns(image.ndim, False)):
            result[key] = size[:, a].copy()
    return result


def locate(frames, separation, diameter=None, minmass=0, percentile=64, margin=None, precise=True,
           device=0, dtype=None, noise_size=None, smoothing_size=None, threshold=None):
    """Features of a block of frames with their mass, signal and size: :func:`locate_maxima`,
    then :func:`characterize_arrays` with the positions still on the device, then the rows with
    ``mass >= minmass`` (reference ``find_link``, find_link.py:927-971, without the relocation loop:
    that is ``find_link.find_link``, its candidate search ``relocate.relocate_arrays``).

    ``diameter`` defaults to ``separation``; the mask radius is ``int(diameter // 2)`` per axis,
    the sizes are per axis when a diameter is given and anisotropic, and ``margin`` defaults to
    ``max(diameter // 2, separation // 2 - 1)`` per axis.  Returns a DataFrame with the columns
    (z,) y, x, mass, signal, size (or size_z, size_y, size_x), frame, rows as
    :func:`locate_maxima` orders them; these are the start values ``refine_leastsq`` wants.

    ``noise_size``, ``smoothing_size``, ``threshold``: as for :func:`locate_maxima`, the maxima
    come from the preprocessed frames, which never leave the device; mass, signal and size come
    from the RAW frames with a scale factor of 1 (find_link.py:967,994).  The default
    ``noise_size=None`` skips the preprocessing, where the reference's ``find_link`` defaults to 1."""
    if not hasattr(frames, 'shape'):
        frames = np.asarray(frames)
    shape = tuple(frames.shape)
    ndim = len(shape) - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]")
    separation = validate_tuple(separation, ndim)
    # find_link.py:923: the isotropy is that of the diameter AS GIVEN (none given: isotropic)
    isotropic = not hasattr(diameter, '__iter__') or all(d == diameter[0] for d in diameter)
    diameter = separation if diameter is None else validate_tuple(diameter, ndim)
    radius = tuple(int(d // 2) for d in diameter)
    if margin is None:
        margin = tuple(int(max(d // 2, s // 2 - 1)) for d, s in zip(diameter, separation))
    margin = validate_tuple(margin, ndim)
    if any(n <= 2 * m for n, m in zip(shape[1:], margin)):
        raise ValueError("the margin %s leaves nothing of frames of shape %s: use a smaller diameter or "
                         "separation" % (margin, shape[1:]))
    if noise_size is not None:
        from . import preprocessing
        preprocessing.check_sizes(noise_size, separation if smoothing_size is None else smoothing_size, ndim)
    _lib.default_engine(device)     # EngineError without a library or a GPU
    t, pix, pos, offset, _ = locate_arrays(frames, separation, percentile, margin, precise, device, dtype,
                                           _on_device=True, noise_size=noise_size, smoothing_size=smoothing_size,
                                           threshold=threshold)
    mass, signal, size = _characterize_device(t, pos, offset, radius, isotropic, 1., device, pix)
    result = pd.DataFrame(pos.cpu().numpy().astype(np.float64), columns=['z', 'y', 'x'][3 - ndim:])
    result['mass'] = mass.cpu().numpy()
    result['signal'] = signal.cpu().numpy()
    size = size.cpu().numpy()
    for a, key in enumerate(_size_columns(ndim, isotropic)):
        result[key] = size[:, a]
    result['frame'] = np.repeat(np.arange(len(frames), dtype=np.int64), np.diff(offset.cpu().numpy()))
    return result[result['mass'] >= minmass].reset_index(drop=True)
