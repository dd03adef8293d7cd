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
                  dtype=None, capacity=None):
    """The device pass behind :func:`locate_maxima`: (positions int32 [N, ndim] in frame order,
    frame_offset int64 [T + 1], per-frame threshold float64 [T]) as NumPy arrays.
    ``capacity``: rows to reserve at first; a larger buffer is taken when the frames hold more."""
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    t, pix = _device_frames(frames, device, dtype)
    ndim = t.dim() - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]")
    separation = validate_tuple(separation, ndim)
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
            cur = torch.cuda.current_stream(dev)
            if cur.cuda_stream:
                eng.locate_maxima_device(loc, cur.cuda_stream)
            else:   # legacy default stream: the engine's stream, ordered by events on the device
                eng.engine_wait_stream(0)
                eng.locate_maxima_device(loc, 0)
                eng.stream_wait_engine(0)
            torch.cuda.synchronize(dev)
            n = int(total.item())
            if n <= capacity:
                break
            capacity = n        # more maxima than rows: run again with room for all of them
        return (pos[:n].cpu().numpy(), offset.cpu().numpy(), thr[:n_frames].cpu().numpy())


def locate_maxima(frames, separation, percentile=64, margin=None, precise=True, device=0,
                  dtype=None):
    """Local maxima of every frame of a block by the rule of reference ``grey_dilation``,
    on the MI355X.

    frames: ndarray [T, (z,) y, x] or a torch tensor already on cuda:``device`` (for example
    ``device.draw_frames`` output); ``dtype=np.uint16`` reads an int16 tensor as unsigned.
    Returns a DataFrame with the position columns ((z,) y, x; float64) and ``frame``, rows in
    frame order and, within a frame, in the order :func:`grey_dilation` returns them."""
    pos, offset, _ = locate_arrays(frames, separation, percentile, margin, precise, device, dtype)
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
