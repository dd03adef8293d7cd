"""Centre-of-mass refinement of features on the MI355X (``ctr_refine_com_device``):
what the reference's ``find_link(refine=True)`` asks of ``trackpy.refine(image, image, radius,
coords, separation=0, characterize=False)`` (find_link.py:436-465).

trackpy is not part of the reference's tree.  The rule (include/ctrefine.h) is trackpy's
``refine_com`` loop restated from its published source and made total: a start closer to the edge
of the frame than the radius is clipped into the frame, where trackpy would slice out of it.
Parity with trackpy itself is not pinned; the loop that applies the rule after every level of
``find_link`` is the reference's and is pinned by fixtures.  There is no CPU fallback.
"""
import numpy as np

from . import _abi, _lib
from .find import _device_frames
from .utils import validate_tuple

MAX_ITERATIONS = 10     # trackpy's defaults
SHIFT_THRESH = 0.6


def check_arguments(max_iterations, shift_thresh):
    """(max_iterations, shift_thresh) as the descriptor takes them; ``ValueError`` beyond the rule"""
    if int(max_iterations) != max_iterations or not 1 <= max_iterations <= 100:
        raise ValueError("max_iterations must be an integer in [1, 100]")
    if not float(shift_thresh) > 0:
        raise ValueError("shift_thresh must be greater than 0")
    return int(max_iterations), float(shift_thresh)


def descriptor(shape, pixel_type, n_frames, radius, max_iterations=MAX_ITERATIONS, shift_thresh=SHIFT_THRESH):
    """An ``_abi.RefineCom`` with its scalars set (no pointer): frames of ``shape`` ((z,) y, x)."""
    ndim = len(shape)
    radius = validate_tuple(radius, ndim)
    if any(int(r) != r for r in radius):
        raise ValueError("radius must be integer")
    d = _abi.RefineCom()
    d.ndim, d.frame_dtype, d.n_frames = ndim, _abi.DTYPE_CODES[np.dtype(pixel_type)], int(n_frames)
    for a in range(ndim):
        d.shape[a] = int(shape[a])
        d.radius[a] = int(radius[a])
    d.max_iterations, d.shift_thresh = check_arguments(max_iterations, shift_thresh)
    return d


def refine_com_arrays(frames, pos, frame_offset, radius, max_iterations=MAX_ITERATIONS, shift_thresh=SHIFT_THRESH,
                      device=0, dtype=None, _on_device=False):
    """Centre-of-mass refinement of the features of a block of frames (``ctr_refine_com_device``).

    frames: ndarray [T, (z,) y, x] or a torch tensor on cuda:``device`` (as for ``locate_arrays``);
    pos: [N, ndim] starts sorted by frame, float64 or int32, ndarray or tensor on the device;
    frame_offset: [T + 1] int64, rows ``[off[t], off[t + 1])`` belong to frame t -- what
    ``locate_arrays`` and ``find_link_arrays`` return goes in as it is.  radius: integer per axis,
    at least 1, with ``2 * radius + 1`` no wider than the frame; max_iterations: 1 .. 100;
    shift_thresh: greater than 0.

    Returns ``(pos float64 [N, ndim], mass float64 [N], n_iter int32 [N])``: the centre of mass of
    the last window evaluated, the sum of its masked pixels (not divided by any scale factor) and
    the number of windows evaluated -- NumPy arrays for arrays, torch tensors on the device for
    tensors (``_on_device``, internal: tensors whatever came in).
    ``ValueError`` for a start that is not a number, and for arguments beyond the rule."""
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    tensors_in = isinstance(frames, torch.Tensor)
    t, pix = _device_frames(frames, device, dtype)
    ndim = t.dim() - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]")
    dev = t.device
    n_frames = int(t.shape[0])
    d = descriptor(tuple(t.shape[1:]), pix, n_frames, radius, max_iterations, shift_thresh)
    with torch.cuda.device(dev):
        if isinstance(pos, torch.Tensor):
            if pos.device != dev:
                raise ValueError("pos must be on cuda:%d (it is on %s)" % (device, pos.device))
            if pos.dtype not in (torch.int32, torch.float64):
                raise ValueError("a position tensor is int32 or float64, not %s" % pos.dtype)
            pos_t = pos.to(torch.float64).contiguous()
        else:
            pos = np.ascontiguousarray(pos, dtype=np.float64)
            pos_t = torch.from_numpy(pos.reshape(-1, ndim) if pos.size == 0 else pos).to(dev)
        if pos_t.dim() != 2 or pos_t.shape[1] != ndim:
            raise ValueError("pos must be [N, %d]" % ndim)
        n = int(pos_t.shape[0])
        if bool(torch.isnan(pos_t).any()):
            raise ValueError("pos holds a NaN: a start must be a number")
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
        out = torch.empty((n, ndim), dtype=torch.float64, device=dev)
        mass = torch.empty(n, dtype=torch.float64, device=dev)
        n_iter = torch.empty(n, dtype=torch.int32, device=dev)
        d.n_features = n
        if n:       # (an empty tensor has no address to pass)
            d.frames, d.frame_offset, d.pos = t.data_ptr(), off_t.data_ptr(), pos_t.data_ptr()
            d.pos_out, d.mass, d.n_iter = out.data_ptr(), mass.data_ptr(), n_iter.data_ptr()
        eng.on_current_stream(eng.refine_com_device, d, dev=dev)    # n == 0: the descriptor is still checked
    if _on_device or tensors_in:
        return out, mass, n_iter
    return out.cpu().numpy(), mass.cpu().numpy(), n_iter.cpu().numpy()


def refine_com(image, coords, radius, max_iterations=MAX_ITERATIONS, shift_thresh=SHIFT_THRESH, device=0):
    """The one-frame form, as ``trackpy.refine(image, image, radius, coords, separation=0,
    characterize=False)`` is called by the reference: ``coords`` [N, ndim] in (z,) y, x order of
    ``image``; returns float64 [N, ndim + 1], the refined positions in (z,) y, x order, then the
    mass.  The rule and its arguments: :func:`refine_com_arrays`."""
    _lib.default_engine(device)     # EngineError without a library or a GPU
    image = np.asarray(image)
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, image.ndim)
    pos, mass, _ = refine_com_arrays(image[None], coords, [0, len(coords)], radius, max_iterations, shift_thresh,
                                     device)
    return np.concatenate([pos, mass[:, None]], axis=1)
