"""The front-end of a table stage (``cluster_tracks``, ``drift``, ``msd``, ``vanhove``, ``static``, ``twopoint``, ``motion``, ``motion_ci``, ``shape``, ``residual``, ``contacts``, ``fit_error``):
the argument checks of a linked table, its placement on the device, the prologue and the tail of a
call.  A stage module keeps its rule, its descriptor and its outputs; what two of them would spell
alike lives here, and no stage module is imported.  Argument errors are raised before the engine is
looked up (:func:`stage`), so they need neither the library nor a GPU.
"""
import math
import sys

import numpy as np

from . import _lib


def is_tensor(x):
    torch = sys.modules.get('torch')
    return torch is not None and isinstance(x, torch.Tensor)


def integer(value, least, what):
    if isinstance(value, bool) or int(value) != value or value < least or value > 2 ** 31 - 1:
        raise ValueError("%s must be an integer >= %d, not %r" % (what, least, value))
    return int(value)


def positive(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) \
            or not math.isfinite(value) or value <= 0:
        raise ValueError("%s must be a finite positive number, not %r" % (what, value))
    return float(value)


def column(x, n, what, dtype=np.int64):
    """a 1-D table column: a tensor as it is (checked later against the device), else an ndarray"""
    if is_tensor(x):
        if x.dim() != 1 or (n is not None and x.shape[0] != n):
            raise ValueError("%s must be one-dimensional%s, not %s"
                             % (what, '' if n is None else ' with %d entries' % n, tuple(x.shape)))
        return x
    x = np.asarray(x)
    if x.ndim != 1 or (n is not None and len(x) != n):
        raise ValueError("%s must be one-dimensional%s, not %s"
                         % (what, '' if n is None else ' with %d entries' % n, x.shape))
    if x.dtype.kind not in 'iu':
        raise ValueError("%s must hold integers, not %s" % (what, x.dtype))
    return np.ascontiguousarray(x, dtype=dtype)


def int64_column(x, n, what):
    """:func:`column` of an int64 column: a tensor is not converted, so it has to be int64 already"""
    if is_tensor(x) and str(x.dtype) != 'torch.int64':
        raise ValueError("a %s tensor is int64, not %s" % (what, x.dtype))
    return column(x, n, what)


def positions(pos, what='pos'):
    """(pos, N, ndim) of a float64 [N, ndim] table: a tensor as it is, else a contiguous ndarray"""
    if not is_tensor(pos):
        pos = np.asarray(pos)
        if pos.dtype.kind not in 'fiu':
            raise ValueError("%s must hold numbers, not %s" % (what, pos.dtype))
        pos = np.ascontiguousarray(pos, dtype=np.float64)
    if len(pos.shape) != 2 or pos.shape[1] not in (2, 3):
        raise ValueError("%s must be [N, ndim] with ndim 2 or 3, not %s" % (what, tuple(pos.shape)))
    return pos, int(pos.shape[0]), int(pos.shape[1])


def offsets(frame_offset):
    """(frame_offset, T) of an int64 [T + 1] column"""
    frame_offset = column(frame_offset, None, 'frame_offset')
    if frame_offset.shape[0] < 1:
        raise ValueError("frame_offset must have T + 1 >= 1 entries")
    return frame_offset, int(frame_offset.shape[0]) - 1


def particles(particle, n, n_particles):
    """(particle, P or None): None where a tensor has to be read for it (:func:`count_particles`)"""
    particle = column(particle, n, 'particle')
    if n_particles is None:
        if is_tensor(particle):
            return particle, None
        n_particles = max(int(particle.max()) + 1, 0) if particle.shape[0] else 0
    elif isinstance(n_particles, bool) or int(n_particles) != n_particles or n_particles < 0:
        raise ValueError("n_particles must be an integer >= 0")
    if n_particles > 2 ** 31 - 2:
        raise ValueError("more than 2^31 - 2 particles")
    return particle, int(n_particles)


def count_particles(par_t, n):
    """P = ``particle.max() + 1`` of the ``n`` ids on the device: one host read"""
    n_particles = max(int(par_t.max().item()) + 1, 0) if n else 0
    if n_particles > 2 ** 31 - 2:
        raise ValueError("more than 2^31 - 2 particles")
    return n_particles


def on_device(x, dev, dtype, what):
    """a contiguous tensor of ``dtype`` on ``dev`` from an ndarray, or the tensor itself (checked, not converted)"""
    import torch
    if is_tensor(x):
        if x.device != dev or x.dtype != dtype:
            raise ValueError("a %s tensor is %s on %s" % (what, str(dtype).replace('torch.', ''), dev))
        return x.contiguous()
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


class stage:
    """``with stage(device) as (eng, dev):`` the prologue of a call, in this order: the engine
    (``EngineError`` without a library or a GPU; it loads torch's HIP runtime before the library where
    torch is not imported yet), then torch, then ``cuda:device`` as the current device."""

    def __init__(self, device):
        self.device = device

    def __enter__(self):
        eng = _lib.default_engine(self.device)
        import torch
        dev = torch.device('cuda', self.device)
        self.guard = torch.cuda.device(dev)
        self.guard.__enter__()
        return eng, dev

    def __exit__(self, *exc):
        return self.guard.__exit__(*exc)


def results(as_tensor, status, ok, refused, *tensors):
    """the tail of a call: the tensors as they are (no host read), or, after the one read of
    ``status`` (``ValueError(refused)`` unless it is ``ok``), as ndarrays"""
    if as_tensor:
        return tensors
    if int(status.item()) != ok:
        raise ValueError(refused)
    return tuple(x.cpu().numpy() for x in tensors)


_LINK_FIRST = {'particle': ': link it first (find_link, link_df)', 'cluster': ': label it first (find_clusters)'}


def frame_sorted(f, pos_columns, t_column, extra=(), with_pos=True, particle=True):
    """the rows of the DataFrame ``f`` sorted by frame, the frames dense from the first to the last:
    (order, frame_offset, first_frame, ids, dense particle, pos_columns, pos) and then the int64 values of
    every column of ``extra``.  ``particle=False``: a table of features that need not be linked; ids and
    dense are None, and a missing column is no hint to link or label the table."""
    integers = (('particle',) if particle else ()) + tuple(extra) + (t_column,)
    for col in integers:
        if col not in f:
            raise ValueError("the table has no %r column%s" % (col, _LINK_FIRST.get(col, '') if particle else ''))
    if with_pos:
        if pos_columns is None:
            pos_columns = ['z', 'y', 'x'] if 'z' in f else ['y', 'x']
        pos_columns = list(pos_columns)
        if [c for c in pos_columns if c not in f] or len(pos_columns) not in (2, 3):
            raise ValueError("pos_columns must name 2 or 3 columns of the table, not %r" % (pos_columns,))
    if len(f) == 0:
        raise ValueError("an empty table has no frames")
    for col in integers:
        if np.asarray(f[col].values).dtype.kind not in 'iu':
            raise ValueError("the %r column must hold integers, not %s" % (col, f[col].values.dtype))
    frames = f[t_column].values.astype(np.int64)
    order = np.argsort(frames, kind='stable')
    first = int(frames.min())
    length = int(frames.max()) - first + 1
    offset = np.searchsorted(frames[order] - first, np.arange(length + 1), side='left').astype(np.int64)
    ids = dense = None
    if particle:
        ids, dense = np.unique(f['particle'].values[order], return_inverse=True)
        dense = dense.astype(np.int64).reshape(-1)
    pos = np.ascontiguousarray(f[pos_columns].values[order], dtype=np.float64) if with_pos else None
    return (order, offset, first, ids, dense, pos_columns, pos) \
        + tuple(f[col].values[order].astype(np.int64) for col in extra)
