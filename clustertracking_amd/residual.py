"""Model and residual frames of a fitted table on the MI355X (``ctr_residual_device``):
the step after ``refine_leastsq`` / ``refine_arrays``.  Those return one number per cluster, ``cost``,
measured on the window of the last round and thrown away with it; this draws the fitted model back
into the frames, subtracts it, and returns the goodness-of-fit sums per feature and per cluster by the
rule of the reference's ``FitFunctions.get_residual`` (fitfunc.py:421-450; what ``display.show_fit``
shows there).  A feature that the location missed inside a cluster is a bright blob of the residual
frame, which goes straight into ``locate_arrays``.  The residual is against the raw frame
(``noise_size`` / ``threshold`` are not taken), and constraints do not enter the model.

The rule is the project's own (``include/ctrefine.h`` has it in the same words; ``tests/_residual.py``
restates it in NumPy with plain loops over the rows).  No operation is contracted to a fused
multiply-add.

For pixel x of frame t and the rows i of that frame in ascending row order:
  Covering.  Row i covers x when sum(((x - mask_pos_i) / radius)**2) <= 1, evaluated as NumPy
    does: per axis a division, a product and a sum, in axis order, each rounded once; the edge is
    included.  The box of a mask is clipped to the frame: a centre outside the frame covers
    whatever part of its ellipse lies inside, a non-finite centre covers nothing.
  Per-pixel maps.  coverage(x) is the number of covering rows (int32), owner(x) the lowest
    covering row, or -1.
  Term of a row.  term_i(x) = signal_i * g(r2_i(x)), with r2 and g as the refine kernels evaluate
    them: d_a = x_a - pos_a, r2 = the sum over the axes, in axis order, of (d_a * d_a) * (1 / (size_a
    * size_a)), every operation rounded on its own.  gauss: g = exp(-0.5 ndim r2).  ring (e =
    thickness): r = sqrt(r2), num = r - 1 + e, g = exp(-0.5 ndim ((num / e) * (num / e))).  disc (e =
    disc_size): e <= 0 the Gaussian; else ds = e, or 0.999 where e >= 1; g = 1 unless r2 > ds ds,
    where u = (sqrt(r2) - ds) / (1 - ds), g = exp(u u ndim / -2).  inv_series_<N> (e[0 .. N]): g = e[0] / y,
    y = polyval([1, e[1], ..., e[N]], r2) in Horner's order.  For ring and disc these are the
    reference's r2_*_safe forms: where q = the sum of d_a d_a over the axes, last axis first, is
    below 1, g is NaN (the disc with disc_size > 0 has the value 1 there, as the reference's
    disc_func leaves it).
  Residual.  residual(x) = ((image(x) - background_owner) - term_i1) - term_i2 ... over the covering
    rows in ascending row order (fitfunc.py:443-448).
  Model.  model(x) = background_owner + s, where s starts from 0 and takes the terms of the
    covering rows in the same order.
  Outside every mask.  outside decides the residual: 0.0 ('zero'), NaN ('nan') or
    float64(image(x)) ('image'); model is 0.0, NaN or 0.0 respectively.
  Per feature [N].  n_pix: covered pixels; n_own: pixels with owner == i; n_nan: covered pixels
    whose residual is NaN; sum, sum_sq, max_abs: over its covered pixels whose residual is not NaN
    (the reference's nansum; 0 where there is none); own_sum_sq: the same over its owned pixels;
    rms = sqrt(sum_sq / n_pix), the divisor counting the NaN pixels as len(image) does there, NaN
    for n_pix == 0.  Order of the sums: the pixels of the clipped box of the mask (every axis from
    floor(max(c - radius - 1, 0)) to ceil(min(c + radius + 1, shape - 1))) are numbered in
    row-major order; lane l of the feature's wavefront adds the pixels l, l + 64, ... in that order,
    and the 64 lane sums are added by the butterfly x += x[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.
  Per cluster, only when cluster is given; per row [N], every row carrying its cluster's value.
    cluster_n_pix = the sum of n_own over the rows of the cluster, cluster_sum_sq = the sum of
    own_sum_sq, in ascending row order; cost = sqrt(cluster_sum_sq / cluster_n_pix) / max(frame_t).
    Where the masks of different clusters do not overlap (always for separation >= diameter),
    cluster_sum_sq / cluster_n_pix is what get_residual(..., norm=1.) returns for that cluster, and
    with mask_pos the last round's centres cost is ``refine_leastsq``'s ``cost``.
No float atomics; every output is the same bytes on every call, on every stream, and a frame's
outputs do not depend on which other frames are in the call.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import collections

import numpy as np

from . import _abi, _tables
from .fitfunc import FIT_FUNCTION_CODES, FitFunctions
from .utils import validate_tuple

Residual = collections.namedtuple('Residual', [
    'residual', 'model', 'coverage', 'owner', 'n_pix', 'n_own', 'n_nan', 'sum', 'sum_sq', 'own_sum_sq', 'max_abs',
    'rms', 'cluster_n_pix', 'cluster_sum_sq', 'cost', 'status'])

OUTSIDE = {'zero': _abi.RESID_ZERO, 'nan': _abi.RESID_NAN, 'image': _abi.RESID_IMAGE}


def fit_model(fit_function, ndim, diameter):
    """What the stage takes from the model: ``(ff, radius, isotropic, CTR_FIT_* code, profile
    parameters)``.  ``NotImplementedError`` for a dict fit function; ``ValueError`` for an unknown
    profile, for an ``inv_series`` order beyond ``CTR_MAX_PARAMS`` columns and for a bad diameter."""
    if isinstance(ndim, bool) or ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]: ndim 2 or 3, not %r" % (ndim,))
    diameter = validate_tuple(diameter, ndim)
    if any(isinstance(d, bool) or int(d) != d or d < 2 for d in diameter):
        raise ValueError("diameter must hold integers >= 2 (the mask radius is diameter // 2), not %r" % (diameter,))
    radius = tuple(int(d) // 2 for d in diameter)
    isotropic = all(d == diameter[0] for d in diameter)
    ff = FitFunctions(fit_function, ndim, isotropic)
    n_profile = len(ff.params) - 2 - ndim - len(ff.size_columns)
    if ff.n_params > _abi.MAX_PARAMS or n_profile > _abi.INV_SERIES_MAX_PROFILE:
        raise ValueError("%s has %d parameter columns: at most %d (CTR_MAX_PARAMS)"
                         % (fit_function, ff.n_params, _abi.MAX_PARAMS))
    code = FIT_FUNCTION_CODES[fit_function if fit_function in FIT_FUNCTION_CODES else 'inv_series']
    return ff, radius, isotropic, code, n_profile


def descriptor(shape, pixel_type, n_frames, n_features, diameter, fit_function='gauss', outside='zero',
               want_model=False, want_frames=True, has_cluster=False, max_grid=0):
    """An ``_abi.Residual`` with its scalars set (no pointer): what ``_lib.residual_plan`` takes.
    ``shape``: (z,) y, x of a frame; ``max_grid`` > 0 lowers the cap on every grid (a test switch)."""
    ndim = len(shape)
    _, radius, isotropic, code, n_profile = fit_model(fit_function, ndim, diameter)
    if outside not in OUTSIDE:
        raise ValueError("outside must be 'zero', 'nan' or 'image', not %r" % (outside,))
    d = _abi.Residual()
    d.ndim, d.frame_dtype, d.fit_function, d.isotropic = ndim, _abi.DTYPE_CODES[np.dtype(pixel_type)], code, int(isotropic)
    d.n_profile, d.outside = n_profile, OUTSIDE[outside]
    d.want_frames, d.want_model, d.has_cluster, d.max_grid = int(bool(want_frames)), int(bool(want_model)), int(bool(has_cluster)), int(max_grid)
    d.n_frames, d.n_features = int(n_frames), int(n_features)
    for a in range(ndim):
        d.shape[a], d.radius[a] = int(shape[a]), radius[a]
    return d


def _check(frames, params, frame_offset, diameter, fit_function, mask_pos, cluster, outside):
    """everything refused before any device work: (frames, params, frame_offset, mask_pos, cluster, ndim, N, T)"""
    if not hasattr(frames, 'shape'):
        frames = np.asarray(frames)
    ndim = len(frames.shape) - 1
    ff = fit_model(fit_function, ndim, diameter)[0]
    if outside not in OUTSIDE:
        raise ValueError("outside must be 'zero', 'nan' or 'image', not %r" % (outside,))
    if not _tables.is_tensor(params):
        params = np.asarray(params)
        if params.dtype.kind not in 'fiu':
            raise ValueError("params must hold numbers, not %s" % params.dtype)
        params = np.ascontiguousarray(params, dtype=np.float64)
    if len(params.shape) != 2 or params.shape[1] != ff.n_params:
        raise ValueError("params must be [N, %d] (%s), not %s" % (ff.n_params, ', '.join(ff.params), tuple(params.shape)))
    n, n_frames = int(params.shape[0]), int(frames.shape[0])
    if n >= 2 ** 31 - 1:
        raise ValueError("%d rows: one call takes fewer than 2**31 - 1" % n)
    frame_offset, t = _tables.offsets(frame_offset)
    if t != n_frames:
        raise ValueError("frame_offset must have one entry per frame and one more (%d), not %d" % (n_frames + 1, t + 1))
    if not _tables.is_tensor(frame_offset) and \
            (frame_offset[0] != 0 or frame_offset[-1] != n or np.any(np.diff(frame_offset) < 0)):
        raise ValueError("frame_offset must not decrease, from 0 to the number of rows (%d)" % n)
    if mask_pos is not None:
        mask_pos, m, mdim = _tables.positions(mask_pos, 'mask_pos')
        if m != n or mdim != ndim:
            raise ValueError("mask_pos must be [%d, %d], not %s" % (n, ndim, tuple(mask_pos.shape)))
    if cluster is not None:
        cluster = _tables.int64_column(cluster, n, 'cluster')
    return frames, params, frame_offset, mask_pos, cluster, ndim, n, n_frames


def residual_arrays(frames, params, frame_offset, diameter, fit_function='gauss', mask_pos=None, cluster=None,
                    outside='zero', want_model=False, want_frames=True, device=0, _max_grid=0):
    """The model and residual frames of a fitted table and its goodness-of-fit sums (the rule of the
    module; ``ctr_residual_device``).

    frames ``[T, (z,) y, x]`` of any of the six pixel types (u8, u16, i16, i32, f32, f64); params
    float64 ``[N, n_params]`` in the column order of ``FitFunctions(fit_function, ndim,
    isotropic).params`` -- ``RefineResult.params``; frame_offset ``[T + 1]``; diameter gives the mask
    radius ``d // 2`` per axis as ``refine_leastsq`` does, an anisotropic one means anisotropic size
    columns; mask_pos float64 ``[N, ndim]``, the centres of the masks, or None for the positions in
    params; cluster int64 ``[N]``, the smallest row of the row's cluster (``RefineResult.cluster``), or
    None; outside 'zero', 'nan' or 'image'.  ndarrays, or tensors on ``cuda:device``: tensor params in,
    tensors out, and nothing is read back (``status`` then says whether the table was taken:
    ``_abi.RESID_OK``, ``RESID_BAD_TABLE``, ``RESID_BAD_CLUSTER``); ndarrays in, ndarrays out and
    ``ValueError`` for a refused table.

    Returns ``Residual(residual, model float64 [T, (z,) y, x], coverage, owner int32 of the same shape,
    n_pix, n_own, n_nan int64 [N], sum, sum_sq, own_sum_sq, max_abs, rms float64 [N], cluster_n_pix int64
    [N], cluster_sum_sq, cost float64 [N], status int32 [1])``; what was not asked for is None: model
    without ``want_model``, residual, coverage and owner without ``want_frames``, the last three
    without ``cluster``.

    Raises before any device work: ``NotImplementedError`` for a dict fit function; ``ValueError`` for
    an unknown profile, an ``inv_series`` order beyond ``CTR_MAX_PARAMS`` columns, shapes that do not
    fit together, an ``outside`` other than the three, and the offsets of an ndarray that do not rise
    from 0 to N (those of a tensor are checked by the stage's first kernel and reported in
    ``status``).  ``EngineError`` without a library or a GPU."""
    frames, params, frame_offset, mask_pos, cluster, ndim, n, n_frames = _check(
        frames, params, frame_offset, diameter, fit_function, mask_pos, cluster, outside)
    as_tensor = _tables.is_tensor(params)
    with _tables.stage(device) as (eng, dev):
        import torch
        from .find import _device_frames
        if not _tables.is_tensor(frames) and frames.dtype not in _abi.DTYPE_CODES:
            frames = frames.astype(np.float64)
        frames_t, pix = _device_frames(frames, device, None)
        shape = tuple(int(s) for s in frames_t.shape[1:])
        d = descriptor(shape, pix, n_frames, n, diameter, fit_function, outside, want_model, want_frames,
                       cluster is not None, _max_grid)
        par_t = _tables.on_device(params, dev, torch.float64, 'params')
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        mp_t = None if mask_pos is None else _tables.on_device(mask_pos, dev, torch.float64, 'mask_pos')
        cl_t = None if cluster is None else _tables.on_device(cluster, dev, torch.int64, 'cluster')
        full = (n_frames,) + shape
        res = torch.empty(full, dtype=torch.float64, device=dev) if want_frames else None
        cov, own = ((torch.empty(full, dtype=torch.int32, device=dev) for _ in range(2)) if want_frames else (None, None))
        mdl = torch.empty(full, dtype=torch.float64, device=dev) if want_model else None
        n_pix, n_own, n_nan = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
        s1, s2, so, mx, rms = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(5))
        c_n = torch.empty(n, dtype=torch.int64, device=dev) if cluster is not None else None
        c_sq, cost = ((torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2)) if cluster is not None else (None, None))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ptr = lambda x: None if x is None else (x.data_ptr() or None)     # (an empty tensor has no address to pass)
        d.frames, d.frame_offset, d.params, d.mask_pos, d.cluster = ptr(frames_t), ptr(off_t), ptr(par_t), ptr(mp_t), ptr(cl_t)
        d.residual, d.model, d.coverage, d.owner = ptr(res), ptr(mdl), ptr(cov), ptr(own)
        d.n_pix, d.n_own, d.n_nan = ptr(n_pix), ptr(n_own), ptr(n_nan)
        d.sum, d.sum_sq, d.own_sum_sq, d.max_abs, d.rms = ptr(s1), ptr(s2), ptr(so), ptr(mx), ptr(rms)
        d.cluster_n_pix, d.cluster_sum_sq, d.cost = ptr(c_n), ptr(c_sq), ptr(cost)
        d.status = status.data_ptr()
        eng.on_current_stream(eng.residual_device, d, dev=dev)
        out = (res, mdl, cov, own, n_pix, n_own, n_nan, s1, s2, so, mx, rms, c_n, c_sq, cost, status)
        if as_tensor:
            return Residual(*out)
        code = int(status.item())
        if code == _abi.RESID_BAD_TABLE:
            raise ValueError("frame_offset must not decrease, from 0 to the number of rows (%d)" % n)
        if code == _abi.RESID_BAD_CLUSTER:
            raise ValueError("cluster must hold, for every row, the smallest row of its cluster in its frame")
        return Residual(*(None if x is None else x.cpu().numpy() for x in out))


def residual(f, reader, diameter, fit_function='gauss', pos_columns=None, t_column='frame', cluster_column=None,
             mask_pos_columns=None, outside='zero', return_frames=False, device=0):
    """The table form of :func:`residual_arrays`: ``f`` a DataFrame of fitted features, as
    ``refine_leastsq`` returns it; ``reader`` the frames it was fitted to, as ``refine_leastsq`` takes them
    -- a sequence with ``frame_shape`` indexed by the frame number (``utils.ArrayReader``), or one frame.  The parameter columns of ``f`` are read through
    ``FitFunctions`` as ``prepare_batch`` does (a missing profile parameter or background takes its
    default); ``mask_pos_columns`` names the columns of the mask centres where they are not the
    positions; ``cluster_column`` the column of cluster labels (``'cluster'`` of ``refine_leastsq``).

    Returns a copy of ``f`` with the columns ``res_rms``, ``res_max`` (``max_abs``), ``res_n``
    (``n_pix``) and ``res_nan`` (``n_nan``), with a ``cluster_column`` also ``res_cost``; with
    ``return_frames`` a tuple of that and the residual block, an ndarray with one frame per frame
    number that occurs in ``f``, in ascending order."""
    from .refine import _normalise_reader
    from .utils import guess_pos_columns
    if pos_columns is None:
        pos_columns = guess_pos_columns(f)
    pos_columns = list(pos_columns)
    f = f.copy()
    frames_src, ndim, _ = _normalise_reader(f, reader, t_column)
    if ndim != len(pos_columns):
        raise ValueError("the frames have %d dimensions and pos_columns names %d" % (ndim, len(pos_columns)))
    ff = fit_model(fit_function, ndim, diameter)[0]
    if outside not in OUTSIDE:
        raise ValueError("outside must be 'zero', 'nan' or 'image', not %r" % (outside,))
    cols = []
    for name in ff.params:
        col = pos_columns[ff.pos_columns.index(name)] if name in ff.pos_columns else name
        if col in f:
            cols.append(np.asarray(f[col].values, dtype=np.float64))
        elif name in ff.default:
            cols.append(np.full(len(f), ff.default[name]))
        else:
            raise ValueError("the table has no %r column" % col)
    frame_no = np.asarray(f[t_column].values).astype(np.int64)
    order = np.argsort(frame_no, kind='stable')
    numbers, index = np.unique(frame_no[order], return_inverse=True)
    offset = np.searchsorted(index, np.arange(len(numbers) + 1), side='left').astype(np.int64)
    params = np.stack(cols, axis=1)[order] if len(f) else np.zeros((0, ff.n_params))
    mask_pos = None
    if mask_pos_columns is not None:
        mask_pos = np.ascontiguousarray(f[list(mask_pos_columns)].values[order], dtype=np.float64)
    cluster = None
    if cluster_column is not None:
        # the smallest row of every (frame, label), in the sorted order
        _, group = np.unique(np.stack([index.reshape(-1), np.asarray(f[cluster_column].values)[order]], axis=1), axis=0,
                             return_inverse=True)
        group = group.reshape(-1)
        first = np.full(group.max() + 1 if len(group) else 0, len(f), dtype=np.int64)
        np.minimum.at(first, group, np.arange(len(f), dtype=np.int64))
        cluster = first[group]
    if len(numbers):
        frames = np.stack([np.asarray(frames_src[int(i)]) for i in numbers])
    else:
        frames = np.zeros((0,) + (1,) * ndim, dtype=np.uint8)
    out = residual_arrays(frames, params, offset, diameter, fit_function, mask_pos, cluster, outside,
                          want_model=False, want_frames=bool(return_frames), device=device)
    for name, values in (('res_rms', out.rms), ('res_max', out.max_abs), ('res_n', out.n_pix), ('res_nan', out.n_nan)) \
            + ((('res_cost', out.cost),) if cluster_column is not None else ()):
        back = np.empty(len(f), dtype=values.dtype)
        back[order] = values
        f[name] = back
    return (f, out.residual) if return_frames else f
