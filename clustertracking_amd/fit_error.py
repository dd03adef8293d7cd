"""Standard errors and covariance of a fitted table on the MI355X (``ctr_fit_error_device``):
the other step after ``refine_leastsq`` / ``refine_arrays``.  ``residual`` answers how well the model
describes the image; this answers how well every parameter is determined.  It forms the exact Hessian
of the reference's objective (``FitFunctions.get_residual``, fitfunc.py:421-450) at a fitted table, per
cluster, for every profile, parameter mode and pixel type, and returns the reference's
``sqrt(2 diag(inv H))`` (refine.py:400-406) -- what ``compute_error`` gives for the Gaussian only --
and, on request, the covariance of the cluster's variables.  For two overlapping features the errors
of the two positions are correlated, so the error of their distance is not the sum of the position
errors: :func:`distance_std` takes it from the covariance.  Gaussian clusters of the large-cluster path (more
than 64 rows or ``CTR_MAX_VARS`` = 127 variables) stay out of scope: they come back ``TOO_LARGE``.

With ``mask_pos=None`` the masks sit on the fitted positions, while ``refine_leastsq``'s own ``_std``
uses the centres of the last round: the two agree exactly only when ``mask_pos`` holds those centres.
The frames are the raw frames (``noise_size`` / ``threshold`` are not taken, as in ``residual``).

The rule is the project's own (``include/ctrefine.h`` has it in the same words; ``tests/_fit_error.py``
restates it in NumPy with plain loops); bounds and constraints do not enter, as in the reference.

  Clusters.  A cluster is the set of rows of one frame with one value of `cluster`; the rows need
    not be contiguous in the table; within a cluster the rows are taken in ascending row order.
  Variables.  The layout is that of vect_from_params (fitfunc.py:207-263) for the modes of the
    columns, in column order: a CTR_MODE_VAR column gives one variable per row, a
    CTR_MODE_CLUSTER column one variable per cluster, a CTR_MODE_CONST column none;
    CTR_MODE_GLOBAL is refused.  The background is CONST or CLUSTER.  The value of a cluster
    variable is that of the cluster's first row where all its rows are equal (as
    ctr_batch.params_out has them), else their sum in row order divided by their number; the
    model reads that value for every row.  A constant background is that of the first row.
  Pixels.  Covering, box clipping, r2, g and the NaN rule of the ring and disc "safe" forms are
    ctr_residual's "Covering" and "Term of a row", with the values of the variables as above.
    P is the number of pixels covered by at least one row of the cluster, NaN pixels included,
    whatever other clusters cover.  A pixel whose residual is NaN enters no sum (the reference's
    nansum).
  Residual and Hessian.  res(x) = image(x) - background - sum_i signal_i g(r2_i(x), e_i) over the
    covering rows of the cluster in row order.  F = sum res^2 / (P norm), norm = max(frame)^2 /
    residual_factor (refine.py:354), the frame maximum of ctr_frame_max_device.  The Hessian of F
    is 2 (J^T J + Q) / (P norm): J the Jacobian of res in the variables, Q = sum_x res(x)
    d2res(x), exact in all variables -- signal, centres, sizes and every profile parameter.  With
    m = s g(r2(c, size), e): m_ss = 0, m_sp = g' r2_p, m_se = g_e, m_pq = s (g'' r2_p r2_q + g'
    r2_pq), m_pe = s g'_e r2_p, m_ee' = s g_ee' (p, q over centres and sizes, ' the derivative in
    r2), and d2res = -d2m.  r2_c = -2 d / size^2, r2_size = -2 d^2 / size^3 (isotropic: -2 q /
    size^3, q the sum of d^2), r2_cc = 2 / size^2, r2_c,size = 4 d / size^3, r2_size,size = 6 d^2
    / size^4 (isotropic: 6 q / size^4), all others 0.  gauss (k = ndim / 2): g' = -k g, g'' = k^2 g.
    ring and disc through r = sqrt(r2): g' = g_r / (2 r), g'' = g_rr / (4 r2) - g_r / (4 r^3), g'_e
    = g_re / (2 r), with g = exp(phi), g_a = g phi_a, g_ab = g (phi_a phi_b + phi_ab); ring: phi =
    -k w^2, w = (r - 1 + e) / e; disc: phi = -k u^2, u = (r - ds) / (1 - ds), in the region r2 <=
    ds^2 g = 1 with all derivatives 0, the clamp disc_size >= 1 -> 0.999 has derivative 0 in
    disc_size, disc_size <= 0 is the Gaussian.  inv_series: g = e0 / y, y the polynomial in r2; g'
    = -e0 y' / y^2, g'' = e0 (2 y'^2 / y^3 - y'' / y^2), g_e0 = 1 / y, g_ek = -e0 r2^(N - k) / y^2,
    g_e0,ek = -r2^(N - k) / y^2, g_ek,el = 2 e0 r2^(N - k) r2^(N - l) / y^3, g'_e0 = -y' / y^2, g'_ek
    = -e0 ((N - k) r2^(N - k - 1) / y^2 - 2 y' r2^(N - k) / y^3).  Where the safe form makes the
    disc's g 1 (q < 1, disc_size > 0) all derivatives are 0.  A feature's block in parameter space
    is added to the rows and columns of the variables its parameters map to; a shared variable
    collects every feature's block.
  Result.  A = J^T J + Q is factored by Cholesky; a pivot that is not a positive finite number
    makes the cluster CTR_FITERR_NOT_POSITIVE_DEFINITE.  Otherwise cov = P norm A^-1 and std_v =
    sqrt(cov_vv).  params_std [N, n_params] is vect_to_params of std: a cluster variable's value
    goes on every row of the cluster, a constant column is NaN, a failed cluster is all NaN.
  Statuses, per cluster (every row carries its cluster's), as data and never as errors:
    CTR_FITERR_OK; CTR_FITERR_NOT_POSITIVE_DEFINITE; CTR_FITERR_NONFINITE, a non-finite
    parameter in a variable or in a value the model reads (a mask centre included);
    CTR_FITERR_EMPTY, P == 0; CTR_FITERR_TOO_LARGE, more than 64 rows or more than CTR_MAX_VARS
    variables (n_pix is then 0 and the cluster has no covariance block); CTR_FITERR_BAD_TABLE
    on every row, when frame_offset, order, cluster_offset or the offsets of the covariance do
    not fit together or a cluster's rows lie in more than one frame.
  Order of the sums.  The covered pixels of a cluster are numbered by owner (the lowest covering
    row of the cluster, in row order) and, within an owner, in row-major order of the clipped box
    of its mask; every entry of J^T J adds the pixels in that order.  The block of a feature adds
    the pixels of its box as ctr_residual's per-feature sums do (lane l the pixels l, l + 64, ...,
    then the butterfly), and the blocks are added to A after J^T J in row order.  Cholesky and
    the inverse take their terms in index order.
No float atomics; every output is the same bytes on every call, on every stream, whatever else is
in the batch.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import collections

import numpy as np

from . import _abi, _tables
from .residual import fit_model

FitError = collections.namedtuple('FitError', [
    'params_std', 'status', 'n_vars', 'n_pix', 'cov', 'cov_offset', 'var_row', 'var_col'])

OK, NOT_POSITIVE_DEFINITE, NONFINITE, EMPTY, TOO_LARGE, BAD_TABLE = (
    _abi.FITERR_OK, _abi.FITERR_NOT_POSITIVE_DEFINITE, _abi.FITERR_NONFINITE, _abi.FITERR_EMPTY,
    _abi.FITERR_TOO_LARGE, _abi.FITERR_BAD_TABLE)

_REFUSED = "frame_offset must not decrease, from 0 to the number of rows, and n_clusters must be the number of clusters"


def model(fit_function, ndim, diameter, param_mode=None):
    """``(ff, radius, isotropic, CTR_FIT_* code, profile parameters)`` with the modes of
    ``FitFunctions(fit_function, ndim, isotropic, param_mode)``.  Refuses what ``refine_leastsq``
    refuses, with its messages: ``NotImplementedError`` for a dict fit function and for the
    ``param_mode`` values 'global', 'particle' and 'frame'; ``ValueError`` as ``residual.fit_model``."""
    from .refine import _check_options
    _, radius, isotropic, code, n_profile = fit_model(fit_function, ndim, diameter)
    ff = _check_options(ndim, diameter, None, fit_function, param_mode, None, 1)[4]
    return ff, radius, isotropic, code, n_profile


def descriptor(shape, pixel_type, n_frames, n_features, n_clusters, diameter, fit_function='gauss', param_mode=None,
               residual_factor=100000., want_cov=False, max_grid=0):
    """An ``_abi.FitError`` with its scalars set (no pointer): what ``_lib.fit_error_plan`` takes.
    ``shape``: (z,) y, x of a frame."""
    ndim = len(shape)
    ff, radius, isotropic, code, n_profile = model(fit_function, ndim, diameter, param_mode)
    d = _abi.FitError()
    d.ndim, d.frame_dtype, d.fit_function, d.isotropic = ndim, _abi.DTYPE_CODES[np.dtype(pixel_type)], code, int(isotropic)
    d.n_profile, d.want_cov, d.max_grid = n_profile, int(bool(want_cov)), int(max_grid)
    d.n_frames, d.n_features, d.n_clusters = int(n_frames), int(n_features), int(n_clusters)
    d.residual_factor = _tables.positive(residual_factor, 'residual_factor')
    for k, mode in enumerate(ff.modes):
        d.modes[k] = mode
    for a in range(ndim):
        d.shape[a], d.radius[a] = int(shape[a]), radius[a]
    return d


def _check(frames, params, frame_offset, cluster, diameter, fit_function, param_mode, mask_pos, residual_factor, n_clusters):
    """everything refused before any device work"""
    if not hasattr(frames, 'shape'):
        frames = np.asarray(frames)
    ndim = len(frames.shape) - 1
    ff = model(fit_function, ndim, diameter, param_mode)[0]
    _tables.positive(residual_factor, 'residual_factor')
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
    cluster = _tables.int64_column(cluster, n, 'cluster')
    if mask_pos is not None:
        mask_pos, m, mdim = _tables.positions(mask_pos, 'mask_pos')
        if m != n or mdim != ndim:
            raise ValueError("mask_pos must be [%d, %d], not %s" % (n, ndim, tuple(mask_pos.shape)))
    if n_clusters is not None:
        n_clusters = _tables.integer(n_clusters, 0, 'n_clusters')
        if n_clusters > n:
            raise ValueError("n_clusters (%d) is more than the number of rows (%d)" % (n_clusters, n))
    return frames, params, frame_offset, cluster, mask_pos, n_clusters, ndim, n, n_frames


def fit_error_arrays(frames, params, frame_offset, cluster, diameter, fit_function='gauss', param_mode=None,
                     mask_pos=None, residual_factor=100000., want_cov=False, n_clusters=None, device=0, _max_grid=0):
    """The standard errors of a fitted table and, with ``want_cov``, the covariance of every cluster
    (the rule of the module; ``ctr_fit_error_device``).

    frames ``[T, (z,) y, x]`` of any of the six pixel types; params float64 ``[N, n_params]`` in the
    column order of ``FitFunctions(fit_function, ndim, isotropic).params`` -- ``RefineResult.params``;
    frame_offset ``[T + 1]``; cluster int64 ``[N]``, any label that is one value per cluster of a frame
    (``RefineResult.cluster``; the labels of two frames may coincide); diameter, fit_function and
    param_mode as ``refine_leastsq`` takes them; mask_pos float64 ``[N, ndim]``, the centres of the
    masks, or None for the positions in params; n_clusters: the number of clusters, or None to read
    it from the device.  ndarrays, or tensors on ``cuda:device``: tensor params in, tensors out, and
    with ``n_clusters`` given and without ``want_cov`` nothing is read back (the length of ``cov`` is
    data: ``want_cov`` reads it); ndarrays in, ndarrays out.

    Returns ``FitError(params_std float64 [N, n_params], status int32 [N], n_vars int32 [N], n_pix
    int64 [N], cov float64, cov_offset int64 [C + 1], var_row int64, var_col int32)``: per row the
    status (``fit_error.OK``, ``NOT_POSITIVE_DEFINITE``, ``NONFINITE``, ``EMPTY``, ``TOO_LARGE``;
    ``BAD_TABLE`` on every row for offsets of a tensor that do not rise from 0 to N or an
    ``n_clusters`` that is not the number of clusters), the variables and the covered pixels of its
    cluster.  The clusters are numbered in the order of (frame, label); cluster c has the block
    ``cov[cov_offset[c] : cov_offset[c + 1]]``, ``n_vars x n_vars`` in row-major order (NaN for a failed
    cluster, absent for one that is ``TOO_LARGE``), and its variables follow those of the clusters
    before it in ``var_row`` and ``var_col``: variable v is column ``var_col[v]`` of table row
    ``var_row[v]`` (-1: a variable of the cluster).  The four are None without ``want_cov``.

    Raises before any device work: ``NotImplementedError`` for a dict fit function and for
    ``param_mode`` 'global'; ``ValueError`` for an unknown profile, shapes that do not fit together
    and the offsets of an ndarray that do not rise from 0 to N.  ``EngineError`` without a library or
    a GPU."""
    frames, params, frame_offset, cluster, mask_pos, n_clusters, ndim, n, n_frames = _check(
        frames, params, frame_offset, cluster, diameter, fit_function, param_mode, mask_pos, residual_factor, n_clusters)
    as_tensor = _tables.is_tensor(params)
    with _tables.stage(device) as (eng, dev):
        import torch
        from .find import _device_frames
        if not _tables.is_tensor(frames) and frames.dtype not in _abi.DTYPE_CODES:
            frames = frames.astype(np.float64)
        frames_t, pix = _device_frames(frames, device, None)
        shape = tuple(int(s) for s in frames_t.shape[1:])
        par_t = _tables.on_device(params, dev, torch.float64, 'params')
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        cl_t = _tables.on_device(cluster, dev, torch.int64, 'cluster')
        mp_t = None if mask_pos is None else _tables.on_device(mask_pos, dev, torch.float64, 'mask_pos')
        i64 = dict(dtype=torch.int64, device=dev)
        # the rows grouped by (frame, label), the row order kept inside a group: two stable sorts
        rows = torch.arange(n, **i64)
        frame_of = torch.searchsorted(off_t[1:].contiguous(), rows, right=True)
        by_label = torch.sort(cl_t, stable=True)[1]
        order = by_label[torch.sort(frame_of[by_label], stable=True)[1]] if n else rows
        start = torch.ones(n, dtype=torch.bool, device=dev)
        if n > 1:
            start[1:] = (frame_of[order][1:] != frame_of[order][:-1]) | (cl_t[order][1:] != cl_t[order][:-1])
        if n_clusters is None:
            n_clusters = int(start.sum().item())
        c = n_clusters
        cluster_offset = torch.searchsorted(torch.cumsum(start, 0) - 1, torch.arange(c + 1, **i64))
        d = descriptor(shape, pix, n_frames, n, c, diameter, fit_function, param_mode, residual_factor, want_cov, _max_grid)
        np_cols = par_t.shape[1]
        std = torch.empty((n, np_cols), dtype=torch.float64, device=dev)
        status, n_vars = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        n_pix = torch.empty(n, **i64)
        cov = cov_offset = var_offset = var_row = var_col = None
        if want_cov:
            modes = [d.modes[k] for k in range(np_cols)]
            size = torch.diff(cluster_offset)
            nv = size * modes.count(_abi.MODE_VAR) + modes.count(_abi.MODE_CLUSTER)
            nv = torch.where((size > _abi.FITERR_MAX_ROWS) | (nv > _abi.MAX_VARS), torch.zeros_like(nv), nv)
            zero = torch.zeros(1, **i64)
            var_offset = torch.cat([zero, torch.cumsum(nv, 0)])
            cov_offset = torch.cat([zero, torch.cumsum(nv * nv, 0)])
            totals = torch.stack([var_offset[-1], cov_offset[-1]]).cpu()      # the one read: the lengths are data
            d.n_vars_total, d.n_cov_total = int(totals[0]), int(totals[1])
            cov = torch.empty(d.n_cov_total, dtype=torch.float64, device=dev)
            var_row = torch.empty(d.n_vars_total, **i64)
            var_col = torch.empty(d.n_vars_total, dtype=torch.int32, device=dev)
        ptr = lambda x: None if x is None else (x.data_ptr() or None)     # (an empty tensor has no address to pass)
        d.frames, d.frame_offset, d.params, d.mask_pos = ptr(frames_t), ptr(off_t), ptr(par_t), ptr(mp_t)
        d.order, d.cluster_offset, d.var_offset, d.cov_offset = ptr(order), ptr(cluster_offset), ptr(var_offset), ptr(cov_offset)
        d.params_std, d.status, d.n_vars, d.n_pix = ptr(std), ptr(status), ptr(n_vars), ptr(n_pix)
        d.cov, d.var_row, d.var_col = ptr(cov), ptr(var_row), ptr(var_col)
        eng.on_current_stream(eng.fit_error_device, d, dev=dev)
        out = (std, status, n_vars, n_pix, cov, cov_offset, var_row, var_col)
        if as_tensor:
            return FitError(*out)
        out = FitError(*(None if x is None else x.cpu().numpy() for x in out))
        if n and out.status[0] == BAD_TABLE:
            raise ValueError(_REFUSED)
        return out


def fit_error(f, reader, diameter, separation=None, fit_function='gauss', param_mode=None, pos_columns=None,
              t_column='frame', residual_factor=100000., device=0):
    """The table form of :func:`fit_error_arrays`: ``f`` a DataFrame of fitted features, as
    ``refine_leastsq`` returns it; ``reader`` the frames it was fitted to, as ``refine_leastsq`` takes
    them.  The parameter columns of ``f`` are read through ``FitFunctions`` as ``residual`` reads them;
    the clusters are those of ``f['cluster']`` where present, otherwise of ``find_clusters(f,
    separation)`` (``separation`` defaults to ``diameter``).  The masks sit on the fitted positions.

    Returns a copy of ``f`` with the ``<param>_std`` columns that ``refine_leastsq(compute_error=True)``
    adds (NaN for a constant column and for a cluster that is not ``OK``), and ``std_status``, the
    status of the row's cluster."""
    from .find import find_clusters
    from .refine import _normalise_reader
    from .utils import guess_pos_columns
    if pos_columns is None:
        pos_columns = guess_pos_columns(f)
    pos_columns = list(pos_columns)
    f = f.copy()
    frames_src, ndim, _ = _normalise_reader(f, reader, t_column)
    if ndim != len(pos_columns):
        raise ValueError("the frames have %d dimensions and pos_columns names %d" % (ndim, len(pos_columns)))
    ff = model(fit_function, ndim, diameter, param_mode)[0]
    if 'cluster' not in f:
        labelled = find_clusters(f, diameter if separation is None else separation, pos_columns, t_column)
        f['cluster'] = labelled['cluster'].reindex(f.index)
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
    offset = np.searchsorted(index.reshape(-1), np.arange(len(numbers) + 1), side='left').astype(np.int64)
    params = np.stack(cols, axis=1)[order] if len(f) else np.zeros((0, ff.n_params))
    cluster = np.asarray(f['cluster'].values)[order].astype(np.int64)
    if len(numbers):
        frames = np.stack([np.asarray(frames_src[int(i)]) for i in numbers])
    else:
        frames = np.zeros((0,) + (1,) * ndim, dtype=np.uint8)
    out = fit_error_arrays(frames, params, offset, cluster, diameter, fit_function, param_mode,
                           residual_factor=residual_factor, device=device)
    for k, name in enumerate(ff.params):
        col = pos_columns[ff.pos_columns.index(name)] if name in ff.pos_columns else name
        back = np.empty(len(f))
        back[order] = out.params_std[:, k]
        f[col + '_std'] = back
    back = np.empty(len(f), dtype=np.int32)
    back[order] = out.status
    f['std_status'] = back
    return f


def distance_std(result, params, row_a, row_b, mpp=1., ndim=None):
    """The standard error of the distance between rows ``row_a`` and ``row_b`` of one cluster, from
    the covariance of a :func:`fit_error_arrays` call with ``want_cov`` (``result``) on ``params``:
    the delta method on the position variables, sqrt(g^T cov g) with g the gradient of the distance
    (``mpp``: a scalar or one factor per axis, applied to the coordinates; ``ndim``: the number of
    position columns, by default the length of a sequence ``mpp``, else 2).  A constant position
    contributes nothing, a position shared by the cluster cancels.  NaN for rows of different
    clusters, a failed cluster and coincident rows."""
    if result.cov is None:
        raise ValueError("distance_std needs the covariance: call fit_error_arrays with want_cov=True")
    to_np = lambda x: x.detach().cpu().numpy() if _tables.is_tensor(x) else np.asarray(x)
    cov, cov_offset, var_row, var_col = (to_np(x) for x in (result.cov, result.cov_offset, result.var_row, result.var_col))
    status, params = to_np(result.status), to_np(params)
    var_offset = np.concatenate([[0], np.cumsum(np.rint(np.sqrt(np.diff(cov_offset))).astype(np.int64))])
    if ndim is None:
        ndim = len(mpp) if np.ndim(mpp) else 2
    where_a, where_b = np.flatnonzero(var_row == row_a), np.flatnonzero(var_row == row_b)
    if row_a == row_b or status[row_a] != OK or status[row_b] != OK or not len(where_a) or not len(where_b):
        return np.nan
    c = int(np.searchsorted(var_offset, where_a[0], side='right')) - 1
    if not var_offset[c] <= where_b[0] < var_offset[c + 1]:
        return np.nan
    v0, nv = int(var_offset[c]), int(var_offset[c + 1] - var_offset[c])
    block = cov[cov_offset[c]:cov_offset[c + 1]].reshape(nv, nv)
    scale = np.broadcast_to(np.asarray(mpp, dtype=np.float64), (ndim,))
    delta = (params[row_a, 2:2 + ndim] - params[row_b, 2:2 + ndim]) * scale
    dist = np.sqrt(np.sum(delta * delta))
    g = np.zeros(nv)
    for a in range(ndim):
        for rows, sign in ((where_a, 1.), (where_b, -1.)):
            for v in rows:
                if var_col[v] == 2 + a:
                    g[v - v0] += sign * delta[a] * scale[a] / dist
    return float(np.sqrt(g @ block @ g))


# ``ct.fit_error`` is the function: what a caller reaches through it
fit_error.distance_std = distance_std
fit_error.OK, fit_error.NOT_POSITIVE_DEFINITE, fit_error.NONFINITE = OK, NOT_POSITIVE_DEFINITE, NONFINITE
fit_error.EMPTY, fit_error.TOO_LARGE, fit_error.BAD_TABLE = EMPTY, TOO_LARGE, BAD_TABLE
