"""``refine_global`` -- the reference's ``refine_leastsq`` with a ``param_mode`` ``'global'``
(``clustertracking/refine.py:317-332``) on the MI355X (``ctr_refine_global_device``):
one value per global column for all features of a problem, fitted together with whatever varies per
feature (``'var'``) or per cluster (``'cluster'``).  This is how the one ``size`` of a monodisperse
sample, the ``thickness`` of a ring or the ``disc_size`` of a batch of particles is measured while
positions, signals and backgrounds stay free.

The damped normal matrix of such a problem is an arrowhead over its clusters; the engine
eliminates every cluster's own variables in the cluster's workgroup, solves the small shared
system per problem and back-substitutes (include/ctrefine.h has the rule).  ``refine_leastsq`` and
``refine_arrays`` keep refusing global columns; ``train_leastsq`` is the case with everything
else constant.  There is no CPU fallback.
"""
from collections import namedtuple

import numpy as np

from . import _abi, _lib
from .find import _device_frames, find_clusters
from .fitfunc import FitFunctions
from .refine import _normalise_reader
from .train import XTOL, FTOL, CHECK_EVERY, pack_problems as _pack_globals
from .utils import ArrayReader, guess_pos_columns, is_isotropic, validate_tuple

GlobalResult = namedtuple('GlobalResult', ['params', 'cost', 'status', 'n_rounds', 'n_iter', 'globals', 'global_names'])

MAX_COLUMNS = _abi.REFINE_GLOBAL_MAX_COLUMNS
MAX_FEATURES = _abi.TRAIN_MAX_FEATURES


def global_param_mode(fit_function, ndim, isotropic, param_mode=None):
    """The ``FitFunctions`` of a global fit: the reference's defaults (background ``'cluster'``,
    signal and positions ``'var'``, the rest ``'const'``) with ``param_mode`` on top.
    ``NotImplementedError`` for a dict fit function, a global position, the modes ``'particle'`` /
    ``'frame'`` and for no global column at all."""
    if isinstance(fit_function, dict):
        raise NotImplementedError("custom (dict) fit functions need Python callbacks per evaluation "
                                  "and are not supported by the MI355X engine")
    ff = FitFunctions(fit_function, ndim, isotropic, param_mode)
    for param, m in zip(ff.params, ff.modes):
        if m not in (_abi.MODE_CONST, _abi.MODE_VAR, _abi.MODE_GLOBAL, _abi.MODE_CLUSTER):
            raise NotImplementedError("param modes 'particle'/'frame' are not implemented "
                                      "(reference refine.py:339-340): %r" % param)
        if m == _abi.MODE_GLOBAL and param in ff.pos_columns:
            raise NotImplementedError("a global position (%r) is not supported: background, signal, the "
                                      "sizes and the profile's parameters may be global" % param)
    n_glob = ff.modes.count(_abi.MODE_GLOBAL)
    if n_glob == 0:
        raise NotImplementedError("no parameter is global: refine_leastsq fits per-feature and "
                                  "per-cluster parameters")
    if n_glob > _abi.REFINE_GLOBAL_MAX_GLOBALS:
        raise NotImplementedError("%d global columns, the engine takes %d" % (n_glob, _abi.REFINE_GLOBAL_MAX_GLOBALS))
    return ff


def n_locals(ff, n_features):
    """L_c of a cluster of ``n_features``: one per ``'cluster'`` column, one per feature and ``'var'`` column"""
    return ff.modes.count(_abi.MODE_CLUSTER) + int(n_features) * ff.modes.count(_abi.MODE_VAR)


def pack_problems(ff, params, feat_offset, problem_offset, bounds, radius):
    """The start vector and the box of a call (refine.py:361-364, fitfunc.py:535-558):
    ``(start, low, high [P, G], local_start, local_low, local_high [C, max_locals], max_locals)``.
    A global column: the mean over the problem's rows, the min of the lows, the max of the highs.
    The locals of a cluster, in column order: a ``'cluster'`` column the same over the cluster's
    rows, a ``'var'`` column every row's own value and bounds."""
    params = np.asarray(params, dtype=np.float64)
    start, low, high = _pack_globals(ff, params, feat_offset, problem_offset, bounds, radius)
    lo_f, hi_f = ff.feature_bounds(ff.validate_bounds(bounds, radius=radius), params)
    sizes = np.diff(feat_offset)
    n_cl = len(sizes)
    lm = max([n_locals(ff, n) for n in sizes], default=0)
    ls, ll, lh = (np.zeros((n_cl, lm)) for _ in range(3))
    # whole columns at once; only the mean of a cluster of two or more rows is taken cluster by cluster
    # (np.mean's own order of summation: the reference's bytes)
    sizes = np.asarray(sizes, dtype=np.int64)
    first = np.asarray(feat_offset[:-1], dtype=np.int64)
    cl = np.repeat(np.arange(n_cl), sizes)
    rank = np.arange(len(params)) - first[cl]
    full = np.flatnonzero(sizes > 0)
    # (reduceat over the starts alone would run an empty cluster into the next one: every segment gets its own end)
    seg = np.stack([first[full], first[full] + sizes[full]], 1).ravel()
    pad = lambda x: np.append(x, x[-1:])      # (an index equal to the length ends the last segment)
    at = np.zeros(n_cl, dtype=np.int64)
    for k, m in enumerate(ff.modes):
        if m == _abi.MODE_VAR:
            col = at[cl] + rank
            ls[cl, col], ll[cl, col], lh[cl, col] = params[:, k], lo_f[:, k], hi_f[:, k]
            at += sizes
        elif m == _abi.MODE_CLUSTER:
            empty = np.flatnonzero(sizes == 0)
            ls[empty, at[empty]], ll[empty, at[empty]], lh[empty, at[empty]] = np.nan, -np.inf, np.inf
            if len(full):
                ls[full, at[full]] = params[first[full], k]
                ll[full, at[full]] = np.minimum.reduceat(pad(lo_f[:, k]), seg)[::2]
                lh[full, at[full]] = np.maximum.reduceat(pad(hi_f[:, k]), seg)[::2]
            for c in np.flatnonzero(sizes > 1):
                ls[c, at[c]] = np.mean(np.ascontiguousarray(params[feat_offset[c]:feat_offset[c + 1], k]))
            at += 1
    return start, low, high, ls, ll, lh, lm


def descriptor(ff, shape, pixel_type, n_frames, radius, max_iter=10, max_shift=1., max_rms_dev=1.,
               residual_factor=100000., solver_maxiter=100, xtol=0., ftol=0., check_every=CHECK_EVERY):
    """An ``_abi.RefineGlobal`` with its scalars set (no pointer, no count)."""
    d = _abi.RefineGlobal()
    d.ndim, d.isotropic = ff.ndim, int(ff.isotropic)
    d.fit_function, _ = _abi.fit_code(ff.fit_function)
    d.n_params = len(ff.params)
    if d.n_params > _abi.MAX_PARAMS:
        raise NotImplementedError("%s: %d parameter columns, the engine takes %d"
                                  % (ff.fit_function, d.n_params, _abi.MAX_PARAMS))
    for k, m in enumerate(ff.modes):
        d.modes[k] = int(m)
    for a in range(ff.ndim):
        d.radius[a] = int(radius[a])
        d.shape[a] = int(shape[a])
    d.frame_dtype = _abi.DTYPE_CODES[np.dtype(pixel_type)]
    d.n_frames = int(n_frames)
    d.solver_maxiter, d.max_iter, d.check_every = int(solver_maxiter), int(max_iter), int(check_every)
    d.residual_factor, d.max_rms_dev, d.max_shift = float(residual_factor), float(max_rms_dev), float(max_shift)
    d.xtol, d.ftol = float(xtol), float(ftol)
    return d


def _host(x, dtype):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


def refine_global_arrays(frames, params, feat_offset, frame_index, problem_offset, diameter, fit_function='gauss',
                         param_mode=None, bounds=None, max_iter=10, max_shift=1, max_rms_dev=1.,
                         residual_factor=100000., solver_maxiter=100, check_every=CHECK_EVERY, device=0,
                         xtol=XTOL, ftol=FTOL, dtype=None, max_locals=None):
    """Fit the shared and the per-feature parameters of P independent problems in one device call
    (``ctr_refine_global_device``; the rule: include/ctrefine.h).

    frames: ndarray [T, (z,) y, x] or a torch tensor on cuda:``device``; params: [N, n_params] in the
    column order of ``FitFunctions.params``; feat_offset [C + 1]: the features of cluster c are the
    rows ``[off[c], off[c + 1])``; frame_index [C]: its frame; problem_offset [P + 1]: problem p owns
    the clusters ``[off[p], off[p + 1])``.  Arrays or tensors; the tables are read on the host (start
    values and bounds come from them).  ``param_mode``: as for the reference's ``refine_leastsq``,
    with at least one ``'global'`` column.  ``check_every``: iterations between two reads of the count
    of finished problems (same results for any value).  ``max_locals``: the caller's statement of the
    most locals of a cluster, as the C call takes it (default: counted from ``feat_offset``, and a
    cluster beyond the kernels raises ``NotImplementedError``); with a statement nothing is counted
    here and the device answers a cluster beyond it with ``STATUS_TOO_LARGE`` for its problem.

    Returns ``GlobalResult(params [N, n_params], cost [P], status [P], n_rounds [P], n_iter [P],
    globals [P, G], global_names)`` -- NumPy arrays, or tensors on the device where ``frames`` was one.
    A failed problem keeps its rows, has NaN cost and globals and a non-zero status
    (``_abi.STATUS_TEXT``); nothing is raised for it."""
    if int(max_iter) < 1:
        raise ValueError("max_iter must be at least 1")
    if int(check_every) < 1:
        raise ValueError("check_every must be at least 1")
    frames_nd = frames.dim() if hasattr(frames, 'dim') else np.ndim(frames)
    ndim = frames_nd - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]")
    diameter = validate_tuple(diameter, ndim)
    radius = tuple(int(x) // 2 for x in diameter)
    isotropic = is_isotropic(diameter)
    ff = global_param_mode(fit_function, ndim, isotropic, param_mode)
    names = [p for p, m in zip(ff.params, ff.modes) if m == _abi.MODE_GLOBAL]

    params = _host(params, np.float64)
    feat_offset = _host(feat_offset, np.int32)
    frame_index = _host(frame_index, np.int32)
    problem_offset = _host(problem_offset, np.int32)
    n_cl, n_prob = len(frame_index), len(problem_offset) - 1
    if params.ndim != 2 or params.shape[1] != len(ff.params):
        raise ValueError("params must be [n_features, %d]" % len(ff.params))
    if feat_offset.shape != (n_cl + 1,) or feat_offset[0] != 0 or feat_offset[-1] != len(params) \
            or np.any(np.diff(feat_offset) < 0):
        raise ValueError("feat_offset must be [n_clusters + 1], rising from 0 to the number of features")
    if n_prob < 0 or problem_offset[0] != 0 or problem_offset[-1] != n_cl or np.any(np.diff(problem_offset) < 0):
        raise ValueError("problem_offset must be [n_problems + 1], rising from 0 to the number of clusters")
    sizes = np.diff(feat_offset)
    if n_cl and max_locals is None:
        c = int(np.argmax(sizes))
        cols = n_locals(ff, sizes[c]) + len(names) + 1
        if sizes[c] > MAX_FEATURES or cols > MAX_COLUMNS:
            raise NotImplementedError("cluster %d has %d features (%d columns: locals, globals and the residual): "
                                      "the global-fit kernels take clusters of up to %d features and %d columns"
                                      % (c, sizes[c], cols, MAX_FEATURES, MAX_COLUMNS))
    start, low, high, ls, ll, lh, lm = pack_problems(ff, params, feat_offset, problem_offset, bounds, radius)
    if max_locals is not None:     # the tables as stated: a longer cluster's row is cut, the device refuses it
        lm = int(max_locals)
        ls, ll, lh = (np.ascontiguousarray(np.pad(x, ((0, 0), (0, max(0, lm - x.shape[1]))))[:, :lm]) for x in (ls, ll, lh))

    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    tensors_in = isinstance(frames, torch.Tensor)
    t, pix = _device_frames(frames, device, dtype)
    if n_cl and (frame_index.min() < 0 or frame_index.max() >= t.shape[0]):
        raise ValueError("frame_index out of range")
    d = descriptor(ff, tuple(t.shape[1:]), pix, int(t.shape[0]), radius, max_iter, max_shift, max_rms_dev,
                   residual_factor, solver_maxiter, xtol, ftol, check_every)
    d.n_problems, d.n_clusters, d.n_features = n_prob, n_cl, len(params)
    d.max_features = int(sizes.max()) if n_cl else 0
    d.max_locals = lm
    dev = t.device
    with torch.cuda.device(dev):
        up = [torch.from_numpy(x).to(dev) for x in (params, feat_offset, frame_index, problem_offset, start, low, high,
                                                    ls, ll, lh)]
        out_p = torch.empty((len(params), len(ff.params)), dtype=torch.float64, device=dev)
        out_g = torch.full((n_prob, len(names)), float('nan'), dtype=torch.float64, device=dev)
        out_c = torch.full((n_prob,), float('nan'), dtype=torch.float64, device=dev)
        out_s = torch.zeros(n_prob, dtype=torch.int32, device=dev)
        out_r = torch.zeros(n_prob, dtype=torch.int32, device=dev)
        out_n = torch.zeros(n_prob, dtype=torch.int32, device=dev)
        ptr = lambda x: x.data_ptr() if x.numel() else None     # (an empty tensor has no address to pass)
        d.frames = ptr(t)
        (d.params, d.feat_offset, d.frame_index, d.problem_offset, d.start, d.low, d.high,
         d.local_start, d.local_low, d.local_high) = [ptr(x) for x in up]
        d.params_out, d.globals, d.cost, d.status = ptr(out_p), ptr(out_g), ptr(out_c), ptr(out_s)
        d.n_rounds, d.n_iter = ptr(out_r), ptr(out_n)
        if n_prob == 0:
            out_p.copy_(up[0])
        eng.on_current_stream(eng.refine_global_device, d, dev=dev)
        torch.cuda.current_stream(dev).synchronize()   # the tables uploaded here live until the kernels have read them
    outs = (out_p, out_c, out_s, out_r, out_n, out_g)
    if not tensors_in:
        outs = tuple(x.cpu().numpy() for x in outs)
    return GlobalResult(*outs, names)


def refine_global(f, reader, diameter, separation=None, fit_function='gauss', param_mode=None, param_val=None,
                  bounds=None, pos_columns=None, t_column='frame', max_iter=10, max_shift=1, max_rms_dev=1.,
                  residual_factor=100000., per_frame=False, **kwargs):
    """``refine_leastsq`` with global columns (reference refine.py:317-332) on the MI355X engine.

    Signature and result follow the reference: a copy of ``f`` with the columns ``cluster``,
    ``cluster_size``, the parameter columns and ``cost`` -- the same on every row of a problem; a
    failed problem keeps its rows and has a NaN cost.  ``per_frame=True`` makes every frame a
    problem of its own, all in one device call (the reference fits the whole table as one).

    Differences, all deliberate: the minimiser is the engine's bounded Levenberg-Marquardt run to
    convergence (``tol`` and ``method`` are accepted and ignored, ``options['maxiter']`` caps the
    iterations of a round; engine keys ``xtol``, ``ftol``, ``device``, ``cluster_labels``,
    ``check_every``).  ``constraints``, ``compute_error``, ``noise_size`` / ``threshold``, a dict fit
    function, a global position and a ``param_mode`` without a global column raise
    ``NotImplementedError`` before any device work, and so does a cluster beyond 48 columns."""
    options = dict(maxiter=100)
    options.update(kwargs.pop('options', None) or {})
    kwargs.pop('method', None)
    kwargs.pop('tol', None)
    xtol, ftol = kwargs.pop('xtol', XTOL), kwargs.pop('ftol', FTOL)
    device = kwargs.pop('device', 0)
    cluster_labels = kwargs.pop('cluster_labels', 'reference')
    check_every = kwargs.pop('check_every', CHECK_EVERY)
    if kwargs.pop('constraints', None):
        raise NotImplementedError("constraints are not implemented in a global fit")
    if kwargs.pop('compute_error', False):
        raise NotImplementedError("compute_error is not implemented in a global fit")
    if kwargs.pop('noise_size', None) is not None or kwargs.pop('threshold', None) is not None:
        raise NotImplementedError("noise_size / threshold (the lowpass of the window) is not implemented in a global fit")
    if kwargs:
        raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
    if int(max_iter) < 1:
        raise ValueError("max_iter must be at least 1")

    if pos_columns is None:
        pos_columns = guess_pos_columns(f)
    f = f.copy()
    frames_src, ndim, _ = _normalise_reader(f, reader, t_column)
    if ndim != len(pos_columns):
        raise ValueError("%d position columns for %d-dimensional frames" % (len(pos_columns), ndim))
    diameter = validate_tuple(diameter, ndim)
    isotropic = is_isotropic(diameter)
    ff = global_param_mode(fit_function, ndim, isotropic, param_mode)   # raises first
    # the table's own names of the parameter columns: the positions are pos_columns, in axis order
    pos_columns = list(pos_columns)
    cols = [pos_columns[ff.pos_columns.index(c)] if c in ff.pos_columns else c for c in ff.params]
    if separation is None:
        separation = diameter

    # the frames of the table, in order, as one block
    frame_vals = f[t_column].values
    uniq = np.unique(frame_vals)
    if isinstance(frames_src, ArrayReader):
        frames = np.stack([frames_src.array[int(i)] for i in uniq]) if len(uniq) else frames_src.array[:0]
    else:
        frames = np.stack([np.asarray(frames_src[int(i)]) for i in uniq])
    if frames.dtype not in _abi.DTYPE_CODES:
        frames = frames.astype(np.float64)

    f = find_clusters(f, separation, pos_columns, t_column, labels=cluster_labels, device=device)
    if param_val is not None:
        for col in param_val:
            f[col] = param_val[col]
    for col in cols:
        if col not in f.columns:
            f[col] = ff.default[col]
    dense = np.searchsorted(uniq, f[t_column].values)

    # groupby([frame, cluster]) order, as prepare_batch
    order = np.lexsort((f['cluster'].values, dense))
    fr_s, cl_s = dense[order], f['cluster'].values[order]
    new = np.ones(len(order), dtype=bool)
    new[1:] = (fr_s[1:] != fr_s[:-1]) | (cl_s[1:] != cl_s[:-1])
    starts = np.flatnonzero(new)
    feat_offset = np.append(starts, len(order)).astype(np.int32)
    frame_index = fr_s[starts].astype(np.int32)
    if per_frame:
        problem_offset = np.searchsorted(frame_index, np.arange(len(uniq) + 1)).astype(np.int32)
    else:
        problem_offset = np.array([0, len(starts)], dtype=np.int32)
    params = f[cols].values.astype(np.float64)[order]

    back = {_abi.MODE_CONST: 'const', _abi.MODE_VAR: 'var', _abi.MODE_GLOBAL: 'global', _abi.MODE_CLUSTER: 'cluster'}
    res = refine_global_arrays(frames, params, feat_offset, frame_index, problem_offset, diameter, fit_function,
                               param_mode={p: back[m] for p, m in zip(ff.params, ff.modes)}, bounds=bounds,
                               max_iter=max_iter, max_shift=max_shift, max_rms_dev=max_rms_dev,
                               residual_factor=residual_factor, solver_maxiter=int(options.get('maxiter', 100)),
                               check_every=check_every, device=device, xtol=xtol, ftol=ftol)
    # refine.py:408-431: the rows of a problem that succeeded, and the problem's cost on each of them
    rows_of = np.repeat(np.arange(len(problem_offset) - 1), np.diff(feat_offset[problem_offset]))
    out = np.empty_like(res.params)
    out[order] = res.params
    cost = np.empty(len(order))
    cost[order] = res.cost[rows_of]
    f[cols] = out
    f['cost'] = cost
    return f
