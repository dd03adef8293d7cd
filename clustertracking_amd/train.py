"""``train_leastsq`` -- reference ``clustertracking/refine.py:455-515`` on the MI355X
(``ctr_train_device``): the fit parameters that ``refine_leastsq`` keeps constant
(``size``, ``thickness``, ``disc_size``, ``param_*``), obtained from an image of equal features.

Positions, signal and background are held constant; everything else is fitted as one value shared
by all features (``param_mode='global'``).  With nothing varying per feature the unknowns are those
G shared values alone and the windows never move, so one iteration is a sum of a G x G normal
matrix over all pixels of all clusters and a small bounded Levenberg-Marquardt step: the engine
runs that, P independent problems per call.  General global mode -- per-feature variables beside
shared ones -- is ``refine_global`` (``refine_leastsq`` and this module refuse it).  There is no CPU
fallback.
"""
from collections import namedtuple

import numpy as np

from . import _abi, _lib
from .find import _device_frames, characterize_arrays, find_clusters
from .fitfunc import FitFunctions
from .refine import _normalise_reader
from .refine_com import refine_com_arrays
from .utils import (ArrayReader, RefineException, guess_pos_columns, is_isotropic, validate_tuple)

TrainResult = namedtuple('TrainResult', ['globals', 'cost', 'status', 'n_iter'])

# Stopping tolerances of a training call (relative step, relative predicted decrease): the rounding
# floor of float64, not the engine's 1e-9 / 1e-14.  What is trained here becomes a constant of every
# fit after it, the reference's converged run ends within a few tens of units in the last place, and
# the iterations are queued whether they are used or not.
XTOL, FTOL = 1e-15, 1e-30
# Iterations between two looks at the count of finished problems.  This layer waits for the
# results anyway, so the asynchrony of the blind queue (0, the descriptor's default) buys nothing
# here and its unused launches cost: measured on an MI355X (profiles/train_time.json) one cfg-2 frame
# 0.91 ms blind, 0.68 / 0.65 / 0.61 ms at K = 4 / 8 / 16; 1250 frames in one call 25.9 ms blind,
# 22.2 / 22.1 / 22.2 ms.  8 and 16 do not differ beyond the spread; 8 stops sooner after a short fit.
CHECK_EVERY = 8

ONLY_CONST_AND_GLOBAL = ("only constant and global parameters are trained: param_mode %r of %r is "
                         "not (refine_leastsq fits per-feature and per-cluster parameters)")


def training_param_mode(fit_function, ndim, isotropic, param_mode=None, pos_columns=None):
    """The ``FitFunctions`` of a training call (refine.py:491-501): positions, signal and
    background ``'const'``, every other parameter ``'global'``, unless ``param_mode`` names it.
    ``NotImplementedError`` for a mode other than ``'const'`` and ``'global'``, and for
    ``'global'`` on background, signal or a position."""
    if isinstance(fit_function, dict):
        raise NotImplementedError("custom (dict) fit functions need Python callbacks per evaluation "
                                  "and are not supported by the MI355X engine")
    plain = FitFunctions(fit_function, ndim, isotropic)
    if pos_columns is None:
        pos_columns = plain.pos_columns
    mode = dict(param_mode or {})
    for param in plain.params:
        if param in mode:
            continue
        mode[param] = 'const' if param in list(pos_columns) + ['signal', 'background'] else 'global'
    ff = FitFunctions(fit_function, ndim, isotropic, mode)
    for param, m in zip(ff.params, ff.modes):
        if m not in (_abi.MODE_CONST, _abi.MODE_GLOBAL):
            raise NotImplementedError(ONLY_CONST_AND_GLOBAL % (ff.param_mode[param], param))
        if m == _abi.MODE_GLOBAL and param in ['background', 'signal'] + ff.pos_columns:
            raise NotImplementedError("%r cannot be global in training: with background, signal or a "
                                      "position shared, per-feature variables couple all clusters" % param)
    if _abi.MODE_GLOBAL not in ff.modes:
        raise ValueError("no parameter is global: there is nothing to train")
    return ff


def training_bounds(bounds, size_columns):
    """``bounds`` with ``<size>_rel_diff = (0.9, 9)`` added where the caller gave none
    (refine.py:503-508); a copy."""
    bounds = dict(bounds or {})
    for col in size_columns:
        bounds.setdefault(col + '_rel_diff', (0.9, 9))   # - 90 %, + 900 %
    return bounds


def pack_problems(ff, params, feat_offset, problem_offset, bounds, radius):
    """``start, low, high [P, G]`` of the global columns: the mean of the column over the problem's
    features (refine.py:361), the minimum of the per-feature lower and the maximum of the
    per-feature upper bounds (fitfunc.py:535-558)."""
    cols = [k for k, m in enumerate(ff.modes) if m == _abi.MODE_GLOBAL]
    n_prob = len(problem_offset) - 1
    start = np.empty((n_prob, len(cols)))
    low = np.empty((n_prob, len(cols)))
    high = np.empty((n_prob, len(cols)))
    lo_f, hi_f = ff.feature_bounds(ff.validate_bounds(bounds, radius=radius), params)
    for p in range(n_prob):
        r0, r1 = int(feat_offset[problem_offset[p]]), int(feat_offset[problem_offset[p + 1]])
        for v, k in enumerate(cols):
            if r1 > r0:
                start[p, v] = np.mean(params[r0:r1, k])
                low[p, v] = np.min(lo_f[r0:r1, k])
                high[p, v] = np.max(hi_f[r0:r1, k])
            else:
                start[p, v], low[p, v], high[p, v] = np.nan, -np.inf, np.inf
    return start, low, high


def descriptor(ff, shape, pixel_type, n_frames, radius, max_rms_dev=1., residual_factor=100000.,
               solver_maxiter=100, xtol=0., ftol=0., check_every=0):
    """An ``_abi.Train`` with its scalars set (no pointer, no count)."""
    d = _abi.Train()
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
    d.solver_maxiter, d.check_every = int(solver_maxiter), int(check_every)
    d.residual_factor, d.max_rms_dev = float(residual_factor), float(max_rms_dev)
    d.xtol, d.ftol = float(xtol), float(ftol)
    return d


def _host(x, dtype):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


def train_arrays(frames, params, feat_offset, frame_index, problem_offset, diameter, fit_function='gauss',
                 modes=None, param_mode=None, bounds=None, max_rms_dev=1., residual_factor=100000.,
                 solver_maxiter=100, xtol=XTOL, ftol=FTOL, check_every=CHECK_EVERY, device=0, dtype=None):
    """Train the shared parameters of P independent problems in one device call
    (``ctr_train_device``; the rule: include/ctrefine.h).

    frames: ndarray [T, (z,) y, x] or a torch tensor on cuda:``device``; params: [N, n_params] in the
    column order of ``FitFunctions.params``; feat_offset [C + 1]: the features of cluster c are the
    rows ``[off[c], off[c + 1])``; frame_index [C]: its frame; problem_offset [P + 1]: problem p owns
    the clusters ``[off[p], off[p + 1])``.  Arrays or tensors; the tables are read on the host (start
    values and bounds come from them).  ``modes``: one ``_abi.MODE_CONST`` / ``MODE_GLOBAL`` per
    column, or ``param_mode`` as for :func:`train_leastsq` (neither: positions, signal and
    background constant, the rest global).  ``bounds``: as for ``refine_leastsq``, taken as given
    (:func:`train_leastsq` adds ``size_rel_diff``).  ``check_every``: 0 queues ``solver_maxiter + 1``
    iterations blind; K > 0 reads one word every K iterations and stops early (same results).
    ``xtol``, ``ftol``: the stopping tolerances (``XTOL``, ``FTOL``: the rounding floor).

    Returns ``TrainResult(globals [P, G], cost [P], status [P], n_iter [P])`` -- NumPy arrays, or
    tensors on the device where ``frames`` was one.  A failed problem has NaN globals and cost and a
    non-zero status (``_abi.STATUS_TEXT``); nothing is raised for it."""
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    tensors_in = isinstance(frames, torch.Tensor)
    t, pix = _device_frames(frames, device, dtype)
    ndim = t.dim() - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x]")
    diameter = validate_tuple(diameter, ndim)
    radius = tuple(int(x) // 2 for x in diameter)
    isotropic = is_isotropic(diameter)
    if modes is not None:
        if param_mode is not None:
            raise ValueError("give modes or param_mode, not both")
        names = FitFunctions(fit_function, ndim, isotropic).params
        if len(modes) != len(names):
            raise ValueError("modes must have %d entries" % len(names))
        back = {_abi.MODE_CONST: 'const', _abi.MODE_VAR: 'var', _abi.MODE_GLOBAL: 'global',
                _abi.MODE_CLUSTER: 'cluster'}
        param_mode = {name: back.get(int(m), int(m)) for name, m in zip(names, modes)}
    ff = training_param_mode(fit_function, ndim, isotropic, param_mode)

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
    if n_cl and (frame_index.min() < 0 or frame_index.max() >= t.shape[0]):
        raise ValueError("frame_index out of range")
    sizes = np.diff(feat_offset)
    if n_cl and sizes.max() > _abi.TRAIN_MAX_FEATURES:
        c = int(np.argmax(sizes))
        raise NotImplementedError("cluster %d has %d features: the training kernels take clusters of up to %d"
                                  % (c, sizes[c], _abi.TRAIN_MAX_FEATURES))
    start, low, high = pack_problems(ff, params, feat_offset, problem_offset, bounds, radius)
    n_glob = start.shape[1]

    d = descriptor(ff, tuple(t.shape[1:]), pix, int(t.shape[0]), radius, max_rms_dev, residual_factor,
                   solver_maxiter, xtol, ftol, check_every)
    d.n_problems, d.n_clusters, d.n_features = n_prob, n_cl, len(params)
    d.max_features = int(sizes.max()) if n_cl else 0
    dev = t.device
    with torch.cuda.device(dev):
        up = [torch.from_numpy(x).to(dev) for x in (params, feat_offset, frame_index, problem_offset, start, low, high)]
        out_g = torch.full((n_prob, n_glob), float('nan'), dtype=torch.float64, device=dev)
        out_c = torch.full((n_prob,), float('nan'), dtype=torch.float64, device=dev)
        out_s = torch.zeros(n_prob, dtype=torch.int32, device=dev)
        out_n = torch.zeros(n_prob, dtype=torch.int32, device=dev)
        ptr = lambda x: x.data_ptr() if x.numel() else None     # (an empty tensor has no address to pass)
        d.frames = ptr(t)
        d.params, d.feat_offset, d.frame_index, d.problem_offset, d.start, d.low, d.high = [ptr(x) for x in up]
        d.globals, d.cost, d.status, d.n_iter = ptr(out_g), ptr(out_c), ptr(out_s), ptr(out_n)
        eng.on_current_stream(eng.train_device, d, dev=dev)     # no problem: the descriptor is still checked
        torch.cuda.current_stream(dev).synchronize()   # the tables uploaded here live until the kernels have read them
    if tensors_in:
        return TrainResult(out_g, out_c, out_s, out_n)
    return TrainResult(out_g.cpu().numpy(), out_c.cpu().numpy(), out_s.cpu().numpy(), out_n.cpu().numpy())


def train_leastsq(f, reader, diameter, separation, fit_function, param_mode=None, tol=1e-7,
                  pos_columns=None, refine_com=True, per_frame=False, **kwargs):
    """Obtain fit parameters from an image of features with equal size, on the MI355X engine.
    Different signal intensities per feature are allowed.

    Signature and meaning follow reference ``train_leastsq`` (refine.py:455-515): positions, signal
    and background are constant, every other parameter of the fit function is ``'global'``;
    ``param_mode`` may move more parameters to ``'const'``; ``bounds`` gets ``size_rel_diff = (0.9,
    9)`` where none is given.  Returns ``{param: value}`` for the global parameters.  ``f`` is not
    changed (the reference writes the refined columns into it).

    Differences, all deliberate:

    * The minimiser is the engine's bounded Levenberg-Marquardt on the shared values, run to
      convergence, as in ``refine_leastsq`` here: ``tol`` and ``method`` are accepted and ignored,
      ``options['maxiter']`` (default 100) caps the iterations; engine keys ``xtol``, ``ftol``,
      ``device``, ``cluster_labels``, ``check_every``.
    * ``'var'`` or ``'cluster'`` anywhere in ``param_mode`` raises ``NotImplementedError``: only
      constant and global parameters are trained.  So do ``constraints``, ``compute_error``,
      ``noise_size`` / ``threshold`` and a dict fit function.
    * A failed fit raises ``RefineException`` (the reference's ``assert np.isfinite(f['cost']).all()``
      fires there).
    * ``per_frame=True`` trains one problem per frame, all in one device call, and returns a
      DataFrame indexed by frame with one column per global parameter: a focus drift through a
      video, for instance.
    * ``refine_com=True`` (what the reference always does, with ``trackpy.refine_com``): the
      positions are first moved by ``refine_com_arrays``, then ``signal`` and the size column(s) are
      taken from ``characterize_arrays`` at the refined positions, both on the device.  trackpy is
      not part of the reference's tree: this step is restated from what the engine already has,
      and parity with trackpy itself is not pinned (as for ``find_link(refine=True)``).
      ``refine_com=False`` uses ``f``'s own columns; that path is the one pinned to the reference.
    """
    import pandas as pd
    options = dict(maxiter=100)
    options.update(kwargs.pop('options', None) or {})
    kwargs.pop('method', None)
    xtol, ftol = kwargs.pop('xtol', XTOL), kwargs.pop('ftol', FTOL)
    device = kwargs.pop('device', 0)
    cluster_labels = kwargs.pop('cluster_labels', 'reference')
    check_every = kwargs.pop('check_every', CHECK_EVERY)
    bounds = kwargs.pop('bounds', None)
    param_val = kwargs.pop('param_val', None)
    t_column = kwargs.pop('t_column', 'frame')
    max_rms_dev = kwargs.pop('max_rms_dev', 1.)
    residual_factor = kwargs.pop('residual_factor', 100000.)
    kwargs.pop('max_iter', None)       # window rounds: the positions are constant, there is one
    kwargs.pop('max_shift', None)
    if kwargs.pop('constraints', None):
        raise NotImplementedError("constraints act on positions, which are constant in training")
    if kwargs.pop('compute_error', False):
        raise NotImplementedError("compute_error is not implemented for trained parameters")
    if kwargs.pop('noise_size', None) is not None or kwargs.pop('threshold', None) is not None:
        raise NotImplementedError("noise_size / threshold (the lowpass of the window) is not implemented in training")
    if kwargs:
        raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))

    f = f.copy()
    if pos_columns is None:
        pos_columns = guess_pos_columns(f)
    frames_src, ndim, _ = _normalise_reader(f, reader, t_column)
    if ndim != len(pos_columns):
        raise ValueError("%d position columns for %d-dimensional frames" % (len(pos_columns), ndim))
    diameter = validate_tuple(diameter, ndim)
    radius = tuple(int(x) // 2 for x in diameter)
    isotropic = is_isotropic(diameter)
    ff = training_param_mode(fit_function, ndim, isotropic, param_mode, pos_columns)   # raises first
    bounds = training_bounds(bounds, ff.size_columns)
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
    f['_train_frame'] = np.searchsorted(uniq, frame_vals)

    if refine_com:
        # refine.py:475-489 with the engine's own centre of mass and characterisation
        order = np.argsort(f['_train_frame'].values, kind='stable')
        off = np.searchsorted(f['_train_frame'].values[order], np.arange(len(uniq) + 1)).astype(np.int64)
        pos, _, _ = refine_com_arrays(frames, f[pos_columns].values[order].astype(np.float64), off, radius,
                                      device=device)
        _, signal, size = characterize_arrays(frames, pos, off, radius, isotropic=isotropic, device=device)
        rows = f.index[order]
        f.loc[rows, pos_columns] = pos
        f.loc[rows, 'signal'] = signal
        f.loc[rows, ff.size_columns] = size.reshape(len(order), -1)

    f = find_clusters(f, separation, pos_columns, t_column, labels=cluster_labels, device=device)
    if param_val is not None:
        for col in param_val:
            f[col] = param_val[col]
    for col in ff.params:
        if col not in f.columns:
            f[col] = ff.default[col]

    # groupby([frame, cluster]) order, as prepare_batch
    order = np.lexsort((f['cluster'].values, f['_train_frame'].values))
    fr_s, cl_s = f['_train_frame'].values[order], f['cluster'].values[order]
    new = np.ones(len(order), dtype=bool)
    new[1:] = (fr_s[1:] != fr_s[:-1]) | (cl_s[1:] != cl_s[:-1])
    starts = np.flatnonzero(new)
    feat_offset = np.append(starts, len(order)).astype(np.int32)
    frame_index = fr_s[starts].astype(np.int32)
    if per_frame:
        problem_offset = np.searchsorted(frame_index, np.arange(len(uniq) + 1)).astype(np.int32)
    else:
        problem_offset = np.array([0, len(starts)], dtype=np.int32)
    params = f[ff.params].values.astype(np.float64)[order]

    res = train_arrays(frames, params, feat_offset, frame_index, problem_offset, diameter, fit_function,
                       param_mode={p: ('global' if m == _abi.MODE_GLOBAL else 'const')
                                   for p, m in zip(ff.params, ff.modes)},
                       bounds=bounds, max_rms_dev=max_rms_dev, residual_factor=residual_factor,
                       solver_maxiter=int(options.get('maxiter', 100)), xtol=xtol, ftol=ftol,
                       check_every=check_every, device=device)
    failed = np.flatnonzero(res.status != _abi.STATUS_OK)
    if len(failed):
        p = int(failed[0])
        where = (" (frame %s)" % uniq[p]) if per_frame else ""
        raise RefineException("training failed%s: %s" % (where, _abi.STATUS_TEXT.get(int(res.status[p]),
                                                                                    'status %d' % res.status[p])))
    names = [p for p, m in zip(ff.params, ff.modes) if m == _abi.MODE_GLOBAL]
    if per_frame:
        return pd.DataFrame(res.globals, index=pd.Index(uniq, name=t_column), columns=names)
    return {p: float(res.globals[0, v]) for v, p in enumerate(names)}
