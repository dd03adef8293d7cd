"""``refine_leastsq`` -- drop-in for reference ``clustertracking/refine.py:82-452``.

The host side keeps what the reference does before and after its per-cluster
loop (option / reader normalisation refine.py:242-289, cluster labelling :297,
parameter columns :299-305, bounds templates :315, and the DataFrame output
:419-430), vectorised.  The loop itself (refine.py:343-430: windows, masks,
objective, minimiser, re-window rounds, failure rules) is ONE batched call into
the HIP engine through the C-ABI of ``include/ctrefine.h``.
"""
import collections
import logging

import numpy as np

from . import _abi
from ._tables import is_tensor
from .constraints import engine_constraint
from .find import find_clusters
from .fitfunc import FitFunctions
from .utils import (ArrayReader, guess_pos_columns, is_isotropic,
                    validate_tuple)

logger = logging.getLogger(__name__)


class PreparedBatch(object):
    """Everything one engine call needs, plus how to scatter results back."""

    def __init__(self, f, ff, problem, batch, order, cluster_of_row):
        self.f = f                    # clustered copy of the input (output frame)
        self.ff = ff
        self.problem = problem
        self.batch = batch            # _abi.HostBatch
        self.order = order            # row positions of f in batch feature order
        self.cluster_of_row = cluster_of_row  # batch cluster index per batch feature


def _normalise_reader(f, reader, t_column):
    """refine.py:251-281.  Returns (get_frame, ndim, is_sequence)."""
    try:
        ndim = len(reader.frame_shape)
        return reader, ndim, True
    except AttributeError:
        pass
    try:
        ndim = reader.ndim
    except AttributeError:
        raise ValueError('For multiple frames, the reader should be a'
                         'FramesSequence object exposing the "frame_shape"'
                         'attribute')
    frame_no = getattr(reader, 'frame_no', None)
    if frame_no is not None:
        frame_no = int(frame_no)
    if frame_no is not None and t_column in f:
        assert np.all(f[t_column] == frame_no)
    elif frame_no is not None:
        f[t_column] = frame_no
    elif t_column in f:
        assert f[t_column].nunique() == 1
        frame_no = int(f[t_column].iloc[0])
    else:
        f[t_column] = 0
        frame_no = 0
    return {frame_no: reader}, ndim, False


def _check_options(ndim, diameter, separation, fit_function, param_mode, constraints, max_iter):
    """What ``prepare_batch`` and ``refine_arrays`` refuse before any work, and the model they agree
    on: ``(diameter, radius, isotropic, separation, ff, cons)``."""
    if int(max_iter) < 1:
        raise ValueError("max_iter must be at least 1")

    diameter = validate_tuple(diameter, ndim)
    radius = tuple([x // 2 for x in diameter])
    isotropic = is_isotropic(diameter)
    if separation is None:
        separation = diameter

    ff = FitFunctions(fit_function, ndim, isotropic, param_mode)
    modes = np.array(ff.modes)
    if np.any(modes == 2):
        raise NotImplementedError(
            "param_mode 'global' couples all features into one problem "
            "(reference refine.py:319-332) and is not supported by the MI355X "
            "engine; train_leastsq fits shared parameters with everything else constant"
            "; ct.refine_global fits them together with per-feature and per-cluster parameters")
    if not np.all(modes <= 3):
        raise NotImplementedError("param modes 'particle'/'frame' are not "
                                  "implemented (reference refine.py:339-340)")
    cons = engine_constraint(constraints, ndim)
    return diameter, radius, isotropic, separation, ff, cons


def prepare_batch(f, reader, diameter, separation=None, fit_function='gauss',
                  param_mode=None, param_val=None, constraints=None, bounds=None,
                  pos_columns=None, t_column='frame', max_iter=10, max_shift=1,
                  max_rms_dev=1., residual_factor=100000., solver_maxiter=100,
                  xtol=0., ftol=0., cluster_labels='reference', device=0,
                  compute_error=False, noise_size=None, threshold=None):
    """Host-side set-up of one refine call (reference refine.py:242-341)."""
    if pos_columns is None:
        pos_columns = guess_pos_columns(f)
    frames_src, ndim, _ = _normalise_reader(f, reader, t_column)
    assert ndim == len(pos_columns)
    diameter, radius, isotropic, separation, ff, cons = _check_options(
        ndim, diameter, separation, fit_function, param_mode, constraints, max_iter)
    f = find_clusters(f, separation, pos_columns, t_column, labels=cluster_labels,
                      device=device)  # makes a copy
    if param_val is not None:
        for col in param_val:
            f[col] = param_val[col]
    for col in ff.params:
        if col not in f.columns:
            f[col] = ff.default[col]

    templates = ff.validate_bounds(bounds, radius=radius)
    params = f[ff.params].values.astype(np.float64)
    low, high = ff.feature_bounds(templates, params)

    # groupby([t_column, 'cluster']) order, rows keep their order inside a group
    frame_vals = f[t_column].values
    cluster_vals = f['cluster'].values
    if len(frame_vals) and np.issubdtype(frame_vals.dtype, np.integer) and \
            np.issubdtype(cluster_vals.dtype, np.integer) and frame_vals.min() >= 0 and cluster_vals.min() >= 0 \
            and (int(frame_vals.max()) + 1) * (int(cluster_vals.max()) + 1) < 2 ** 62:
        # one stable sort of a combined key (the same order as lexsort, at half its cost)
        key = frame_vals.astype(np.int64) * (int(cluster_vals.max()) + 1) + cluster_vals
        order = np.argsort(key, kind='stable')
    else:
        order = np.lexsort((cluster_vals, frame_vals))
    fr_s, cl_s = frame_vals[order], cluster_vals[order]
    n_rows = len(order)
    new = np.ones(n_rows, dtype=bool)
    new[1:] = (fr_s[1:] != fr_s[:-1]) | (cl_s[1:] != cl_s[:-1])
    starts = np.flatnonzero(new)
    feat_offset = np.append(starts, n_rows).astype(np.int32)
    cluster_of_row = np.cumsum(new) - 1
    cl_frames = fr_s[starts]

    # frames block
    if isinstance(frames_src, ArrayReader):
        frames = frames_src.array
        frame_index = cl_frames.astype(np.int64)
        if len(frame_index) and (frame_index.min() < 0 or frame_index.max() >= len(frames)):
            raise IndexError("frame number outside of the video")
    else:
        uniq, inv = np.unique(cl_frames, return_inverse=True)
        if len(uniq):
            frames = np.stack([np.asarray(frames_src[int(i)]) for i in uniq])
        else:
            frames = np.zeros((0,) + (1,) * ndim, dtype=np.uint8)
        frame_index = inv
    if frames.ndim != ndim + 1:
        raise ValueError("frames must have %d dimensions" % ndim)

    problem = _abi.make_problem(ndim, isotropic, ff.modes, radius, cons,
                                max_iter=max_iter, max_shift=max_shift,
                                max_rms_dev=max_rms_dev,
                                residual_factor=residual_factor,
                                solver_maxiter=solver_maxiter, xtol=xtol, ftol=ftol,
                                noise_size=None if noise_size is None else validate_tuple(noise_size, ndim),
                                threshold=threshold, fit_function=ff.fit_function)
    batch = _abi.HostBatch(frames, frame_index, feat_offset, params[order],
                           low[order], high[order], want_std=bool(compute_error))
    # SciPy raises ValueError for an infeasible box (lower > upper)
    n_per = np.diff(feat_offset)
    if n_rows:
        for k, m in enumerate(ff.modes):
            if m == 0:
                continue
            lo_k, hi_k = batch.low[:, k], batch.high[:, k]
            if m != 1:  # shared: loosest bound over the cluster (fitfunc.py:554-557)
                lo_k = np.minimum.reduceat(lo_k, starts)
                hi_k = np.maximum.reduceat(hi_k, starts)
            if np.any(lo_k > hi_k):
                raise ValueError("SLSQP Error: the lower bound exceeds the "
                                 "upper bound (parameter %r)" % ff.params[k])
    return PreparedBatch(f, ff, problem, batch, order, cluster_of_row)


def write_back(prep):
    """Vectorised equivalent of refine.py:408-430."""
    f, ff, batch = prep.f, prep.ff, prep.batch
    n_rows = len(prep.order)
    out = np.empty((n_rows, len(ff.params)), dtype=np.float64)
    out[prep.order] = batch.params_out
    cost = np.empty(n_rows, dtype=np.float64)
    cost[prep.order] = batch.cost[prep.cluster_of_row]
    for k, col in enumerate(ff.params):
        f[col] = out[:, k]
    f['cost'] = cost
    if batch.params_std is not None:      # refine.py:307-312,423-429: '<param>_std' of the fitted ones
        std = np.empty((n_rows, len(ff.params)), dtype=np.float64)
        std[prep.order] = batch.params_std
        for k, col in enumerate(ff.params):
            if ff.modes[k] > 0:
                f[col + '_std'] = std[:, k]
    failed = np.flatnonzero(batch.status != _abi.STATUS_OK)
    for c in failed:
        logger.warning('RefineException: ' + _abi.STATUS_TEXT.get(
            int(batch.status[c]), 'status %d' % batch.status[c]))
    return f


def _run_on_engine(problem, batch, device=0):
    from . import _lib
    return _lib.default_engine(device).refine_batch(problem, batch)


def refine_leastsq(f, reader, diameter, separation=None, fit_function='gauss',
                   param_mode=None, param_val=None, constraints=None,
                   bounds=None, pos_columns=None, t_column='frame',
                   noise_size=None, threshold=None, max_iter=10, max_shift=1,
                   max_rms_dev=1., residual_factor=100000.,
                   compute_error=False, **kwargs):
    """Refines cluster coordinates by least-squares fitting to radial model
    functions, on the MI355X engine.

    Signature, defaults, side effects and output columns follow reference
    ``refine_leastsq`` (refine.py:82-241); see there for the parameters.  This
    does not raise an error if minimization fails: coordinates are unchanged
    and the added column ``cost`` is NaN for that cluster.

    Differences, all deliberate:

    * The minimiser is the engine's bounded Levenberg-Marquardt, run to
      convergence, not SciPy SLSQP at ``tol=1e-6``: ``method`` and ``tol`` in
      ``kwargs`` are accepted and ignored; ``options['maxiter']`` (default 100)
      caps the solver iterations per re-window round.  Engine-specific keys:
      ``xtol``, ``ftol``, ``device``, ``cluster_labels`` ('reference': ids equal to
      the reference's, labelled on the host; 'device': same partition labelled on
      the GPU, canonical ids).
    * ``fit_function``: ``'gauss'``, ``'ring'``, ``'disc'`` and ``'inv_series_<N>'`` (fitfunc.py:112-154,
      with the profile parameters ``thickness`` / ``disc_size`` / ``signal_mult, param_a, ...`` as
      columns like any other: constant by default, ``param_val`` sets them); custom (dict)
      functions and the ``param_mode`` value ``'global'`` raise ``NotImplementedError`` (there is no
      CPU fallback to hand them to).  Fits of the other profiles iterate with the Gauss-Newton
      model, have no ``compute_error`` (NaN) and are limited to clusters of 64 features / 127
      variables and to 12 parameter columns.
    * ``noise_size`` (the lowpass of every window, refine.py:37-40) up to sigma 4.
    * ``compute_error``: the ``'<param>_std'`` columns come from the exact second
      derivatives of the objective (the reference differentiates numerically with
      numdifftools), for every ``param_mode``; clusters of more than 64 features or 127
      variables (the large-cluster kernel) get NaN there.
    * A cluster whose coordinates are all outside the frame, or that has
      non-finite parameters, gets ``cost = NaN`` (the reference means to do
      that, but crashes with IndexError at refine.py:417).
    """
    options = dict(maxiter=100)
    options.update(kwargs.pop('options', None) or {})
    kwargs.pop('method', None)
    kwargs.pop('tol', None)
    xtol = kwargs.pop('xtol', 0.)
    ftol = kwargs.pop('ftol', 0.)
    device = kwargs.pop('device', 0)
    cluster_labels = kwargs.pop('cluster_labels', 'reference')
    if kwargs:
        raise TypeError("unexpected keyword arguments: %s" % sorted(kwargs))
    prep = prepare_batch(f, reader, diameter, separation, fit_function,
                         param_mode, param_val, constraints, bounds,
                         pos_columns, t_column, max_iter, max_shift,
                         max_rms_dev, residual_factor,
                         solver_maxiter=int(options.get('maxiter', 100)),
                         xtol=xtol, ftol=ftol, cluster_labels=cluster_labels, device=device,
                         compute_error=compute_error, noise_size=noise_size, threshold=threshold)
    if prep.batch.n_clusters:
        _run_on_engine(prep.problem, prep.batch, device)
    return write_back(prep)


RefineResult = collections.namedtuple(
    'RefineResult', 'params columns cost cluster cluster_size params_std status n_rounds n_iter feat_offset')


def _check_tables(frames, pos, frame_offset):
    """The shapes ``refine_arrays`` refuses before any device work: ``(ndim, n_rows, n_frames)``.
    The offsets of an ndarray are checked here, those of a tensor by the stage's first kernel."""
    ndim = len(frames.shape) - 1
    if ndim not in (2, 3):
        raise ValueError("frames must be [T, (z,) y, x], not an array of %d dimensions" % len(frames.shape))
    if len(pos.shape) != 2 or pos.shape[1] != ndim:
        raise ValueError("pos must be [N, %d], not %s" % (ndim, tuple(pos.shape)))
    n, n_frames = int(pos.shape[0]), int(frames.shape[0])
    if n >= 2 ** 31 - 1:
        raise ValueError("%d rows: one call takes fewer than 2**31 - 1" % n)
    if len(frame_offset.shape) != 1 or frame_offset.shape[0] != n_frames + 1:
        raise ValueError("frame_offset must have one entry per frame and one more (%d), not %s"
                         % (n_frames + 1, tuple(frame_offset.shape)))
    if not is_tensor(frame_offset):
        if frame_offset.dtype.kind not in 'iu':
            raise ValueError("frame_offset must hold integers, not %s" % frame_offset.dtype)
        if frame_offset[0] != 0 or frame_offset[-1] != n or np.any(np.diff(frame_offset.astype(np.int64)) < 0):
            raise ValueError("frame_offset must not decrease, from 0 to the number of rows (%d)" % n)
    return ndim, n, n_frames


def _start_values(ff, pos_t, columns, n, dev):
    """``params0`` [N, n_params] on the device from the start columns (scalars, ndarrays, tensors):
    a handful of column copies."""
    import torch
    cols = []
    for name in ff.params:
        if name in ff.pos_columns:
            cols.append(pos_t[:, ff.pos_columns.index(name)])
            continue
        v = columns[name]
        if is_tensor(v):
            if v.device != dev:
                raise ValueError("the %r tensor must be on %s" % (name, dev))
            v = v.to(torch.float64)
        else:
            v = torch.from_numpy(np.array(v, dtype=np.float64)).to(dev)
        if v.dim() == 0:
            v = v.expand(n)
        if v.dim() != 1 or v.shape[0] != n:
            raise ValueError("%r must be a scalar or have one value per row (%d), not %s" % (name, n, tuple(v.shape)))
        cols.append(v)
    return torch.stack(cols, dim=1).contiguous()


def _prepare_on_device(eng, dev, pos_t, off_t, params0, separation, ff, templates):
    """Queue ``ctr_refine_prepare_device`` (CTR_PREPARE_BATCH) on torch's current stream; no
    synchronisation.  Returns the descriptor and the tensors it names: ``head`` int32 ``[4 + N + 1]``
    holds ``n_clusters``, ``status[2]``, a pad and ``feat_offset``, so that one copy brings all of
    them to the host; then label, cluster_size, order, frame_index ``[N]`` and params, low, high."""
    import torch
    n, np_, ndim = int(pos_t.shape[0]), ff.n_params, int(pos_t.shape[1])
    head = torch.empty(4 + n + 1, dtype=torch.int32, device=dev)
    label, csize, order, frame_index = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    params, low, high = (torch.empty((n, np_), dtype=torch.float64, device=dev) for _ in range(3))
    d = _abi.RefinePrepare()
    d.mode, d.ndim, d.n_params, d.n_frames, d.n_features = _abi.PREPARE_BATCH, ndim, np_, int(off_t.shape[0]) - 1, n
    for k, m in enumerate(ff.modes):
        d.modes[k] = int(m)
    for a in range(ndim):
        d.separation[a] = float(separation[a])
    for field, tmpl in zip(('bound_abs', 'bound_diff', 'bound_rel'), templates):
        arr = getattr(d, field)
        for row in range(2):
            for k in range(_abi.MAX_PARAMS):
                arr[row * _abi.MAX_PARAMS + k] = float(tmpl[row][k]) if k < np_ else np.nan
    d.pos, d.frame_offset, d.params0 = pos_t.data_ptr() or None, off_t.data_ptr(), params0.data_ptr() or None
    d.label, d.cluster_size, d.order = label.data_ptr() or None, csize.data_ptr() or None, order.data_ptr() or None
    d.frame_index = frame_index.data_ptr() or None
    d.n_clusters_out, d.status, d.feat_offset = head.data_ptr(), head[1:].data_ptr(), head[4:].data_ptr()
    d.params, d.low, d.high = params.data_ptr() or None, low.data_ptr() or None, high.data_ptr() or None
    eng.on_current_stream(eng.refine_prepare_device, d, dev=dev)
    return d, head, label, csize, order, frame_index, params, low, high


PreparedArrays = collections.namedtuple(
    'PreparedArrays', 'label cluster_size order feat_offset frame_index params low high n_clusters status')


def prepare_arrays(pos, frame_offset, params0, separation, ff, bounds=None, radius=None, device=0):
    """The prepare stage of :func:`refine_arrays` alone (``ctr_refine_prepare_device``): pos float64
    ``[N, ndim]`` in frame order, frame_offset int64 ``[T + 1]``, params0 float64 ``[N, n_params]`` in
    the column order of ``ff`` (a ``FitFunctions``), ndarrays or tensors on ``cuda:device``; bounds
    and radius as ``FitFunctions.validate_bounds`` takes them.  Returns ``PreparedArrays`` of
    tensors on the device -- label, cluster_size, order int32 ``[N]``, feat_offset int32 ``[C + 1]``,
    frame_index int32 ``[C]``, params, low, high ``[N, n_params]`` in grouped
    order -- and the ints ``n_clusters`` and ``status = (code, parameter)``: ``_abi.PREPARE_OK``,
    ``PREPARE_BAD_TABLE`` (offsets that do not rise from 0 to N) or ``PREPARE_INFEASIBLE`` with the
    index of the parameter.  One synchronisation, at the end."""
    from . import _lib
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    dev = torch.device('cuda', device)
    templates = ff.validate_bounds(bounds, radius=radius)
    with torch.cuda.device(dev):
        pos_t, off_t, par_t = (x if is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=t)).to(dev)
                               for x, t in ((pos, np.float64), (frame_offset, np.int64), (params0, np.float64)))
        if pos_t.dim() != 2 or pos_t.shape[1] not in (2, 3) or tuple(par_t.shape) != (pos_t.shape[0], ff.n_params):
            raise ValueError("pos must be [N, ndim] and params0 [N, %d]" % ff.n_params)
        separation = validate_tuple(separation, int(pos_t.shape[1]))
        _, head, label, csize, order, frame_index, params, low, high = _prepare_on_device(
            eng, dev, pos_t.contiguous(), off_t.contiguous(), par_t.contiguous(), separation, ff, templates)
        n_clusters, code, bad = (int(v) for v in head[:3].cpu())
        return PreparedArrays(label, csize, order, head[4:4 + n_clusters + 1], frame_index[:n_clusters], params, low,
                              high, n_clusters, (code, bad))


def refine_arrays(frames, pos, frame_offset, diameter, separation=None, signal=None, size=None,
                  background=0., fit_function='gauss', param_mode=None, param_val=None,
                  constraints=None, bounds=None, noise_size=None, threshold=None, max_iter=10,
                  max_shift=1, max_rms_dev=1., residual_factor=100000., compute_error=False,
                  options=None, xtol=0., ftol=0., device=0):
    """:func:`refine_leastsq` on arrays: tensors in, tensors on the device out; NumPy in, NumPy out.

    frames ``[T, (z,) y, x]``; pos float64 ``[N, ndim]``, rows sorted by frame; frame_offset
    ``[T + 1]`` integers, rows ``[off[t], off[t + 1])`` are frame t -- what ``locate_arrays`` and
    ``find_link_arrays`` return; ndarrays, or tensors on ``cuda:device``.  signal: a scalar or
    ``[N]``; size: a scalar, ``[N]`` or, for an anisotropic ``diameter``, ``[N, ndim]``; background as
    signal; param_val: further columns of ``FitFunctions.params`` (scalars or ``[N]``), which also
    override the three.  Everything else as :func:`refine_leastsq`, with ``cluster_labels='device'``:
    the same kernels on the same batch, so the same bytes.

    Returns ``RefineResult(params [N, n_params] and cost [N] in input row order, columns =
    ff.params, cluster and cluster_size int64 [N] (the smallest row of the row's cluster, as
    find_clusters(labels='device')), params_std ([N, n_params], NaN where a column is not fitted) or
    None, status, n_rounds, n_iter int32 [C] per cluster in batch order, feat_offset int32 [C + 1])``.
    A failed cluster keeps its parameters and has ``cost`` NaN and a non-zero ``status``
    (``_abi.STATUS_TEXT``); no warning is logged.

    The batch is grouped, bounded and laid out on the device (``ctr_refine_prepare_device``) on
    torch's current stream.  There is ONE synchronisation with the host, after that stage: the words
    ``n_clusters`` and ``status`` and the clusters' row ranges come over in one copy of 4 (N + 5)
    bytes, of which the C + 1 offsets are used, because ``ctr_plan_create`` bins the clusters on the
    host and sizes the grids from them.  Frames, positions and parameter tables given as tensors never
    cross PCIe.  The plan (and the large clusters' workspace in it) lives for the call: the stream is
    synchronised once more before it is destroyed, so the results are complete on return.

    Raises, before any device work: ``NotImplementedError`` for ``param_mode`` 'global', dict fit
    functions and more than one constraint; ``ValueError`` for ``max_iter < 1``, frames that are not
    ``[T, (z,) y, x]``, a ``pos`` that is not ``[N, ndim]``, ``N >= 2**31 - 1`` and a ``frame_offset``
    ndarray that decreases or does not run from 0 to N (a tensor's offsets are checked by the stage's
    first kernel and refused at the synchronisation).  ``ValueError("SLSQP Error: ...")`` for a lower
    bound above its upper bound, as ``prepare_batch``.  ``EngineError`` without a library or a GPU."""
    as_tensor = is_tensor(pos)
    if not hasattr(frames, 'shape'):
        frames = np.asarray(frames)
    if not as_tensor:
        pos = np.asarray(pos)
    if not is_tensor(frame_offset):
        frame_offset = np.asarray(frame_offset)
    ndim, n, n_frames = _check_tables(frames, pos, frame_offset)
    diameter, radius, isotropic, separation, ff, cons = _check_options(
        ndim, diameter, separation, fit_function, param_mode, constraints, max_iter)
    separation = validate_tuple(separation, ndim)
    if not all(float(s) > 0 and np.isfinite(float(s)) for s in separation):
        raise ValueError("separation must be positive")
    solver_maxiter = int(dict(options or {}).get('maxiter', 100))
    problem = _abi.make_problem(ndim, isotropic, ff.modes, radius, cons, max_iter=max_iter, max_shift=max_shift,
                                max_rms_dev=max_rms_dev, residual_factor=residual_factor,
                                solver_maxiter=solver_maxiter, xtol=xtol, ftol=ftol,
                                noise_size=None if noise_size is None else validate_tuple(noise_size, ndim),
                                threshold=threshold, fit_function=ff.fit_function)
    templates = ff.validate_bounds(bounds, radius=radius)
    columns = dict(background=background)
    if signal is not None:
        columns['signal'] = signal
    if size is not None:
        if isotropic:
            columns['size'] = size if len(getattr(size, 'shape', ())) < 2 else size[:, 0]
        else:
            for a, col in enumerate(ff.size_columns):
                columns[col] = size if len(getattr(size, 'shape', ())) < 2 else size[:, a]
    columns.update(param_val or {})
    for col in ff.params:
        if col in ff.default:
            columns.setdefault(col, ff.default[col])
    for col in ff.params:
        if col not in columns and col not in ff.pos_columns:
            raise ValueError("no start value for %r: give it as an argument or in param_val" % col)

    from . import _lib
    from .find import _device_frames
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    if not is_tensor(frames) and frames.dtype not in _abi.DTYPE_CODES:
        frames = frames.astype(np.float64)     # as HostBatch: refine.py:58
    frames_t, pix = _device_frames(frames, device, None)
    dev = frames_t.device
    np_ = ff.n_params
    with torch.cuda.device(dev):
        if as_tensor:
            if pos.device != dev or pos.dtype != torch.float64:
                raise ValueError("a pos tensor is float64 on %s" % dev)
            pos_t = pos.contiguous()
        else:
            pos_t = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float64)).to(dev)
        if is_tensor(frame_offset):
            if frame_offset.device != dev or frame_offset.dtype != torch.int64:
                raise ValueError("a frame_offset tensor is int64 on %s" % dev)
            off_t = frame_offset.contiguous()
        else:
            off_t = torch.from_numpy(np.ascontiguousarray(frame_offset, dtype=np.int64)).to(dev)
        params0 = _start_values(ff, pos_t, columns, n, dev)

        d, head, label, csize, order, frame_index, params, low, high = _prepare_on_device(
            eng, dev, pos_t, off_t, params0, separation, ff, templates)
        head_host = head.cpu().numpy()          # the one synchronisation
        n_clusters, code, bad_param = (int(v) for v in head_host[:3])
        if code == _abi.PREPARE_BAD_TABLE:
            raise ValueError("frame_offset must not decrease, from 0 to the number of rows (%d)" % n)
        if code == _abi.PREPARE_INFEASIBLE:
            raise ValueError("SLSQP Error: the lower bound exceeds the "
                             "upper bound (parameter %r)" % ff.params[bad_param])
        feat_offset = head[4:4 + n_clusters + 1]

        params_out = params0.clone()
        cost = torch.full((n,), np.nan, dtype=torch.float64, device=dev)
        std = torch.full((n, np_), np.nan, dtype=torch.float64, device=dev) if compute_error else None
        cl_status, n_rounds, n_iter = (torch.zeros(n_clusters, dtype=torch.int32, device=dev) for _ in range(3))
        if n_clusters:
            plan = eng.plan(problem, head_host[4:4 + n_clusters + 1])
            try:
                fit = torch.empty((n, np_), dtype=torch.float64, device=dev)
                fit_cost = torch.empty(n_clusters, dtype=torch.float64, device=dev)
                fit_std = torch.empty((n, np_), dtype=torch.float64, device=dev) if compute_error else None
                b = _abi.Batch()
                b.frames, b.frame_dtype, b.n_frames = frames_t.data_ptr(), _abi.DTYPE_CODES[np.dtype(pix)], n_frames
                for a in range(ndim):
                    b.shape[a] = int(frames_t.shape[1 + a])
                b.n_clusters, b.n_features = n_clusters, n
                b.frame_index, b.feat_offset = frame_index.data_ptr(), feat_offset.data_ptr()
                b.params, b.low, b.high = params.data_ptr(), low.data_ptr(), high.data_ptr()
                b.params_out, b.cost, b.status = fit.data_ptr(), fit_cost.data_ptr(), cl_status.data_ptr()
                b.n_rounds, b.n_iter = n_rounds.data_ptr(), n_iter.data_ptr()
                b.params_std = fit_std.data_ptr() if compute_error else None
                eng.on_current_stream(eng.refine_batch_device, plan, b, dev=dev)
                d.mode, d.n_clusters = _abi.PREPARE_SCATTER, n_clusters
                d.fit_params, d.fit_cost = fit.data_ptr(), fit_cost.data_ptr()
                d.fit_std = fit_std.data_ptr() if compute_error else None
                d.params_out, d.cost_out = params_out.data_ptr(), cost.data_ptr()
                d.std_out = std.data_ptr() if compute_error else None
                eng.on_current_stream(eng.refine_prepare_device, d, dev=dev)
                torch.cuda.current_stream(dev).synchronize()     # the plan's tables are in use until here
            finally:
                plan.close()
        res = RefineResult(params_out, list(ff.params), cost, label.to(torch.int64), csize.to(torch.int64), std,
                           cl_status, n_rounds, n_iter, feat_offset.clone())
        if as_tensor:
            return res
        return RefineResult(*(x.cpu().numpy() if is_tensor(x) else x for x in res))
