"""Drift of a linked video on the MI355X: compute it, subtract it, drop the stubs.  The step between
``find_link`` / ``link_arrays`` and the cluster tracks and motion analysis: ``motion.diffusion_tensor``
is a second moment, not a covariance, so a stage drift of ``v`` px per frame adds
``v**2 * lag**2 / (2 dt)`` to its translational entries.

The rule is this project's dense restatement of trackpy's published ``compute_drift``,
``subtract_drift`` and ``filter_stubs`` (``include/ctrefine.h`` has it in full):

1. row ``i`` of frame ``t >= 1`` and row ``j`` of frame ``t - 1`` form a *pair* of frame ``t`` when
   ``particle[i] == particle[j] >= 0``; of several such rows ``j`` the lowest;
2. ``n_pairs[t]`` counts the pairs of frame ``t`` and ``dx[t]`` is the mean of ``pos[i] - pos[j]`` over them;
3. ``smoothing = s``: 0 and 1 mean none (``sm = dx`` where there is a pair, else 0), otherwise
   ``sm[t]`` is the mean of ``dx[u]`` over the frames ``u`` in ``[max(1, t - s + 1), t]`` that have a pair;
4. ``drift[0] = 0`` and ``drift[t] = drift[t - 1] + sm[t]``;
5. ``pos_out[i] = pos[i] - drift[frame of i]``;
6. a row whose particle has fewer than ``threshold`` rows gets particle -1; no row is removed and
   no id renumbered in the array form, so the result goes straight into 1 and into
   ``cluster_tracks_arrays``, which ignore negative ids.

Where this differs from trackpy: its drift table has no row for the first frame and none for a
frame without pairs, its ``subtract_drift`` leaves the rows of such frames unshifted, and its
rolling window counts table rows, not frames.  Here the drift is carried forward through a frame
without pairs, and ``n_pairs`` says which frames those are.  On a table where every frame
``t >= 1`` has a pair the values of the frames ``t >= 1`` are trackpy's.  Parity with trackpy itself
is not pinned by a test: it is not a dependency.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import collections

import numpy as np

from . import _abi, _tables

Drift = collections.namedtuple('Drift', ['drift', 'n_pairs', 'status'])
Stubs = collections.namedtuple('Stubs', ['particle', 'count'])

_REFUSED = "frame_offset must rise within [0, N] and particle must be below n_particles"


def compute_drift_arrays(pos, frame_offset, particle, smoothing=0, n_particles=None, device=0):
    """The drift of every frame (``ctr_drift_device``; clauses 1 to 4 of the module's rule).

    pos float64 ``[N, ndim]``, ndim 2 or 3; frame_offset int64 ``[T + 1]``, rows ``[off[t], off[t + 1])``
    are frame t; particle int64 ``[N]``, dense ids ``0 .. P - 1``, negative = unlinked: what
    ``find_link_arrays`` / ``link_arrays`` return, as ndarrays or as tensors on ``cuda:device``.
    n_particles: P; default ``particle.max() + 1``, which for a tensor is one host read
    (``find_link_arrays`` returns it as ``n_tracks``); with tensors and a given P there is no host
    copy and no synchronisation.  Returns ``Drift(drift float64 [T, ndim], n_pairs int32 [T], status)``:
    ndarrays and an int for ndarrays, tensors (status: int32 ``[1]``) for a tensor ``pos``.  A refused
    table (offsets not monotone within N, a particle >= P) raises ``ValueError`` for ndarrays; for
    tensors status is ``_abi.DRIFT_BAD_TABLE``, drift NaN and n_pairs 0.  Unlike trackpy's table the
    result has a row for frame 0 (zero) and for a frame without pairs (the drift carried forward,
    ``n_pairs == 0``).  The same bytes on every call."""
    smoothing = _tables.integer(smoothing, 0, 'smoothing')
    pos, n, ndim = _tables.positions(pos)
    as_tensor = _tables.is_tensor(pos)
    frame_offset, n_frames = _tables.offsets(frame_offset)
    particle, n_particles = _tables.particles(particle, n, n_particles)
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        par_t = _tables.on_device(particle, dev, torch.int64, 'particle')
        if n_particles is None:
            n_particles = _tables.count_particles(par_t, n)
        drift = torch.empty((n_frames, ndim), dtype=torch.float64, device=dev)
        n_pairs = torch.empty(n_frames, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        d = _abi.Drift()
        d.ndim, d.smoothing, d.n_frames, d.n_features, d.n_particles = ndim, smoothing, n_frames, n, n_particles
        d.pos, d.frame_offset, d.particle = pos_t.data_ptr() or None, off_t.data_ptr(), par_t.data_ptr() or None
        d.drift, d.n_pairs, d.status = drift.data_ptr() or None, n_pairs.data_ptr() or None, status.data_ptr()
        eng.on_current_stream(eng.drift_device, d, dev=dev)
        out = _tables.results(as_tensor, status, _abi.DRIFT_OK, "compute_drift_arrays: " + _REFUSED, drift, n_pairs)
        return Drift(*out, status if as_tensor else _abi.DRIFT_OK)


def subtract_drift_arrays(pos, frame_offset, drift, device=0):
    """``pos[i] - drift[frame of i]`` (``ctr_drift_subtract_device``): one subtraction per coordinate,
    so NumPy's bytes for the same ``drift``.

    pos float64 ``[N, ndim]``, frame_offset int64 ``[T + 1]``, drift float64 ``[T, ndim]`` (what
    :func:`compute_drift_arrays` returns).  A row in no frame is copied.  Returns a new table: an
    ndarray for an ndarray ``pos``, a tensor on ``cuda:device`` (no host copy, no synchronisation)
    for a tensor.  Refused offsets raise ``ValueError`` for ndarrays and give NaN for tensors.  Unlike
    trackpy's ``subtract_drift`` every frame is shifted, frame 0 (by zero) and a frame without pairs
    (by the drift carried forward) included."""
    pos, n, ndim = _tables.positions(pos)
    as_tensor = _tables.is_tensor(pos)
    frame_offset, n_frames = _tables.offsets(frame_offset)
    drift, n_drift, ndim_drift = _tables.positions(drift, 'drift')
    if (n_drift, ndim_drift) != (n_frames, ndim):
        raise ValueError("drift must be [T, ndim] = [%d, %d], not [%d, %d]" % (n_frames, ndim, n_drift, ndim_drift))
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        drift_t = _tables.on_device(drift, dev, torch.float64, 'drift')
        out = torch.empty((n, ndim), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        d = _abi.DriftSubtract()
        d.ndim, d.n_frames, d.n_features = ndim, n_frames, n
        d.pos, d.frame_offset, d.drift = pos_t.data_ptr() or None, off_t.data_ptr(), drift_t.data_ptr() or None
        d.pos_out, d.status = out.data_ptr() or None, status.data_ptr()
        eng.on_current_stream(eng.drift_subtract_device, d, dev=dev)
        return _tables.results(as_tensor, status, _abi.DRIFT_OK,
                               "subtract_drift_arrays: frame_offset must rise within [0, N]", out)[0]


def filter_stubs_arrays(particle, threshold=100, n_particles=None, device=0):
    """Unlink the rows of short tracks (``ctr_filter_stubs_device``; clause 6 of the module's rule).

    particle int64 ``[N]``, dense ids ``0 .. P - 1``, negative = unlinked; n_particles as in
    :func:`compute_drift_arrays`.  Returns ``Stubs(particle int64 [N], count int32 [P])``: ``count[p]``
    the rows of particle p, and a row keeps its id where ``count >= threshold``, else -1.  Rows are
    not removed and ids not renumbered (trackpy's ``filter_stubs`` drops the rows; :func:`filter_stubs`
    does that for a table).  ndarrays for an ndarray, tensors (no host copy, no synchronisation with
    a given P) for a tensor.  A particle >= P raises ``ValueError`` for ndarrays; for tensors every row
    then gets -1 and every count is 0."""
    threshold = _tables.integer(threshold, 1, 'threshold')
    as_tensor = _tables.is_tensor(particle)
    particle, n_particles = _tables.particles(particle, None, n_particles)
    n = int(particle.shape[0])
    with _tables.stage(device) as (eng, dev):
        import torch
        par_t = _tables.on_device(particle, dev, torch.int64, 'particle')
        if n_particles is None:
            n_particles = _tables.count_particles(par_t, n)
        out = torch.empty(n, dtype=torch.int64, device=dev)
        count = torch.empty(n_particles, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        d = _abi.FilterStubs()
        d.threshold, d.n_features, d.n_particles = threshold, n, n_particles
        d.particle, d.particle_out = par_t.data_ptr() or None, out.data_ptr() or None
        d.count, d.status = count.data_ptr() or None, status.data_ptr()
        eng.on_current_stream(eng.filter_stubs_device, d, dev=dev)
        return Stubs(*_tables.results(as_tensor, status, _abi.DRIFT_OK,
                                      "filter_stubs_arrays: particle must be below n_particles", out, count))


def compute_drift(f, smoothing=0, pos_columns=None, t_column='frame', device=0):
    """The drift of a linked table: a DataFrame indexed by every frame from ``f[t_column].min()`` to
    its maximum, with the position columns and ``n_pairs``.

    f: a DataFrame with a ``particle`` column (ids of any integer type: they are mapped through their
    sorted unique values, so every id is a particle).  Unlike trackpy's ``compute_drift`` the result
    has a row for the first frame (zero) and for a frame without pairs (``n_pairs == 0``, the drift
    carried forward), and ``smoothing`` counts frames, not table rows; see the module's text."""
    import pandas as pd
    smoothing = _tables.integer(smoothing, 0, 'smoothing')
    _, offset, first, ids, dense, pos_columns, pos = _tables.frame_sorted(f, pos_columns, t_column)
    res = compute_drift_arrays(pos, offset, dense, smoothing, n_particles=len(ids), device=device)
    out = pd.DataFrame(res.drift, columns=pos_columns,
                       index=pd.RangeIndex(first, first + len(res.drift), name=t_column))
    out['n_pairs'] = res.n_pairs
    return out


def subtract_drift(f, drift=None, smoothing=0, pos_columns=None, t_column='frame', device=0):
    """A copy of ``f`` with the drift of its frame subtracted from the position columns.

    drift: what :func:`compute_drift` returns (a DataFrame indexed by frame that covers every frame
    of ``f``, with the position columns); None computes it from ``f`` with ``smoothing``.  Unlike
    trackpy's ``subtract_drift`` no frame stays unshifted."""
    if drift is None:
        drift = compute_drift(f, smoothing, pos_columns, t_column, device)
    order, offset, first, _, _, pos_columns, pos = _tables.frame_sorted(f, pos_columns, t_column)
    if [c for c in pos_columns if c not in drift]:
        raise ValueError("the drift table has no columns %r" % (pos_columns,))
    frames = np.arange(first, first + len(offset) - 1)
    per_frame = drift[pos_columns].reindex(frames)
    occupied = np.diff(offset) > 0
    if per_frame[occupied].isna().values.any():
        raise ValueError("the drift table does not cover every frame of the table")
    shifted = subtract_drift_arrays(pos, offset, per_frame.fillna(0.).values, device)
    values = np.empty_like(shifted)
    values[order] = shifted
    out = f.copy()
    for k, col in enumerate(pos_columns):
        out[col] = values[:, k]
    return out


def filter_stubs(f, threshold=100, t_column='frame', device=0):
    """The rows of ``f`` whose particle has at least ``threshold`` rows, as trackpy's ``filter_stubs``.
    Particle ids of any integer type (mapped through their sorted unique values)."""
    threshold = _tables.integer(threshold, 1, 'threshold')
    _, _, _, ids, dense, _, _ = _tables.frame_sorted(f, None, t_column, with_pos=False)
    # dense follows the sorted rows; the count of a particle does not depend on the order
    res = filter_stubs_arrays(dense, threshold, n_particles=len(ids), device=device)
    keep = res.count[np.searchsorted(ids, f['particle'].values)] >= threshold
    return f[keep].copy()
