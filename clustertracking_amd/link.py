"""Frame-to-frame linking of refined coordinates on the host.

BASELINE cfg 4 links the refined coordinates after the GPU refine.  The
reference has no public "link these coordinates" function; its ``Linker`` base
class (reference ``clustertracking/find_link.py:579-733``, the Crocker-Grier
scheme with sub-network resolution, ``:236-376,507-576``) is what this module
restates, vectorised per frame pair:

* candidates: for every feature of the new frame its (up to 10) nearest
  features of the previous frame within ``search_range`` (per-axis scaled
  distance <= 1 + 1e-7), ``find_link.py:259-275``;
* sub-networks: connected components of the candidate graph
  (``find_link.py:320-343``);
* inside a sub-network the set of links minimising ``sum(d^2)`` plus one unit
  per missing link (``SubnetLinker``, ``find_link.py:507-576``); solved here as
  an assignment problem, which has the same optimum as the reference's
  exhaustive recursion;
* unmatched new features start tracks, numbered in lexicographic order of their
  position (``_sort_key_spl_dpl``, ``find_link.py:379-383,701-712``);
* unmatched old features stay candidates for ``memory`` more frames at their
  last position (``find_link.py:594-610,716-732``).

The host path above is the default.  ``engine='device'`` (and :func:`link_arrays`) runs the same
rule on the MI355X (``ctr_link_device``); there is no fallback from it.

The adaptive search range (``adaptive_stop``, ``adaptive_step``; on the device
``ctr_link_adaptive_device``) is this project's dense restatement of trackpy's published
``adaptive_link_wrap``; parity with trackpy is not pinned.  A sub-network beyond the limits does not
end the call: its range alone is shrunk, step by step, until it falls apart into pieces that can be
solved.  All distances are scaled, position divided by ``search_range`` per axis.

* ``stop_rel = max_a(adaptive_stop_a / search_range_a)`` must lie inside (0, 1), ``adaptive_step``
  too.  ``rho_0 = 1`` and ``rho_{k+1} = rho_k * adaptive_step``, one double multiplication; ``K`` is
  the smallest k with ``rho_k <= stop_rel``, found by that same loop, and at most 64.
  ``adaptive_step`` without ``adaptive_stop`` is ignored, as in trackpy.
* round 0: candidates and sub-networks are exactly the plain call's.  A 1 x 1 sub-network links; one
  of at most 30 sources and at most 64 destinations is solved exactly.
* an oversize sub-network at round k (more than 30 sources or more than 64 destinations): if
  ``rho_k <= stop_rel`` the call fails (status ``OVERSIZE`` for the sources, ``CAPACITY`` for the
  destinations; :class:`SubnetOversizeException` for both, naming the level and the size).
  Otherwise its edges are cut to ``rho_{k+1}``: an edge stays iff ``d2 <= b * b`` with
  ``b = rho_{k+1} * (1. + 1e-7)`` and ``d2 = sum_a (dst_a / sr_a - src_a / sr_a) ** 2``, summed in
  axis order with no contraction: the number the device stores for a candidate, not the square of
  the kd-tree's distance.  The connected components of the remaining edges among that sub-network's
  members are the sub-networks of round k + 1.  A destination left without an edge starts a track; a
  source left without an edge is unlinked and goes to memory as any lost source does.
* a sub-network solved at round k maximises ``sum(2 rho_k ** 2 - d ** 2)``: the cost entry is
  ``d2 - 2. * (rho * rho)``, trackpy's penalty for a missing link, the current range squared.
* the limits stay 30 and 64 in adaptive mode, on the host too.  trackpy lowers its own limit to 15
  there because its recursion is exponential; the assignment solver here is not.  So where the plain
  call succeeds, the adaptive call returns the same ids.
* the diagnostic ``adaptive_round`` (int32 per row, ``diag=True``) is the k of the round in which a
  destination row was settled: its sub-network was within the limits at ``rho_k`` (whether or not
  the solver linked the row), or the cut to ``rho_k`` took its last edge.  0 for the rows of level 0
  and for rows without any candidate.

Memory, births and ids are unchanged.

Prediction (``predictor``, ``initial_velocity``; on the device ``ctr_link_predict_device``) links a
sample that moves: a track is looked for where it is expected to be, not where it last was.  The
rule is the project's own, after trackpy's nearest-velocity and drift predictors; parity with
trackpy is not pinned.  Every row i of level t(i) gets a velocity ``w_i [ndim]`` in pixels per level
once the links of its level are decided.  ``v0`` is ``initial_velocity`` (default zeros).

* own velocity of a linked row: for a row i of level t that is linked to source row s of level t_s,
  ``q_i[a] = (p_i[a] - p_s[a]) / (double)(t - t_s)``: one subtraction and one division.
* ``predictor='velocity'``: level 0: ``w_i = v0``.  A linked row: ``w_i = q_i``.  An unlinked row (a
  birth) takes ``w_j`` of the linked row j of the same level that is nearest in scaled coordinates:
  the scaled distance is ``sum_a (p_i[a] / sr[a] - p_j[a] / sr[a]) ** 2``, summed in axis order; a
  tie goes to the lower row; there is no distance limit.  If the level has no linked row, the birth
  takes ``v0``.
* ``predictor='drift'``: one vector per level, ``u_0 = v0``.  For level t >= 1 with M linked rows:
  ``u_t[a] = S_a / M`` if M > 0, otherwise ``u_t = u_{t-1}``.  ``S_a`` is summed in this fixed order:
  partial sum l of 256 starts at ``0.`` and adds ``q_i[a]`` of the linked rows among rows
  ``r0 + l, r0 + l + 256, ..`` of the level (r0: its first row), in ascending order; then for
  ``h = 128, 64, .., 1``: ``part[l] += part[l + h]`` for ``l < h``; ``S_a = part[0]``.
  ``w_i = u_t`` for every row of level t.
* prediction: source s (a row of level t_s, the previous level or a remembered one) is offered to
  level t at the predicted position ``P_s``.  ``'velocity'``:
  ``P_s[a] = p_s[a] + w_s[a] * (double)(t - t_s)``; ``'drift'``: the same with ``u_{t-1}[a]`` in
  place of ``w_s[a]``.  One multiplication, then one addition, with no contraction.
  ``P_s[a] / sr[a]`` takes the place of ``p_s[a] / sr[a]`` in the candidate search, and so in the
  ``d2`` that is stored.
* everything else is unchanged: the ten nearest candidates, the ``1 + 1e-7`` bound, sub-networks,
  the exact solver, the limits 30 and 64, birth order, ids and memory.  A remembered source still
  leaves after ``memory`` levels; what changes is that it is predicted forward by its age.
* the adaptive range composes with prediction: the rounds work on the ``d2`` of the predicted
  positions.
* limits of the rule: time is counted in levels.  In the table form (:func:`link`) a frame without
  rows is not a level, as today, so a gap in the frame numbers is not a gap in time.  Without
  ``initial_velocity``, a sample that already moves beyond the range at level 1 never acquires a
  velocity: nothing links, and a level without linked rows passes ``v0`` on.

``want_velocity=True`` returns the ``w`` of every row.  ``predictor=None`` runs exactly the code
paths above.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

from . import _abi, _lib
from .utils import guess_pos_columns, validate_tuple

MAX_NEIGHBORS = 10      # find_link.py:586
MAX_SUB_NET_SIZE = 30   # find_link.py:582
MAX_SUB_NET_DESTINATIONS = _abi.LINK_MAX_DESTINATIONS   # adaptive mode: the device solver's capacity, on the host too


class SubnetOversizeException(Exception):
    """A sub-network has more than 30 source features (find_link.py:531-533)."""


def _assign(n_src, n_dst, cand_src, cand_dst, cand_d):
    """Optimal links inside one level.  Returns link[dst] = src or -1."""
    link = np.full(n_dst, -1, dtype=np.int64)
    if len(cand_src) == 0:
        return link
    graph = coo_matrix((np.ones(len(cand_src)), (cand_src, cand_dst + n_src)),
                       shape=(n_src + n_dst, n_src + n_dst))
    _, comp = connected_components(graph, directed=False)
    comp_of_cand = comp[cand_src]
    order = np.argsort(comp_of_cand, kind='stable')
    bounds = np.flatnonzero(np.r_[True, np.diff(comp_of_cand[order]) != 0, True])
    for a, b in zip(bounds[:-1], bounds[1:]):
        idx = order[a:b]
        s_ids, s_loc = np.unique(cand_src[idx], return_inverse=True)
        d_ids, d_loc = np.unique(cand_dst[idx], return_inverse=True)
        if len(s_ids) == 1 and len(d_ids) == 1:
            link[d_ids[0]] = s_ids[0]
            continue
        if len(s_ids) > MAX_SUB_NET_SIZE:
            raise SubnetOversizeException("Subnetwork contains %d points" % len(s_ids))
        # minimise sum(d^2) + 1 per null link + 1 per missing link  ==  maximise sum(2 - d^2)
        big = 1e6
        cost = np.full((len(s_ids), len(d_ids) + len(s_ids)), big)
        cost[s_loc, d_loc] = cand_d[idx] ** 2 - 2.
        cost[:, len(d_ids):] = 0.          # "no link" for any source
        rows, cols = linear_sum_assignment(cost)
        for r, c in zip(rows, cols):
            if c < len(d_ids) and cost[r, c] < 0.5 * big:
                link[d_ids[c]] = s_ids[r]
    return link


def _adaptive_plan(search_range, adaptive_stop, adaptive_step):
    """``(stop_rel, step, K)`` of the adaptive search range (the module text), or ``ValueError``.
    search_range: one positive value per axis."""
    sr = np.asarray(search_range, dtype=np.float64)
    stop = np.asarray(validate_tuple(adaptive_stop, len(sr)), dtype=np.float64)
    with np.errstate(all='ignore'):
        stop_rel = float(np.max(stop / sr))
    if not 0 < stop_rel < 1:
        raise ValueError("adaptive_stop must be positive and below search_range")
    step = float(adaptive_step)
    if not 0 < step < 1:
        raise ValueError("adaptive_step must lie inside (0, 1)")
    rho, k = 1., 0
    while rho > stop_rel:
        rho = rho * step
        k += 1
        if k > _abi.LINK_MAX_ROUNDS:
            raise ValueError("adaptive_step reaches adaptive_stop only after more than %d rounds"
                             % _abi.LINK_MAX_ROUNDS)
    return stop_rel, step, k


def _assign_adaptive(n_src, n_dst, cand_src, cand_dst, cand_d2, stop_rel, step, level):
    """:func:`_assign` with the adaptive search range (the module text); cand_d2: the scaled squared
    distances, summed in axis order.  Returns (link[dst] = src or -1, round[dst])."""
    link = np.full(n_dst, -1, dtype=np.int64)
    rounds = np.zeros(n_dst, dtype=np.int32)
    edges = np.arange(len(cand_src))
    rho, k = 1., 0
    while len(edges):
        src, dst, d2 = cand_src[edges], cand_dst[edges], cand_d2[edges]
        graph = coo_matrix((np.ones(len(src)), (src, dst + n_src)), shape=(n_src + n_dst, n_src + n_dst))
        _, comp = connected_components(graph, directed=False)
        comp_of_cand = comp[src]
        order = np.argsort(comp_of_cand, kind='stable')
        bounds = np.flatnonzero(np.r_[True, np.diff(comp_of_cand[order]) != 0, True])
        oversize = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            idx = order[a:b]
            s_ids, s_loc = np.unique(src[idx], return_inverse=True)
            d_ids, d_loc = np.unique(dst[idx], return_inverse=True)
            if len(s_ids) > MAX_SUB_NET_SIZE or len(d_ids) > MAX_SUB_NET_DESTINATIONS:
                if rho <= stop_rel:
                    if len(s_ids) > MAX_SUB_NET_SIZE:
                        raise SubnetOversizeException("Subnetwork contains %d points (level %d, adaptive round %d)"
                                                      % (len(s_ids), level, k))
                    raise SubnetOversizeException("Subnetwork contains %d destinations (level %d, adaptive round %d)"
                                                  % (len(d_ids), level, k))
                oversize.append(edges[idx])
                continue
            rounds[d_ids] = k
            if len(s_ids) == 1 and len(d_ids) == 1:
                link[d_ids[0]] = s_ids[0]
                continue
            big = 1e6
            cost = np.full((len(s_ids), len(d_ids) + len(s_ids)), big)
            cost[s_loc, d_loc] = d2[idx] - 2. * (rho * rho)
            cost[:, len(d_ids):] = 0.          # "no link" for any source
            rows, cols = linear_sum_assignment(cost)
            for r, c in zip(rows, cols):
                if c < len(d_ids) and cost[r, c] < 0.5 * big:
                    link[d_ids[c]] = s_ids[r]
        if not oversize:
            break
        rho = rho * step
        k += 1
        b = rho * (1. + 1e-7)
        cut = np.concatenate(oversize)
        edges = cut[cand_d2[cut] <= b * b]
        rounds[np.setdiff1d(cand_dst[cut], cand_dst[edges])] = k     # the cut took their last edge
    return link, rounds


PREDICTORS = {'velocity': _abi.LINK_PREDICT_VELOCITY, 'drift': _abi.LINK_PREDICT_DRIFT}
DRIFT_PARTS = 256       # partial sums of the drift predictor's mean (the module text)


def _predict_plan(predictor, initial_velocity, want_velocity, ndim):
    """``(code, v0 [ndim] float64)`` of a predictive call, ``None`` without a predictor, or
    ``ValueError`` (the module text)."""
    if predictor is None:
        if initial_velocity is not None:
            raise ValueError("initial_velocity needs a predictor")
        if want_velocity:
            raise ValueError("want_velocity needs a predictor")
        return None
    if not isinstance(predictor, str) or predictor not in PREDICTORS:
        raise ValueError("predictor must be None, 'velocity' or 'drift', not %r" % (predictor,))
    if initial_velocity is None:
        initial_velocity = 0.
    if isinstance(initial_velocity, np.ndarray):
        initial_velocity = initial_velocity.reshape(-1).tolist()
    v0 = np.asarray(validate_tuple(initial_velocity, ndim), dtype=np.float64)
    if not np.all(np.isfinite(v0)):
        raise ValueError("initial_velocity must be finite")
    return PREDICTORS[predictor], v0


def _drift_mean(q, linked):
    """``u_t`` of the drift predictor: the mean of q [n, ndim] over the linked rows, summed in the
    order of the module text.  At least one row is linked."""
    n, ndim = q.shape
    trips = -(-n // DRIFT_PARTS)
    padded = np.zeros((trips * DRIFT_PARTS, ndim))
    padded[:n][linked] = q[linked]          # adding 0. for a row that is not linked changes no partial sum
    part = np.zeros((DRIFT_PARTS, ndim))
    for k in range(trips):
        part = part + padded[k * DRIFT_PARTS:(k + 1) * DRIFT_PARTS]
    h = DRIFT_PARTS // 2
    while h:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return part[0] / float(np.count_nonzero(linked))


def _level_velocity(code, pos, link, all_src_pos, all_src_t, t, sr, v0, u_prev):
    """``w [n, ndim]`` of the rows of level t >= 1 once ``link`` is decided (the module text)."""
    n, ndim = pos.shape
    linked = link >= 0
    q = np.zeros((n, ndim))
    if linked.any():
        src = link[linked]
        q[linked] = (pos[linked] - all_src_pos[src]) / (t - all_src_t[src]).astype(np.float64)[:, None]
    if code == _abi.LINK_PREDICT_DRIFT:
        u = _drift_mean(q, linked) if linked.any() else u_prev
        return np.broadcast_to(u, (n, ndim)).copy()
    w = q
    births = np.flatnonzero(~linked)
    if len(births) and not linked.any():
        w[births] = v0
    elif len(births):
        rows = np.flatnonzero(linked)
        d2 = np.zeros((len(births), len(rows)))
        for a in range(ndim):
            df = (pos[births, a] / sr[a])[:, None] - (pos[rows, a] / sr[a])[None, :]
            d2 = d2 + df * df
        w[births] = q[rows[np.argmin(d2, axis=1)]]      # the first minimum: a tie goes to the lower row
    return w


def _check_engine(engine):
    if engine not in ('host', 'device'):
        raise ValueError("engine must be 'host' or 'device', not %r" % (engine,))


def link_arrays(pos, frame_offset, search_range, memory=0, device=0, adaptive_stop=None, adaptive_step=0.95,
                diag=False, _on_device=False, predictor=None, initial_velocity=None, want_velocity=False):
    """Track ids of a level-sorted position table on the MI355X (``ctr_link_device``): the rule
    of :func:`link_levels`, the optimum of every sub-network from an exact assignment solver.

    pos: [N, ndim] float64, ndarray or a torch tensor on cuda:``device``; frame_offset: [T + 1]
    int64, rows ``[off[t], off[t + 1])`` are level t (the tensors of a preceding locate go in as
    they are).  Returns int64 ids [N] as an ndarray (``_on_device``, internal: as the tensor).
    Raises :class:`SubnetOversizeException` for a sub-network of more than 30 sources and
    ``EngineError`` for one of more than 64 destinations (the solver's capacity), or when there
    is no library or no GPU.

    ``adaptive_stop`` (a scalar or one value per axis) and ``adaptive_step``: the adaptive search
    range of the module text (``ctr_link_adaptive_device``); both limits then raise
    :class:`SubnetOversizeException`, and only for a sub-network that is still beyond them at
    ``adaptive_stop``.  ``diag``: returns ``(ids, adaptive_round)``, the second int32 [N], all
    zeros without ``adaptive_stop``.

    ``predictor`` (``'velocity'`` or ``'drift'``) and ``initial_velocity`` (a scalar or one value per
    axis, pixels per level): the prediction of the module text (``ctr_link_predict_device``, always
    queued level by level; with ``adaptive_stop`` the two compose).  ``want_velocity`` appends the
    velocities, float64 [N, ndim], to what is returned."""
    plan = None
    nd = pos.shape[1] if getattr(pos, 'ndim', 0) == 2 else len(np.atleast_1d(search_range))
    if adaptive_stop is not None:         # refused before any device work
        plan = _adaptive_plan(validate_tuple(search_range, nd), adaptive_stop, adaptive_step)
    pred = _predict_plan(predictor, initial_velocity, want_velocity, nd)
    eng = _lib.default_engine(device)     # EngineError without a library or a GPU
    import torch
    dev = torch.device('cuda', device)
    if int(memory) != memory or memory < 0:
        raise ValueError("memory must be a non-negative integer")
    with torch.cuda.device(dev):
        if isinstance(pos, torch.Tensor):
            if pos.device != dev or pos.dtype != torch.float64:
                raise ValueError("a position tensor is float64 on cuda:%d" % device)
            pos_t = pos.contiguous()
        else:
            arr = np.ascontiguousarray(pos, dtype=np.float64)
            if arr.ndim != 2:
                arr = arr.reshape(-1, len(np.atleast_1d(search_range)))
            pos_t = torch.from_numpy(arr).to(dev)
        if pos_t.dim() != 2 or pos_t.shape[1] not in (2, 3):
            raise ValueError("pos must be [N, 2] or [N, 3]")
        n, ndim = int(pos_t.shape[0]), int(pos_t.shape[1])
        sr = validate_tuple(search_range, ndim)
        if not all(np.isfinite(s) and s > 0 for s in sr):
            raise ValueError("search_range must be positive")
        if isinstance(frame_offset, torch.Tensor):
            if frame_offset.device != dev or frame_offset.dtype != torch.int64 or frame_offset.dim() != 1:
                raise ValueError("a frame_offset tensor is int64 [T + 1] on cuda:%d" % device)
            off_t = frame_offset.contiguous()
        else:
            off = np.ascontiguousarray(frame_offset, dtype=np.int64).reshape(-1)
            if len(off) and (off[0] != 0 or off[-1] != n or np.any(np.diff(off) < 0)):
                raise ValueError("frame_offset must rise from 0 to the number of features")
            off_t = torch.from_numpy(off).to(dev)
        n_levels = max(int(off_t.numel()) - 1, 0)
        if n and not n_levels:
            raise ValueError("features without levels")
        particle = torch.empty(n, dtype=torch.int64, device=dev)
        rounds = torch.zeros(n, dtype=torch.int32, device=dev) if diag else None
        velocity = torch.empty((n, ndim), dtype=torch.float64, device=dev) if want_velocity else None

        def result():
            out = [particle] + ([rounds] if diag else []) + ([velocity] if want_velocity else [])
            if not _on_device:
                out = [o.cpu().numpy() for o in out]
            return tuple(out) if len(out) > 1 else out[0]
        if n == 0:          # nothing to launch (and an empty tensor has no address to pass)
            return result()
        n_tracks = torch.empty(1, dtype=torch.int64, device=dev)
        status = torch.empty(4, dtype=torch.int32, device=dev)
        d = _abi.LinkPredict() if pred is not None else _abi.Link() if plan is None else _abi.LinkAdaptive()
        d.ndim, d.memory, d.n_levels, d.n_features = ndim, int(memory), n_levels, n
        for a in range(ndim):
            d.search_range[a] = float(sr[a])
        d.pos, d.frame_offset = pos_t.data_ptr(), off_t.data_ptr()
        d.particle, d.n_tracks, d.status = particle.data_ptr(), n_tracks.data_ptr(), status.data_ptr()
        if plan is not None:
            d.stop_rel, d.step, d.max_rounds = plan
            d.adaptive_round = rounds.data_ptr() if diag else None
        if pred is not None:
            d.predictor = pred[0]             # max_rounds stays 0 without adaptive_stop
            for a in range(ndim):
                d.initial_velocity[a] = float(pred[1][a])
            d.velocity = velocity.data_ptr() if want_velocity else None
            eng.on_current_stream(eng.link_predict_device, d, dev=dev)
        elif plan is None:
            eng.on_current_stream(eng.link_device, d, dev=dev)
        else:
            eng.on_current_stream(eng.link_adaptive_device, d, dev=dev)
        code, level, size, _ = (int(v) for v in status.cpu())   # the one synchronisation of the call
    if code == _abi.LINK_OVERSIZE:
        raise SubnetOversizeException("Subnetwork contains %d points (level %d)" % (size, level))
    if code == _abi.LINK_CAPACITY and plan is not None:
        raise SubnetOversizeException("Subnetwork contains %d destinations (level %d)" % (size, level))
    if code == _abi.LINK_CAPACITY:
        raise _lib.EngineError("ctr_link_device: a sub-network of level %d has %d destinations, the "
                               "device solver takes %d (CTR_ERR_UNSUPPORTED)"
                               % (level, size, _abi.LINK_MAX_DESTINATIONS))
    if code != _abi.LINK_OK:
        raise _lib.EngineError("ctr_link_device: unknown status %d" % code)
    return result()


def _link_levels_device(levels, ndim, search_range, memory, device, adaptive_stop, adaptive_step, diag,
                        predictor=None, initial_velocity=None, want_velocity=False):
    counts = [len(c) for c in levels]
    offs = np.r_[0, np.cumsum(counts)].astype(np.int64)
    pos = (np.concatenate([c.reshape(-1, ndim) for c in levels]) if levels else np.zeros((0, ndim)))

    def split(v):
        return [v[a:b] for a, b in zip(offs[:-1], offs[1:])]
    if predictor is not None:
        out = link_arrays(pos, offs, search_range, memory, device, adaptive_stop, adaptive_step, diag=diag,
                          predictor=predictor, initial_velocity=initial_velocity, want_velocity=want_velocity)
        return tuple(split(o) for o in out) if isinstance(out, tuple) else split(out)
    if adaptive_stop is None and not diag:
        ids = link_arrays(pos, offs, search_range, memory, device)
        return [ids[a:b] for a, b in zip(offs[:-1], offs[1:])]
    ids, rounds = link_arrays(pos, offs, search_range, memory, device, adaptive_stop, adaptive_step, diag=True)
    ids = [ids[a:b] for a, b in zip(offs[:-1], offs[1:])]
    return (ids, [rounds[a:b] for a, b in zip(offs[:-1], offs[1:])]) if diag else ids


def link_levels(levels, search_range, memory=0, engine='host', device=0, adaptive_stop=None, adaptive_step=0.95,
                diag=False, predictor=None, initial_velocity=None, want_velocity=False):
    """Link a sequence of coordinate arrays ``[n_t, ndim]`` (one per frame).
    Returns a list of integer id arrays aligned with the input.  ``engine='device'``: on the
    MI355X through :func:`link_arrays` (no fallback: ``EngineError`` without a GPU).
    ``adaptive_stop``, ``adaptive_step``: the adaptive search range of the module text, on either
    engine.  ``diag``: returns ``(ids, adaptive_round)``, two lists of arrays aligned with the input
    (the rounds int32, all zeros without ``adaptive_stop``).
    ``predictor`` (``'velocity'`` or ``'drift'``), ``initial_velocity`` (a scalar or one value per
    axis, pixels per level): the prediction of the module text, on either engine; a level without
    rows is a level here (time passes).  ``want_velocity`` appends the velocities, a list of float64
    ``[n_t, ndim]`` arrays, to what is returned."""
    _check_engine(engine)
    levels = [np.asarray(c, dtype=np.float64) for c in levels]
    if len(levels) == 0:
        if adaptive_stop is not None:
            _adaptive_plan(validate_tuple(search_range, len(np.atleast_1d(search_range))), adaptive_stop, adaptive_step)
        _predict_plan(predictor, initial_velocity, want_velocity, len(np.atleast_1d(search_range)))
        if engine == 'device':
            _lib.default_engine(device)
        out = [[]] + ([[]] if diag else []) + ([[]] if want_velocity else [])
        return tuple(out) if len(out) > 1 else out[0]
    ndim = levels[0].shape[1] if levels[0].ndim == 2 else len(np.atleast_1d(search_range))
    sr = np.asarray(validate_tuple(search_range, ndim), dtype=np.float64)
    plan = None if adaptive_stop is None else _adaptive_plan(sr, adaptive_stop, adaptive_step)
    pred = _predict_plan(predictor, initial_velocity, want_velocity, ndim)
    if engine == 'device':
        return _link_levels_device(levels, ndim, tuple(sr), memory, device, adaptive_stop, adaptive_step, diag,
                                   predictor, initial_velocity, want_velocity)
    next_id = 0
    ids_out = []
    rounds_out = []
    vel_out = []
    # sources of the next level: previous level + remembered lost features
    src_pos = np.zeros((0, ndim))
    src_id = np.zeros(0, dtype=np.int64)
    mem_pos = np.zeros((0, ndim))
    mem_id = np.zeros(0, dtype=np.int64)
    mem_age = np.zeros(0, dtype=np.int64)
    # prediction: the velocity of every source and the level it was seen at; the drift of the last level
    src_w = mem_w = np.zeros((0, ndim))
    mem_t = np.zeros(0, dtype=np.int64)
    u_prev = None if pred is None else pred[1]
    for t, pos in enumerate(levels):
        pos = pos.reshape(-1, ndim)
        n = len(pos)
        rounds = np.zeros(n, dtype=np.int32)
        if t == 0:
            ids = np.arange(n, dtype=np.int64)      # find_link.py:620-623
            next_id = n
            if pred is not None:
                w = np.broadcast_to(pred[1], (n, ndim)).copy()
        else:
            all_src_pos = np.concatenate([src_pos, mem_pos])
            all_src_id = np.concatenate([src_id, mem_id])
            n_src = len(all_src_pos)
            offered = all_src_pos
            if pred is not None:                    # the sources at their predicted positions
                all_src_t = np.concatenate([np.full(len(src_pos), t - 1, dtype=np.int64), mem_t])
                age = (t - all_src_t).astype(np.float64)[:, None]
                if pred[0] == _abi.LINK_PREDICT_DRIFT:
                    offered = all_src_pos + u_prev[None, :] * age
                else:
                    offered = all_src_pos + np.concatenate([src_w, mem_w]) * age
            ids = np.full(n, -1, dtype=np.int64)
            link = np.full(n, -1, dtype=np.int64)
            if n_src and n:
                tree = cKDTree(offered / sr, 15)
                k = min(MAX_NEIGHBORS, n_src)
                dists, inds = tree.query(pos / sr, k, distance_upper_bound=1 + 1e-7)
                dists = dists.reshape(n, -1)
                inds = inds.reshape(n, -1)
                ok = np.isfinite(dists)
                cand_dst = np.nonzero(ok)[0]
                if plan is None:
                    link = _assign(n_src, n, inds[ok], cand_dst, dists[ok])
                else:
                    cand_src = inds[ok]
                    d2 = np.zeros(len(cand_src))
                    for a in range(ndim):       # in axis order, as the device sums it
                        df = pos[cand_dst, a] / sr[a] - offered[cand_src, a] / sr[a]
                        d2 = d2 + df * df
                    link, rounds = _assign_adaptive(n_src, n, cand_src, cand_dst, d2, plan[0], plan[1], t)
            linked = link >= 0
            ids[linked] = all_src_id[link[linked]]
            # new tracks in lexicographic order of position (find_link.py:379-383,703)
            new = np.flatnonzero(~linked)
            if len(new):
                order = np.lexsort(pos[new].T[::-1])
                ids[new[order]] = next_id + np.arange(len(new))
                next_id += len(new)
            if pred is not None:
                w = _level_velocity(pred[0], pos, link, all_src_pos, all_src_t, t, sr, pred[1], u_prev)
                if pred[0] == _abi.LINK_PREDICT_DRIFT and linked.any():
                    u_prev = w[0]
            # memory bookkeeping (find_link.py:716-732)
            if memory > 0:
                used = np.zeros(n_src, dtype=bool)
                used[link[linked]] = True
                lost_new = ~used[:len(src_pos)]
                keep_mem = ~used[len(src_pos):] & (mem_age + 1 < memory)
                if pred is not None:
                    mem_w = np.concatenate([mem_w[keep_mem], src_w[lost_new]])
                    mem_t = np.concatenate([mem_t[keep_mem], np.full(int(lost_new.sum()), t - 1, dtype=np.int64)])
                mem_pos = np.concatenate([mem_pos[keep_mem], src_pos[lost_new]])
                mem_id = np.concatenate([mem_id[keep_mem], src_id[lost_new]])
                mem_age = np.concatenate([mem_age[keep_mem] + 1,
                                          np.zeros(int(lost_new.sum()), dtype=np.int64)])
        ids_out.append(ids)
        rounds_out.append(rounds)
        src_pos, src_id = pos, ids
        if pred is not None:
            vel_out.append(w)
            src_w = w
    out = [ids_out] + ([rounds_out] if diag else []) + ([vel_out] if want_velocity else [])
    return tuple(out) if len(out) > 1 else out[0]


def link(f, search_range, memory=0, pos_columns=None, t_column='frame', engine='host', device=0, adaptive_stop=None,
         adaptive_step=0.95, diag=False, predictor=None, initial_velocity=None, want_velocity=False):
    """Return a copy of ``f`` (sorted by frame) with a ``particle`` column.  ``engine='device'``
    links on the MI355X (:func:`link_arrays`); the host path is the default.  ``adaptive_stop``,
    ``adaptive_step``: the adaptive search range of the module text; ``diag`` adds the column
    ``adaptive_round``.  ``predictor``, ``initial_velocity``: the prediction of the module text, time
    counted in the frames that have rows; ``want_velocity`` adds one column ``v<pos column>`` per
    axis."""
    _check_engine(engine)
    if pos_columns is None:
        pos_columns = guess_pos_columns(f)
    result = f.sort_values(t_column, kind='stable').copy()
    frames = result[t_column].values
    pos = result[pos_columns].values
    uniq, starts = np.unique(frames, return_index=True)
    stops = np.r_[starts[1:], len(frames)]
    if len(starts) == 0:
        _predict_plan(predictor, initial_velocity, want_velocity, len(pos_columns))
    out = link_levels([pos[a:b] for a, b in zip(starts, stops)], search_range, memory, engine, device,
                      adaptive_stop, adaptive_step, diag, predictor, initial_velocity, want_velocity)
    out = list(out) if (diag or want_velocity) else [out]
    ids = out.pop(0)
    result['particle'] = np.concatenate(ids) if len(ids) else np.zeros(0, dtype=np.int64)
    if diag:
        rounds = out.pop(0)
        result['adaptive_round'] = np.concatenate(rounds) if len(rounds) else np.zeros(0, dtype=np.int32)
    if want_velocity:
        vel = np.concatenate(out.pop(0)) if len(ids) else np.zeros((0, len(pos_columns)))
        for a, name in enumerate(pos_columns):
            result['v' + name] = vel[:, a]
    return result
