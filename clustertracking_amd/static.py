"""Pair correlation function g(r) of a feature table on the MI355X: the structure of a frame, where
``drift``, ``msd`` and ``motion`` describe dynamics.  Users read three numbers off it that other calls
ask them for: the bond length inside a cluster (``dist`` of ``constraints.dimer`` / ``trimer`` /
``tetramer``) is the first peak of g(r) over the pairs of one cluster (``pairs='same'``), ``separation``
of ``find_clusters``, ``locate`` and ``find_link`` is the gap behind that peak, and whether a sample is
dilute enough for ``cluster_tracks`` and ``motion`` shows in g(r) between clusters (``pairs='other'``).
The reference leaves this to trackpy (``static.pair_correlation_2d`` / ``_3d``), one kd-tree query per
particle and frame; here it is an all-pairs distance histogram per frame and an edge correction per
reference row, on the tensors that ``find_link_arrays`` and ``refine_arrays`` already hold.

The rule is the project's own dense rule (``include/ctrefine.h`` has it too, DESIGN.md 7b;
``tests/_pair_correlation.py`` restates it in NumPy):

1. Bins.  ``B = ceil(cutoff / dr)``; ``r_edges[b] = b * dr`` for ``b = 0 .. B``; ``edge2 = r_edges *
   r_edges``; ``shell[b] = pi * (edge2[b + 1] - edge2[b])`` in 2D and ``4/3 * pi * (r_edges[b + 1]**3 -
   r_edges[b]**3)`` in 3D.  The host computes ``edge2`` and ``shell`` once and hands them to the device.
2. Scaling.  ``q = pos * mpp`` per axis, one rounding; everything below is in these units.
3. Box.  ``boundary``, ``[[lo...], [hi...]]`` in pixels, times ``mpp``; by default the minimum and the
   maximum of ``q`` over all rows of the call, NaN ignored: one box for all frames.  ``V`` is the
   product over the axes, in axis order, of ``hi_a - lo_a``.
4. A row exists when every coordinate is finite and within ``[lo_a, hi_a]``.  ``n_rows[t]`` counts the
   existing rows of frame t; ``rho_t = (n_rows[t] - 1) / V``.
5. Reference rows.  ``edge='none'`` and ``'arc'``: every existing row.  ``'interior'``: the existing
   rows with ``q_a - lo_a >= r_edges[B]`` and ``hi_a - q_a >= r_edges[B]`` on every axis.  ``n_ref[t]``
   counts them.
6. Pairs.  A reference row ``i`` and an existing row ``j != i`` of the same frame are a pair, ordered:
   two reference rows count each other.  ``pairs='same'``: also ``group[i] == group[j] >= 0``;
   ``'other'``: the pairs that fail that.  So ``count_all == count_same + count_other`` in every bin.
7. Binning.  ``d2`` is the sum over the axes, in axis order, of ``(q_j - q_i)_a`` squared, every product
   and sum rounded on its own.  The pair falls in bin ``b`` iff ``edge2[b] <= d2 < edge2[b + 1]``, with
   ``d2 >= edge2[B]`` in none; coincident distinct rows (``d2 == 0``) in bin 0.  ``count[t, b]`` is exact.
8. Weight.  ``weight[t, b]`` is the sum over the reference rows of frame t, in row order, of
   ``phi_i(b)``.  ``'none'`` and ``'interior'``: ``phi = 1``, ``weight[t, b] = n_ref[t]``.  ``'arc'`` (2D):
   the fraction of the circle of radius ``R = r_edges[b] + dr / 2`` around row i inside the box -- the
   quadrant angles of the four quadrants (wall distance ``a`` along axis 0 in ``(hi0 - q0, q0 - lo0)``,
   ``b'`` along axis 1 in ``(hi1 - q1, q1 - lo1)``) added and divided by ``2 pi``; a quadrant angle is
   ``pi / 2`` when ``a >= R`` and ``b' >= R`` and ``max(0, asin(min(b' / R, 1)) - acos(min(a / R, 1)))``
   otherwise.  A row further than ``R`` from every wall gets exactly 1.0 without trigonometry.
9. ``g_frame[t, b] = count[t, b] / ((rho_t * shell[b]) * weight[t, b])``, NaN where the denominator is
   not positive and finite: an empty or one-row frame, a degenerate box (``V = 0`` makes it infinite),
   no reference row.
10. ``g[b]`` is the sum of ``count[t, b]`` over t divided by the sum over t, in frame order, of the
    positive finite denominators of clause 9; NaN where no frame has one.

Where this differs from trackpy: the pooled ``g`` is a ratio of sums over the frames (a ratio
estimator), not a mean of per-particle ratios; the arc correction is taken at the middle of the bin;
there is one box for all frames; coincident rows are counted; there is a result per frame; and every
row is a reference (no ``fraction`` or ``p_indices`` sampling).  Parity with trackpy itself is not pinned by a
test: it is not a dependency.  All pairs of a frame are visited; there is no cell list.

Nearest neighbours and proximity (``neighbors_arrays``, ``neighbors``, ``proximity``;
``ctr_neighbors_device``) are the structure per feature, where g(r) is pooled: how far every row is from
its nearest rows, which rows those are, and how many lie within a distance.  Within a frame (``lag=0``)
that is the upper bound of ``search_range``, the coordination number and, with ``pairs='same'``, the bond
length per cluster and frame; from frame t into frame t + 1 (``lag=1``) it is the displacement that
``search_range`` must exceed; with ``pairs='other'`` it is the filter that keeps ``cluster_tracks``,
``motion`` and ``diffusion_tensor_ci`` to clusters that diffuse freely.  trackpy has ``static.proximity``
for the first; parity with it is not pinned.  The rule (``include/ctrefine.h``, DESIGN.md 7b;
``tests/_neighbors.py`` restates it in NumPy):

1. Scaling.  ``q = pos * mpp`` per axis, one rounding: clause 2 above.
2. A row exists when every coordinate of ``q`` is finite.  There is no box.
3. Candidates.  The candidates of row ``i`` of frame ``t`` are the existing rows ``j`` of frame ``t + lag``;
   with ``lag == 0``, ``j == i`` is excluded; a row of a frame with ``t + lag >= T`` has no candidate.
   ``pairs='same'``: also ``group[i] == group[j] >= 0``; ``'other'``: the candidates that fail that.
4. Distance.  ``d2`` is the sum over the axes, in axis order, of ``(q_j - q_i)_a`` squared, every product
   and sum rounded on its own.  A candidate qualifies when ``d2 < limit2``, strictly: a row at exactly
   ``max_dist`` does not.  ``limit2 = max_dist * max_dist``, computed once on the host; ``+inf`` without.
5. ``count[i]`` is the number of qualifying candidates, exact: a coordination number with ``max_dist``.
6. Neighbours.  The qualifying candidates sorted by ``(d2, j)`` ascending; the first ``k`` are the
   neighbours: ``dist2[i, m]`` their ``d2``, ``index[i, m]`` their global row, ``dist[i, m] =
   sqrt(dist2[i, m])``.  Coincident rows (``d2 == 0``) are neighbours like any other.  Where fewer than
   ``k`` qualify, the remaining entries are NaN, NaN and -1.
7. Rows with no result: a row that does not exist, a row of a frame without a candidate frame and a row
   outside ``[frame_offset[0], frame_offset[T])`` get NaN, -1 and 0, and are nobody's neighbour.
8. Per particle (with ``particle`` and ``n_particles = P``).  ``particle_min2[p]`` is the minimum of
   ``dist2[i, 0]`` over the rows with ``particle[i] == p`` that have a neighbour, ``particle_min[p]`` its
   square root, NaN where there is none; rows with an id outside ``[0, P)`` contribute nowhere.
9. A refused table.  A ``frame_offset`` that does not rise within ``[0, N]``: ``status[0] =
   _abi.NBR_BAD_TABLE``, every float output NaN, ``index`` -1, ``count`` 0; ``ValueError`` for ndarrays.

All rows of the candidate frame are visited; every output element has one owner thread, so the same
bytes come back on every call.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import collections
import math

import numpy as np

from . import _abi, _tables

PairCorrelation = collections.namedtuple('PairCorrelation', ['r_edges', 'g', 'g_frame', 'count', 'weight', 'n_ref', 'n_rows', 'status'])
Neighbors = collections.namedtuple('Neighbors', ['dist', 'dist2', 'index', 'count', 'particle_min', 'particle_min2', 'status'])

_REFUSED = "pair_correlation_arrays: frame_offset must rise within [0, N]"
_NBR_REFUSED = "neighbors_arrays: frame_offset must rise within [0, N]"


def bins(cutoff, dr, ndim):
    """clause 1: ``(r_edges [B + 1], edge2 [B + 1], shell [B])`` as float64 ndarrays"""
    cutoff, dr = _tables.positive(cutoff, 'cutoff'), _tables.positive(dr, 'dr')
    if cutoff / dr > _abi.PCF_MAX_BINS:
        raise ValueError("cutoff / dr gives more than %d bins" % _abi.PCF_MAX_BINS)
    n_bins = int(math.ceil(cutoff / dr))
    r_edges = np.arange(n_bins + 1, dtype=np.float64) * dr
    edge2 = r_edges * r_edges
    if ndim == 2:
        shell = np.pi * (edge2[1:] - edge2[:-1])
    else:
        shell = 4. / 3. * np.pi * (r_edges[1:] ** 3 - r_edges[:-1] ** 3)
    return r_edges, edge2, shell


def _scales(mpp, ndim):
    scale = np.asarray(mpp, dtype=np.float64)
    if scale.ndim == 0:
        scale = np.repeat(scale, ndim)
    if scale.shape != (ndim,) or not np.isfinite(scale).all() or not (scale > 0).all():
        raise ValueError("mpp must be a finite positive number or one per axis (%d), not %r" % (ndim, mpp))
    return scale


def _boundary(boundary, ndim):
    """None, a tensor as it is, or a float64 ndarray [2, ndim] with lo <= hi"""
    if boundary is None:
        return None
    if not _tables.is_tensor(boundary):
        boundary = np.asarray(boundary, dtype=np.float64)
    if tuple(boundary.shape) != (2, ndim):
        raise ValueError("boundary must be [[lo...], [hi...]] with %d entries each, not %s" % (ndim, tuple(boundary.shape)))
    if isinstance(boundary, np.ndarray) and not (np.isfinite(boundary).all() and (boundary[1] >= boundary[0]).all()):
        raise ValueError("boundary must be finite with hi >= lo on every axis")
    return boundary


def _pairs(pairs, group, word='group'):
    """``word``: what the caller calls ``group``"""
    if pairs not in _abi.PCF_PAIRS_CODES:
        raise ValueError("pairs must be one of 'all', 'same', 'other', not %r" % (pairs,))
    if pairs != 'all' and group is None:
        raise ValueError("pairs=%r needs a %s" % (pairs, word))


def _modes(edge, pairs, group, ndim):
    if edge not in _abi.PCF_EDGE_CODES:
        raise ValueError("edge must be one of 'none', 'interior', 'arc', not %r" % (edge,))
    if edge == 'arc' and ndim != 2:
        raise ValueError("edge='arc' is the correction of a rectangle: ndim 2 only; use 'interior' or 'none'")
    _pairs(pairs, group)


def pair_correlation_arrays(pos, frame_offset, cutoff, dr=0.5, mpp=1., boundary=None, edge='arc', group=None,
                            pairs='all', device=0):
    """The pair correlation function of every frame and of all frames pooled
    (``ctr_pair_correlation_device``; the module's rule, where trackpy has ``pair_correlation_2d`` /
    ``_3d`` for one frame).

    pos float64 ``[N, ndim]``, ndim 2 or 3, rows sorted by frame; frame_offset int64 ``[T + 1]``: what
    ``locate_arrays``, ``find_link_arrays``, ``refine_arrays`` and ``subtract_drift_arrays`` return, as
    ndarrays or as tensors on ``cuda:device``.  cutoff, dr: the largest distance and the bin width, in
    the units of ``pos * mpp``; at most ``_abi.PCF_MAX_BINS`` bins.  mpp: microns per pixel, a number or
    one per axis.  boundary: ``[[lo...], [hi...]]`` in pixels, default the extent of all rows.  edge:
    ``'none'`` (g falls towards the cutoff), ``'interior'`` (only rows further than the cutoff from every
    wall refer) or ``'arc'`` (2D: every row refers, weighted by the part of its circle inside the box).
    group: int64 ``[N]``, e.g. the cluster labels; pairs: ``'all'``, ``'same'`` (both rows of one group
    ``>= 0``) or ``'other'``.

    Returns ``PairCorrelation(r_edges [B + 1], g [B], g_frame [T, B], count int64 [T, B], weight [T, B],
    n_ref int64 [T], n_rows int64 [T], status)``: ndarrays and an int for ndarrays, tensors (status:
    int32 ``[1]``) for a tensor ``pos``, and then nothing is read back to the host.  A frame_offset that
    does not rise within ``[0, N]`` raises ``ValueError`` for ndarrays; for tensors status is
    ``_abi.PCF_BAD_TABLE``, g, g_frame and weight NaN and the counts 0.  The same bytes on every call."""
    pos, n, ndim = _tables.positions(pos)
    r_edges, edge2, shell = bins(cutoff, dr, ndim)
    scale = _scales(mpp, ndim)
    _modes(edge, pairs, group, ndim)
    boundary = _boundary(boundary, ndim)
    frame_offset, n_frames = _tables.offsets(frame_offset)
    if group is not None:
        group = _tables.int64_column(group, n, 'group')
    if n_frames > 2 ** 31 - 3 or n > 2 ** 31 - 1:
        raise ValueError("too many frames or features for one call")
    as_tensor = _tables.is_tensor(pos)
    n_bins = len(shell)
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        group_t = None if group is None else _tables.on_device(group, dev, torch.int64, 'group')
        scale_t = torch.from_numpy(scale).to(dev)
        if boundary is not None:
            box = _tables.on_device(boundary, dev, torch.float64, 'boundary') * scale_t
        elif n:
            q = pos_t * scale_t
            nan = q.isnan()
            box = torch.stack([q.masked_fill(nan, math.inf).amin(0), q.masked_fill(nan, -math.inf).amax(0)])
        else:
            box = torch.tensor([[math.inf] * ndim, [-math.inf] * ndim], dtype=torch.float64, device=dev)
        box = box.contiguous()
        edges_t, edge2_t, shell_t = (torch.from_numpy(x).to(dev) for x in (r_edges, edge2, shell))
        g = torch.empty(n_bins, dtype=torch.float64, device=dev)
        g_frame = torch.empty((n_frames, n_bins), dtype=torch.float64, device=dev)
        count = torch.empty((n_frames, n_bins), dtype=torch.int64, device=dev)
        weight = torch.empty((n_frames, n_bins), dtype=torch.float64, device=dev)
        n_ref = torch.empty(n_frames, dtype=torch.int64, device=dev)
        n_rows = torch.empty(n_frames, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        d = _abi.PairCorrelation()
        d.ndim, d.edge, d.pairs = ndim, _abi.PCF_EDGE_CODES[edge], _abi.PCF_PAIRS_CODES[pairs]
        d.n_bins, d.n_frames, d.n_features, d.dr = n_bins, n_frames, n, float(dr)
        for a in range(ndim):
            d.mpp[a] = float(scale[a])
        d.pos, d.frame_offset = pos_t.data_ptr() or None, off_t.data_ptr()
        d.group = None if group_t is None else (group_t.data_ptr() or None)
        d.box, d.edge2, d.shell = box.data_ptr(), edge2_t.data_ptr(), shell_t.data_ptr()
        d.g, d.g_frame, d.count, d.weight = g.data_ptr(), g_frame.data_ptr() or None, count.data_ptr() or None, weight.data_ptr() or None
        d.n_ref, d.n_rows, d.status = n_ref.data_ptr() or None, n_rows.data_ptr() or None, status.data_ptr()
        eng.on_current_stream(eng.pair_correlation_device, d, dev=dev)
        out = _tables.results(as_tensor, status, _abi.PCF_OK, _REFUSED, edges_t, g, g_frame, count, weight, n_ref, n_rows)
        return PairCorrelation(*out, status if as_tensor else _abi.PCF_OK)


def pair_correlation(f, cutoff, dr=0.5, mpp=1., boundary=None, edge='arc', group_column=None, pairs='all',
                     pos_columns=None, t_column='frame', per_frame=False, device=0):
    """The pair correlation function of a table of features: ``(r_edges, g)`` as trackpy's
    ``pair_correlation_2d`` returns them, ``g`` pooled over all frames of ``f`` by the module's rule
    (a ratio of sums, where trackpy takes one frame at a time).  With ``per_frame=True`` ``g`` is a
    DataFrame indexed by frame (dense from the first to the last; a frame without rows is NaN) with
    one column per bin's left edge.

    f: a DataFrame with the position columns (default ``['y', 'x']``, with ``'z'`` in front where the
    table has one) and ``t_column``; no ``particle`` column is needed.  group_column: an integer column
    such as ``'cluster'``, ``'particle'`` or ``'cluster_track'`` for ``pairs='same'`` / ``'other'``.  The
    other arguments as for :func:`pair_correlation_arrays`."""
    import pandas as pd
    _pairs(pairs, group_column, 'group_column')
    _, offset, first, _, _, _, pos, *group = _tables.frame_sorted(
        f, pos_columns, t_column, () if group_column is None else (group_column,), particle=False)
    res = pair_correlation_arrays(pos, offset, cutoff, dr, mpp, boundary, edge, group[0] if group else None, pairs, device)
    if not per_frame:
        return res.r_edges, res.g
    frames = pd.RangeIndex(first, first + len(offset) - 1, name=t_column)
    return res.r_edges, pd.DataFrame(res.g_frame, index=frames, columns=pd.Index(res.r_edges[:-1], name='r'))


def neighbors_arrays(pos, frame_offset, k=1, mpp=1., max_dist=None, group=None, pairs='all', lag=0, particle=None,
                     n_particles=None, device=0):
    """The ``k`` nearest rows of every row among the rows of the frame ``lag`` frames on, how many lie
    within ``max_dist`` and, per particle, the smallest nearest-neighbour distance
    (``ctr_neighbors_device``; the module's rule, where trackpy has ``static.proximity`` and a
    ``cKDTree`` per frame).

    pos float64 ``[N, ndim]``, ndim 2 or 3, rows sorted by frame; frame_offset int64 ``[T + 1]``: what
    ``locate_arrays``, ``find_link_arrays``, ``refine_arrays`` and ``subtract_drift_arrays`` return, as
    ndarrays or as tensors on ``cuda:device``.  k: 1 .. ``_abi.NBR_MAX_K``.  mpp: microns per pixel, a
    number or one per axis.  max_dist: only rows nearer than this, in the units of ``pos * mpp``, are
    neighbours and are counted; default no limit.  group: int64 ``[N]``, e.g. the cluster labels; pairs:
    ``'all'``, ``'same'`` (both rows of one group ``>= 0``) or ``'other'``.  lag: 0 for the neighbours
    within a frame, 1 for those of frame t in frame t + 1.  particle: int64 ``[N]`` with ids in
    ``[0, n_particles)`` (default ``particle.max() + 1``, one host read for a tensor).

    Returns ``Neighbors(dist [N, k], dist2 [N, k], index int64 [N, k], count int64 [N], particle_min [P]
    or None, particle_min2 [P] or None, status)``: ndarrays and an int for ndarrays, tensors (status: int32
    ``[1]``) for a tensor ``pos``, and then nothing is read back to the host.  NaN and -1 where a row has
    fewer than ``k`` neighbours.  A frame_offset that does not rise within ``[0, N]`` raises ``ValueError``
    for ndarrays; for tensors status is ``_abi.NBR_BAD_TABLE``, the distances NaN, index -1 and count 0.
    The same bytes on every call."""
    pos, n, ndim = _tables.positions(pos)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= _abi.NBR_MAX_K:
        raise ValueError("k must be an integer within 1 .. %d, not %r" % (_abi.NBR_MAX_K, k))
    if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 0 <= lag <= 2 ** 31 - 1:
        raise ValueError("lag must be an integer >= 0, not %r" % (lag,))
    limit2 = math.inf
    if max_dist is not None:
        limit2 = _tables.positive(max_dist, 'max_dist') ** 2
        if not limit2 > 0:
            raise ValueError("max_dist squared must be positive, not %r" % (limit2,))
    scale = _scales(mpp, ndim)
    _pairs(pairs, group)
    frame_offset, n_frames = _tables.offsets(frame_offset)
    if group is not None:
        group = _tables.int64_column(group, n, 'group')
    if particle is None and n_particles is not None:
        raise ValueError("n_particles needs a particle column")
    if particle is not None:
        particle, n_particles = _tables.particles(_tables.int64_column(particle, n, 'particle'), n, n_particles)
    if n_frames > 2 ** 31 - 3 or n > 2 ** 31 - 1:
        raise ValueError("too many frames or features for one call")
    as_tensor = _tables.is_tensor(pos)
    k, lag = int(k), int(lag)
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        group_t = None if group is None else _tables.on_device(group, dev, torch.int64, 'group')
        par_t = None if particle is None else _tables.on_device(particle, dev, torch.int64, 'particle')
        if par_t is not None and n_particles is None:
            n_particles = _tables.count_particles(par_t, n)
        dist = torch.empty((n, k), dtype=torch.float64, device=dev)
        dist2 = torch.empty((n, k), dtype=torch.float64, device=dev)
        index = torch.empty((n, k), dtype=torch.int64, device=dev)
        count = torch.empty(n, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        per_particle = ()
        if par_t is not None:
            per_particle = (torch.empty(n_particles, dtype=torch.float64, device=dev),
                            torch.empty(n_particles, dtype=torch.float64, device=dev))
        d = _abi.Neighbors()
        d.ndim, d.pairs, d.k, d.lag = ndim, _abi.PCF_PAIRS_CODES[pairs], k, lag
        d.n_frames, d.n_features, d.n_particles, d.limit2 = n_frames, n, n_particles or 0, limit2
        for a in range(ndim):
            d.mpp[a] = float(scale[a])
        d.pos, d.frame_offset = pos_t.data_ptr() or None, off_t.data_ptr()
        d.group = None if group_t is None else (group_t.data_ptr() or None)
        d.particle = None if par_t is None else (par_t.data_ptr() or None)
        d.dist, d.dist2, d.index, d.count = (x.data_ptr() or None for x in (dist, dist2, index, count))
        if per_particle:
            d.particle_min, d.particle_min2 = (x.data_ptr() or None for x in per_particle)
        d.status = status.data_ptr()
        eng.on_current_stream(eng.neighbors_device, d, dev=dev)
        out = _tables.results(as_tensor, status, _abi.NBR_OK, _NBR_REFUSED, dist, dist2, index, count, *per_particle)
        return Neighbors(*(tuple(out) + (() if per_particle else (None, None))), status if as_tensor else _abi.NBR_OK)


def neighbors(f, k=1, mpp=1., max_dist=None, group_column=None, pairs='all', lag=0, pos_columns=None,
              t_column='frame', device=0):
    """The nearest neighbours of every row of a table of features: ``(dist [len(f), k], neighbor
    [len(f), k], count [len(f)])`` in the row order of ``f`` -- the distances, the positions in ``f`` of
    the neighbours as for ``.iloc`` (-1 where there is none, the distance NaN) and the number of rows
    within ``max_dist``.  What ``cKDTree.query`` per frame gives a user of trackpy, by the module's rule;
    parity with trackpy is not pinned: it is not a dependency.

    f: a DataFrame with the position columns (default ``['y', 'x']``, with ``'z'`` in front where the
    table has one) and ``t_column``; no ``particle`` column is needed.  The frames are taken dense from
    the first to the last, so ``lag`` counts frame numbers.  group_column: an integer column such as
    ``'cluster'``, ``'particle'`` or ``'cluster_track'`` for ``pairs='same'`` / ``'other'``.  The other
    arguments as for :func:`neighbors_arrays`."""
    _pairs(pairs, group_column, 'group_column')
    order, offset, _, _, _, _, pos, *group = _tables.frame_sorted(
        f, pos_columns, t_column, () if group_column is None else (group_column,), particle=False)
    res = neighbors_arrays(pos, offset, k, mpp, max_dist, group[0] if group else None, pairs, lag, device=device)
    dist = np.empty_like(res.dist)
    neighbor = np.empty_like(res.index)
    count = np.empty_like(res.count)
    dist[order] = res.dist
    neighbor[order] = np.where(res.index >= 0, order[np.maximum(res.index, 0)], -1)
    count[order] = res.count
    return dist, neighbor, count


def proximity(f, mpp=1., pos_columns=None, t_column='frame', device=0):
    """The distance of every particle to its nearest neighbour, as trackpy's ``static.proximity`` gives
    it: a DataFrame indexed by ``particle`` with one column ``'proximity'``, the smallest same-frame
    nearest-neighbour distance over the particle's rows, in the units of ``pos * mpp``; NaN for a
    particle that was always alone in its frame.  By the module's rule (clause 8 of the neighbours);
    parity with trackpy is not pinned: it is not a dependency.

    f: a linked DataFrame with the position columns, ``t_column`` and ``'particle'``."""
    import pandas as pd
    _, offset, _, ids, dense, _, pos = _tables.frame_sorted(f, pos_columns, t_column)
    res = neighbors_arrays(pos, offset, 1, mpp, particle=dense, n_particles=len(ids), device=device)
    return pd.DataFrame({'proximity': res.particle_min}, index=pd.Index(ids, name='particle'))
