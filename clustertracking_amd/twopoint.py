"""Two-point displacement correlations of linked particles on the MI355X: whether particles move
*together*, as a function of their separation.  ``motion.diffusion_tensor`` treats every cluster track as
freely diffusing, and ``pairs='other'`` of g(r) and the neighbours (``static``) says how close other
clusters come, not whether the motion is coupled; the two-point displacement correlation tensor answers
that.  Its longitudinal part ``D_rr(r, tau)`` and its transverse part ``D_theta_theta(r, tau)`` are the
basis of two-point microrheology (Crocker et al. 2000): ``D_rr`` decays as ``1 / r`` under hydrodynamic
coupling.  A residual drift shows as a constant ``|v|^2 tau^2`` at every ``r``, wrong links show in the
first bins, and with the cluster labels as ``group``, ``pairs='same'`` is the rigid-body correlation
inside a cluster and ``pairs='other'`` the coupling between clusters.  The reference leaves this to
trackpy (``motion.velocity_corr`` / ``direction_corr``); here it is an all-pairs walk per frame and lag
with four exact integer accumulations per pair, on the tensors that ``find_link_arrays`` and
``subtract_drift_arrays`` already hold.

The rule is the project's own dense rule (``include/ctrefine.h`` has it too, DESIGN.md 7b;
``tests/_twopoint.py`` restates it in NumPy with Python integers):

1. Bins.  Clause 1 of g(r): ``static.bins(cutoff, dr, ndim)``, with ``B <= _abi.TP_MAX_BINS``; ``edge2`` is
   computed on the host.
2. Scaling and existence.  ``q = pos * mpp`` per axis, one rounding.  A row exists when every coordinate
   of ``q`` is finite.  There is no box.
3. Lags.  ``lagtime`` is an int or an ascending list of distinct ints ``>= 1``, at most
   ``_abi.TP_MAX_LAGS`` per call.
4. Partner.  The partner of row ``i`` of frame ``t`` at lag ``k`` is the lowest row ``j`` of frame ``t + k``
   with ``particle[j] == particle[i] >= 0``; there is none when ``t + k >= T`` or ``particle[i] < 0``.  This
   is drift's rule for a repeated particle.
5. Displacement.  ``u_a = q_partner,a - q_i,a``; ``u2`` is the sum over the axes, in axis order, of ``u_a *
   u_a``, every product and sum rounded on its own.  Row ``i`` has *moved* at lag ``k`` when it exists, its
   partner exists and ``u2 <= max2``; ``max2 = max_disp * max_disp`` is computed once on the host.
   ``n_moved[k]`` counts the moved rows, ``beyond[k]`` the rows with a finite ``u`` and ``u2 > max2``.  Rows
   outside ``[frame_offset[0], frame_offset[T])`` take no part.
6. Pairs.  A pair is an ordered pair ``(i, j)``, ``j != i``, of rows of one frame that have both moved at
   lag ``k``, with ``0 < d2 < edge2[B]``; ``d2`` and the bin follow clause 7 of g(r).  Coincident rows are
   not pairs, because ``L`` below divides by ``d2``.  ``pairs='same'`` / ``'other'`` with ``group`` follow
   clause 6 of g(r).
7. Per pair, every product and sum rounded on its own: ``R_a = q_j,a - q_i,a``, the differences that
   ``d2`` squares; ``dot`` is the sum over the axes of ``u_i,a * u_j,a``; ``a_i`` that of ``u_i,a * R_a`` and
   ``a_j`` of ``u_j,a * R_a``; ``L = (a_i * a_j) / d2``; ``c = dot / sqrt(u2_i * u2_j)`` where that product is
   ``> 0``, else 0.
8. Fixed point.  ``e`` is the smallest integer with ``2^e >= max2``; ``unit = 2^(e - 40)`` and ``unit_cos =
   2^-40``.  A value ``x`` enters as the integer ``rint(x / unit)``, ties to even; the scaling is exact.
9. Sums.  ``n[k, b]`` counts the pairs, exact int64.  ``sums[k, b, s]``, with ``s`` = dot, L, c, are the
   exact integer sums, each a 128-bit two's-complement number in two int64 words ``(hi, lo)``.  Integer
   addition commutes, so the order of the pairs cannot matter: no float atomics, no float sum at all.
10. Means.  A sum that fits int64 (``hi`` is the sign extension of ``lo``) is converted from that int64
    with one rounding; a larger one is ``(double)hi * 2^64 + (double)(uint64)lo``.  Then ``dot[k, b] = (x *
    unit) / (double)n``, and likewise ``longitudinal`` and ``cos``.  ``transverse`` comes from the exact
    integer difference ``S_dot - S_L`` the same way, divided also by ``ndim - 1``: the mean per transverse
    axis.  NaN where ``n == 0``.
11. A refused table.  A ``frame_offset`` that does not rise within ``[0, N]`` or a ``particle[i] >= P``:
    ``status[0] = _abi.TP_BAD_TABLE``, float outputs NaN, integers 0; ``ValueError`` for ndarrays.

So ``(i, j)`` and ``(j, i)`` give the same three integers (``a_i`` and ``a_j`` swap and change sign
exactly): ``n`` and every sum are even; and ``S_all == S_same + S_other`` as integers.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import collections
import math

import numpy as np

from . import _abi, _tables, static

TwoPoint = collections.namedtuple('TwoPoint', ['r_edges', 'lags', 'n', 'dot', 'longitudinal', 'transverse', 'cos', 'sums',
                                               'n_moved', 'beyond', 'unit', 'status'])

_REFUSED = "twopoint_arrays: frame_offset must rise within [0, N] and particle must be below n_particles"


def _lags(lagtime):
    """clause 3: the lags as a list of ints"""
    if isinstance(lagtime, np.ndarray):
        lagtime = lagtime.tolist()
    given = list(lagtime) if isinstance(lagtime, (list, tuple)) else [lagtime]
    if not all(isinstance(k, (int, float, np.integer, np.floating)) and math.isfinite(k) for k in given):
        raise ValueError("lagtime must be an integer >= 1 or a list of them, not %r" % (lagtime,))
    lags = [_tables.integer(k, 1, 'lagtime') for k in given]
    if not 1 <= len(lags) <= _abi.TP_MAX_LAGS:
        raise ValueError("lagtime must hold 1 to %d lags, not %d" % (_abi.TP_MAX_LAGS, len(lags)))
    if max(lags) > 2 ** 31 - 3:
        raise ValueError("lagtime must be below 2^31 - 2")
    if any(b <= a for a, b in zip(lags, lags[1:])):
        raise ValueError("lagtime must be ascending and distinct, not %r" % (lagtime,))
    return lags


def fixed_point(max_disp):
    """clauses 5 and 8: ``(max2, e, unit)``"""
    if max_disp is None or max_disp is Ellipsis:
        raise ValueError("max_disp is required: the largest displacement of a row that takes part")
    max_disp = _tables.positive(max_disp, 'max_disp')
    max2 = max_disp * max_disp
    if not _abi.TP_MAX2_RANGE[0] <= max2 <= _abi.TP_MAX2_RANGE[1]:
        raise ValueError("max_disp squared must be within [2^-500, 2^500], not %r" % (max2,))
    m, x = math.frexp(max2)                # max2 = m * 2^x, m in [0.5, 1)
    e = x - 1 if m == 0.5 else x
    return max2, e, math.ldexp(1., e - 40)


def _bins(cutoff, dr, ndim):
    cutoff, dr = _tables.positive(cutoff, 'cutoff'), _tables.positive(dr, 'dr')
    if cutoff / dr > _abi.TP_MAX_BINS:
        raise ValueError("cutoff / dr gives more than %d bins" % _abi.TP_MAX_BINS)
    r_edges, edge2, _ = static.bins(cutoff, dr, ndim)
    return r_edges, edge2


def _limits(cutoff, dr, ndim, max_disp):
    """clauses 1, 5 and 8 together: ``(r_edges, edge2, max2, unit)``; ``|a_i * a_j| <= u2 * d2 < max2 * edge2[B]``
    has to stay finite, so that every integer of clause 8 stays below ``2^41``"""
    r_edges, edge2 = _bins(cutoff, dr, ndim)
    max2, _, unit = fixed_point(max_disp)
    if not edge2[-1] * max2 <= _abi.TP_MAX_REACH2_MAX2:
        raise ValueError("cutoff squared times max_disp squared must be at most 2^1000, not %r" % (edge2[-1] * max2,))
    return r_edges, edge2, max2, unit


def twopoint_arrays(pos, frame_offset, particle, lagtime, cutoff, dr=0.5, max_disp=None, mpp=1., group=None, pairs='all',
                    n_particles=None, device=0):
    """The two-point displacement correlations of a linked table at one or several lags, binned by the
    distance of the pair and pooled over all frames (``ctr_twopoint_device``; the module's rule, where
    trackpy has ``velocity_corr`` / ``direction_corr`` for two frames).  Subtract the drift first
    (``subtract_drift_arrays``): a common velocity ``v`` adds ``|v|^2 lag^2`` to ``dot`` in every bin.

    pos float64 ``[N, ndim]``, ndim 2 or 3, rows sorted by frame; frame_offset int64 ``[T + 1]``; particle
    int64 ``[N]``, dense ids ``0 .. P - 1``, negative = unlinked: what ``find_link_arrays``, ``link_arrays``
    and ``subtract_drift_arrays`` produce, as ndarrays or as tensors on ``cuda:device``.  lagtime: an int,
    or an ascending list of at most ``_abi.TP_MAX_LAGS`` distinct ints ``>= 1``, in frames.  cutoff, dr: the
    largest distance of a pair and the bin width, in the units of ``pos * mpp``; at most
    ``_abi.TP_MAX_BINS`` bins.  max_disp (required): rows that moved further take no part and are counted
    in ``beyond``; it also sets the unit of the sums; its square lies within ``[2^-500, 2^500]`` and ``cutoff^2 *
    max_disp^2 <= 2^1000``, so that no product of a pair overflows.  mpp: microns per pixel, a number or one per axis.
    group: int64 ``[N]``, e.g. the cluster labels; pairs: ``'all'``, ``'same'`` (both rows of one group
    ``>= 0``) or ``'other'``.  n_particles: P; default ``particle.max() + 1``, which for a tensor is one
    host read; with tensors and a given P nothing is read back and nothing waits.

    Returns ``TwoPoint(r_edges [B + 1], lags int64 [K], n int64 [K, B], dot [K, B], longitudinal [K, B],
    transverse [K, B], cos [K, B], sums int64 [K, B, 3, 2], n_moved int64 [K], beyond int64 [K], unit,
    status)``: ndarrays and an int for ndarrays, tensors (status: int32 ``[1]``) for a tensor ``pos``;
    ``unit`` is a float.  ``sums[k, b, s]`` is the exact sum ``hi * 2^64 + (lo mod 2^64)`` of dot, L and c
    in units of ``unit``, ``unit`` and ``2^-40``.  ``n`` counts ordered pairs: every pair twice.  A refused
    table raises ``ValueError`` for ndarrays; for tensors status is ``_abi.TP_BAD_TABLE``, the floats NaN
    and the integers 0.  The same bytes on every call."""
    lags = _lags(lagtime)
    pos, n, ndim = _tables.positions(pos)
    r_edges, edge2, max2, unit = _limits(cutoff, dr, ndim, max_disp)
    scale = static._scales(mpp, ndim)
    static._pairs(pairs, group)
    frame_offset, n_frames = _tables.offsets(frame_offset)
    particle, n_particles = _tables.particles(_tables.int64_column(particle, n, 'particle'), n, n_particles)
    if group is not None:
        group = _tables.int64_column(group, n, 'group')
    if n_frames > 2 ** 31 - 3 or n > 2 ** 31 - 1:
        raise ValueError("too many frames or features for one call")
    as_tensor = _tables.is_tensor(pos)
    n_lags, n_bins = len(lags), len(edge2) - 1
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        par_t = _tables.on_device(particle, dev, torch.int64, 'particle')
        group_t = None if group is None else _tables.on_device(group, dev, torch.int64, 'group')
        if n_particles is None:
            n_particles = _tables.count_particles(par_t, n)
        lags_t = torch.tensor(lags, dtype=torch.int64, device=dev)
        edges_t, edge2_t = (torch.from_numpy(x).to(dev) for x in (r_edges, edge2))
        i64 = dict(dtype=torch.int64, device=dev)
        count = torch.empty((n_lags, n_bins), **i64)
        dot, along, across, cos = (torch.empty((n_lags, n_bins), dtype=torch.float64, device=dev) for _ in range(4))
        sums = torch.empty((n_lags, n_bins, 3, 2), **i64)
        n_moved, beyond = torch.empty(n_lags, **i64), torch.empty(n_lags, **i64)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        d = _abi.TwoPoint()
        d.ndim, d.pairs, d.n_lags = ndim, _abi.PCF_PAIRS_CODES[pairs], n_lags
        d.n_bins, d.n_frames, d.n_features, d.n_particles = n_bins, n_frames, n, n_particles
        d.dr, d.max2 = float(dr), max2
        for a in range(ndim):
            d.mpp[a] = float(scale[a])
        for q, k in enumerate(lags):
            d.lag[q] = k
        d.pos, d.frame_offset = pos_t.data_ptr() or None, off_t.data_ptr()
        d.particle = par_t.data_ptr() or None
        d.group = None if group_t is None else (group_t.data_ptr() or None)
        d.edge2 = edge2_t.data_ptr()
        d.n, d.dot, d.longitudinal, d.transverse, d.cos = (x.data_ptr() for x in (count, dot, along, across, cos))
        d.sums, d.n_moved, d.beyond, d.status = sums.data_ptr(), n_moved.data_ptr(), beyond.data_ptr(), status.data_ptr()
        eng.on_current_stream(eng.twopoint_device, d, dev=dev)
        out = _tables.results(as_tensor, status, _abi.TP_OK, _REFUSED, edges_t, lags_t, count, dot, along, across, cos, sums,
                              n_moved, beyond)
        return TwoPoint(*out, unit, status if as_tensor else _abi.TP_OK)


def twopoint(f, lagtime, cutoff, dr, max_disp, mpp=1., group_column=None, pairs='all', pos_columns=None, t_column='frame',
             device=0):
    """The two-point displacement correlations of a linked table: for one ``lagtime`` a DataFrame indexed
    by ``r``, the left edge of the bin (``r_edges[:-1]``, as ``pair_correlation(per_frame=True)`` names its
    columns), with the columns ``n`` (ordered pairs), ``dot`` (the mean of ``u_i . u_j``), ``longitudinal``
    (``D_rr``: the mean of the product of the components along the line between the two), ``transverse``
    (the rest, per transverse axis) and ``cos`` (the mean cosine of the angle between the displacements);
    for a list of lags the same with a ``(lag, r)`` MultiIndex.  Subtract the drift first
    (``subtract_drift``): what is left of it adds ``|v|^2 lag^2`` to ``dot`` at every ``r``.

    Where this differs from trackpy's ``velocity_corr`` / ``direction_corr``, which return one value per
    pair of two given frames: it is binned by ``r`` and pooled over all frames, pairs are ordered (every
    pair counts twice, which leaves the means as they are), any lag is taken, not the next frame alone,
    and rows that moved further than ``max_disp`` are left out.  Parity with trackpy is not pinned: it is
    not a dependency.

    f: a DataFrame with the position columns (default ``['y', 'x']``, with ``'z'`` in front where the table
    has one), ``t_column`` and ``'particle'``; the frames are taken dense from the first to the last, so
    ``lagtime`` counts frame numbers.  group_column: an integer column such as ``'cluster'`` or
    ``'cluster_track'`` for ``pairs='same'`` / ``'other'``.  The other arguments as for
    :func:`twopoint_arrays`, which also returns the exact sums and the counts of the rows."""
    import pandas as pd
    one = not isinstance(lagtime, (list, tuple, np.ndarray))
    _lags(lagtime)
    static._pairs(pairs, group_column, 'group_column')
    ndim = len(pos_columns) if pos_columns is not None else (3 if 'z' in f else 2)
    fixed_point(max_disp)
    if ndim in (2, 3):
        _limits(cutoff, dr, ndim, max_disp)
        static._scales(mpp, ndim)
    _, offset, _, ids, dense, _, pos, *group = _tables.frame_sorted(
        f, pos_columns, t_column, () if group_column is None else (group_column,))
    res = twopoint_arrays(pos, offset, dense, lagtime, cutoff, dr, max_disp, mpp, group[0] if group else None, pairs,
                          n_particles=len(ids), device=device)
    columns = ['n', 'dot', 'longitudinal', 'transverse', 'cos']
    r = res.r_edges[:-1]
    if one:
        return pd.DataFrame({c: getattr(res, c)[0] for c in columns}, index=pd.Index(r, name='r'), columns=columns)
    index = pd.MultiIndex.from_product([res.lags, r], names=['lag', 'r'])
    return pd.DataFrame({c: getattr(res, c).reshape(-1) for c in columns}, index=index, columns=columns)
