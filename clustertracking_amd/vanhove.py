"""Van Hove displacement distributions of linked particles on the MI355X: the histogram of the
displacements at a lag, per coordinate and radial, pooled over all particles, with its first, second
and fourth moment.  Everything this package reports as a diffusion coefficient -- the monomer's D from
``emsd``, the tensor of ``motion.diffusion_tensor`` -- assumes that the displacements are Gaussian;
this is the check of that assumption, for which users of the reference take trackpy's
``motion.vanhove``: stuck particles and wrong links put weight in the tails, a residual drift shifts
the centre, and clusters near a wall or next to another cluster give heavy tails long before the MSD
bends.

The rule is the project's own dense rule (``include/ctrefine.h`` has it in full, DESIGN.md 7b;
``tests/_vanhove.py`` restates it with plain loops):

1. - 3. are clauses 1 to 3 of the MSD rule (``msd``'s text): of several rows of one frame with the same
   id ``>= 0`` only the lowest exists; rows ``i`` (frame ``t``) and ``j`` (frame ``t + k``) of one id
   ``>= 0`` are a pair of lag ``k`` whatever is missing in between; ``d_a = (pos[j, a] - pos[i, a]) *
   mpp_a``, the same double as there;
4. ``lagtime`` is an int or an ascending list of at most ``_abi.VANHOVE_MAX_LAGS`` distinct ints
   ``>= 1``;
5. bins per coordinate: ``H = ceil(max_disp / bin_width) <= _abi.VANHOVE_MAX_HALF_BINS``, ``edges[b] =
   (b - H) * bin_width`` for ``b = 0 .. 2 H``, computed on the host and handed to the device; ``d_a``
   is in bin ``b`` iff ``edges[b] <= d_a < edges[b + 1]``; ``d_a < edges[0]`` counts in ``below``,
   ``d_a >= edges[2 H]`` in ``above``; a NaN is in no bin and in neither tail;
6. radial bins: ``r_edges[b] = b * bin_width`` for ``b = 0 .. H``; ``d2`` is the sum over the axes, in
   axis order, of ``d_a * d_a``, every product and sum rounded on its own; the pair is in bin ``b`` iff
   ``r_edges[b]**2 <= d2 < r_edges[b + 1]**2``, and ``d2 >= r_edges[H]**2`` counts in ``above_r``;
7. ``n[k]`` counts the pairs of lag ``k``; all counts are int64 and exact, and on finite positions
   ``count[k, a].sum() + below[k, a] + above[k, a] == n[k] == count_r[k].sum() + above_r[k]``;
8. ``mean_d``, ``mean_d2``, ``mean_d4`` are the means over the pairs of ``d_a``, ``d_a**2`` and
   ``(d_a**2)**2``, summed in the order of the ensemble's MSD: ``mean_d`` and ``mean_d2`` are bit for
   bit those of ``emsd_arrays`` at the same lag;
9. ``alpha2 = mean_d4 / (3 * (mean_d2 * mean_d2)) - 1``: the one-dimensional non-Gaussian parameter, 0
   for a Gaussian;
10. ``density = count / (n[k] * bin_width)``; ``density_r = count_r / (n[k] * bin_width)``, per unit r,
    not divided by the shell; where ``n[k] == 0`` the densities, the means and ``alpha2`` are NaN and
    the counts 0;
11. a refused table (offsets not rising within ``[0, N]``, a particle ``>= P``) raises ``ValueError``
    for ndarrays; for tensors ``status[0]`` is ``_abi.VANHOVE_BAD_TABLE``, the floats NaN, the counts 0.

Where this differs from trackpy's ``vanhove``: bins are given by a width and a reach, not by a count
over the data's range; the tails are counted rather than dropped; the ensemble only (a histogram per
particle is ``P * B`` numbers and is not offered); all coordinates and the radial part come from one
call; several lags are taken in one call.  Parity with trackpy itself is not pinned by a test: it is
not a dependency.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import collections
import math

import numpy as np

from . import _abi, _tables

VanHove = collections.namedtuple('VanHove', ['lags', 'edges', 'r_edges', 'count', 'below', 'above', 'density',
                                             'count_r', 'above_r', 'density_r', 'n', 'mean_d', 'mean_d2', 'mean_d4',
                                             'alpha2', 'status'])

_REFUSED = "vanhove_arrays: frame_offset must rise within [0, N] and particle must be below n_particles"


def _lags(lagtime):
    """clause 4: the lags as a list of ints"""
    if isinstance(lagtime, np.ndarray):
        lagtime = lagtime.tolist()
    given = list(lagtime) if isinstance(lagtime, (list, tuple)) else [lagtime]
    if not all(isinstance(k, (int, float, np.integer, np.floating)) and math.isfinite(k) for k in given):
        raise ValueError("lagtime must be an integer >= 1 or a list of them, not %r" % (lagtime,))
    lags = [_tables.integer(k, 1, 'lagtime') for k in given]
    if not 1 <= len(lags) <= _abi.VANHOVE_MAX_LAGS:
        raise ValueError("lagtime must hold 1 to %d lags, not %d" % (_abi.VANHOVE_MAX_LAGS, len(lags)))
    if max(lags) > 2 ** 31 - 3:
        raise ValueError("lagtime must be below 2^31 - 2")
    if any(b <= a for a, b in zip(lags, lags[1:])):
        raise ValueError("lagtime must be ascending and distinct, not %r" % (lagtime,))
    return lags


def bins(bin_width, max_disp):
    """clauses 5 and 6: ``(H, edges [2 H + 1], r_edges [H + 1], edge2 [H + 1])`` as float64 ndarrays"""
    bin_width, max_disp = _tables.positive(bin_width, 'bin_width'), _tables.positive(max_disp, 'max_disp')
    if max_disp / bin_width > _abi.VANHOVE_MAX_HALF_BINS:
        raise ValueError("max_disp / bin_width gives more than %d bins on a side" % _abi.VANHOVE_MAX_HALF_BINS)
    half = max(int(math.ceil(max_disp / bin_width)), 1)      # 1 where the quotient underflows to 0
    edges = (np.arange(2 * half + 1, dtype=np.float64) - half) * bin_width
    r_edges = np.arange(half + 1, dtype=np.float64) * bin_width
    return half, edges, r_edges, r_edges * r_edges


def _scales(mpp, ndim):
    scale = np.asarray(mpp, dtype=np.float64)
    if scale.ndim == 0:
        scale = np.repeat(scale, ndim)
    if scale.shape != (ndim,) or not np.isfinite(scale).all():
        raise ValueError("mpp must be a finite number or one per axis (%d), not %r" % (ndim, mpp))
    return [float(x) for x in scale]


def vanhove_arrays(pos, frame_offset, particle, lagtime, bin_width, max_disp, mpp=1., n_particles=None, device=0):
    """The van Hove displacement distributions of the ensemble at one or several lags
    (``ctr_vanhove_device``; the module's rule, where trackpy has ``vanhove(..., ensemble=True)`` for
    one coordinate and one lag).

    pos float64 ``[N, ndim]``, ndim 2 or 3; frame_offset int64 ``[T + 1]``; particle int64 ``[N]``,
    dense ids ``0 .. P - 1``, negative = unlinked: what ``find_link_arrays``, ``link_arrays``,
    ``filter_stubs_arrays`` and ``subtract_drift_arrays`` produce, as ndarrays or as tensors on
    ``cuda:device``.  lagtime: an int, or an ascending list of at most ``_abi.VANHOVE_MAX_LAGS``
    distinct ints ``>= 1``, in frames.  bin_width, max_disp: the width of a bin and the reach of the
    histogram on either side of 0, in the units of ``pos * mpp``; ``H = ceil(max_disp / bin_width)`` is
    at most ``_abi.VANHOVE_MAX_HALF_BINS``.  mpp: microns per pixel, a number or one per axis.
    n_particles: P; default ``particle.max() + 1``, which for a tensor is one host read; with tensors
    and a given P nothing is read back: the lags and the edges go to the device, no result comes from it.

    Returns ``VanHove(lags int64 [K], edges [2 H + 1], r_edges [H + 1], count int64 [K, ndim, 2 H], below
    int64 [K, ndim], above int64 [K, ndim], density [K, ndim, 2 H], count_r int64 [K, H], above_r int64
    [K], density_r [K, H], n int64 [K], mean_d [K, ndim], mean_d2, mean_d4, alpha2, status)``: ndarrays
    and an int for ndarrays, tensors (status: int32 ``[1]``) for a tensor ``pos``.  A refused table
    raises ``ValueError`` for ndarrays; for tensors status is ``_abi.VANHOVE_BAD_TABLE``, the floats
    NaN and the counts 0.  Unlike trackpy's ``vanhove`` the displacements beyond ``max_disp`` are
    counted in ``below`` / ``above`` / ``above_r``, not dropped.  The same bytes on every call."""
    lags = _lags(lagtime)
    half, edges, r_edges, edge2 = bins(bin_width, max_disp)
    pos, n, ndim = _tables.positions(pos)
    scale = _scales(mpp, ndim)
    frame_offset, n_frames = _tables.offsets(frame_offset)
    particle, n_particles = _tables.particles(particle, n, n_particles)
    as_tensor = _tables.is_tensor(pos)
    n_lags = len(lags)
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        par_t = _tables.on_device(particle, dev, torch.int64, 'particle')
        if n_particles is None:
            n_particles = _tables.count_particles(par_t, n)
        # rows are in frame order: one stable sort by particle gives (particle, frame, row) order
        order = torch.sort(par_t, stable=True)[1] if n else par_t
        lags_t = torch.tensor(lags, dtype=torch.int64, device=dev)
        edges_t, r_edges_t, edge2_t = (torch.from_numpy(x).to(dev) for x in (edges, r_edges, edge2))
        i64 = dict(dtype=torch.int64, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        count, density = torch.empty((n_lags, ndim, 2 * half), **i64), torch.empty((n_lags, ndim, 2 * half), **f64)
        below, above = torch.empty((n_lags, ndim), **i64), torch.empty((n_lags, ndim), **i64)
        count_r, density_r = torch.empty((n_lags, half), **i64), torch.empty((n_lags, half), **f64)
        above_r, pairs = torch.empty(n_lags, **i64), torch.empty(n_lags, **i64)
        mean_d, mean_d2, mean_d4, alpha2 = (torch.empty((n_lags, ndim), **f64) for _ in range(4))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        d = _abi.Vanhove()
        d.ndim, d.n_lags, d.half_bins, d.bin_width = ndim, n_lags, half, float(bin_width)
        d.n_frames, d.n_features, d.n_particles = n_frames, n, n_particles
        for a in range(ndim):
            d.mpp[a] = scale[a]
        for q, k in enumerate(lags):
            d.lag[q] = k
        d.pos, d.frame_offset = pos_t.data_ptr() or None, off_t.data_ptr()
        d.particle, d.order = par_t.data_ptr() or None, order.data_ptr() or None
        d.edges, d.edge2 = edges_t.data_ptr(), edge2_t.data_ptr()
        d.count, d.below, d.above, d.density = count.data_ptr(), below.data_ptr(), above.data_ptr(), density.data_ptr()
        d.count_r, d.above_r, d.density_r, d.n = count_r.data_ptr(), above_r.data_ptr(), density_r.data_ptr(), pairs.data_ptr()
        d.mean_d, d.mean_d2, d.mean_d4, d.alpha2 = mean_d.data_ptr(), mean_d2.data_ptr(), mean_d4.data_ptr(), alpha2.data_ptr()
        d.status = status.data_ptr()
        eng.on_current_stream(eng.vanhove_device, d, dev=dev)
        out = _tables.results(as_tensor, status, _abi.VANHOVE_OK, _REFUSED, lags_t, edges_t, r_edges_t, count, below, above,
                              density, count_r, above_r, density_r, pairs, mean_d, mean_d2, mean_d4, alpha2)
        return VanHove(*out, status if as_tensor else _abi.VANHOVE_OK)


def vanhove(f, lagtime, mpp, bin_width, max_disp, pos_columns=None, t_column='frame', radial=False, device=0):
    """The van Hove displacement distribution of a linked table at one lag, indexed as trackpy's
    ``vanhove(..., ensemble=True)`` is: a DataFrame of the probability density of the displacement
    along every position column (one column each), indexed by the bin centres ``(edges[b] + edges[b
    + 1]) / 2``.  With ``radial=True`` a Series ``density_r`` of the displacement's length, per unit r,
    over the radial bin centres.

    f: a DataFrame with a ``particle`` column; the ids are used as they are, the frames from
    ``f[t_column]``'s minimum to its maximum as ``drift`` densifies them.  lagtime: one int, in frames;
    the other arguments as for :func:`vanhove_arrays`, which also returns the tails, the counts and
    the moments.  Unlike trackpy's ``vanhove`` the bins are given by ``bin_width`` and ``max_disp``,
    not by a count over the data's range, and the density is normalised by all pairs, those beyond
    ``max_disp`` included."""
    import pandas as pd
    if isinstance(lagtime, (list, tuple, np.ndarray)):
        raise ValueError("lagtime must be one integer >= 1, not %r; vanhove_arrays takes a list" % (lagtime,))
    _lags(lagtime)
    bins(bin_width, max_disp)
    ndim = len(pos_columns) if pos_columns is not None else (3 if 'z' in f else 2)
    if ndim in (2, 3):
        _scales(mpp, ndim)
    _, offset, _, ids, dense, pos_columns, pos = _tables.frame_sorted(f, pos_columns, t_column)
    res = vanhove_arrays(pos, offset, dense, lagtime, bin_width, max_disp, mpp, n_particles=len(ids), device=device)
    if radial:
        centres = (res.r_edges[:-1] + res.r_edges[1:]) / 2.
        return pd.Series(res.density_r[0], index=pd.Index(centres, name='r'), name='density_r')
    centres = (res.edges[:-1] + res.edges[1:]) / 2.
    return pd.DataFrame(res.density[0].T, index=pd.Index(centres, name='displacement'), columns=list(pos_columns))
