"""Shape coordinates of tracked clusters on the MI355X: the bonds, the opening angles and the radius
of gyration of every cluster in every frame, their distributions, and their displacement statistics
over a sweep of lags.  Everything ``motion`` reports assumes that a tracked cluster is a rigid body:
``orientation_arrays`` builds a basis from the features' positions and ``diffusion_tensor`` reads every
change of it as rotation; a cluster whose bonds breathe, or whose opening angle diffuses, gives a
clean-looking tensor anyway.  This is the check of that assumption, beside ``compute_drift``,
``vanhove``, ``pair_correlation`` and ``twopoint`` for the others, and the plain measurement that
comes with it: the bond length that ``constraints.dimer`` / ``trimer`` / ``tetramer`` take as ``dist``
is the first peak of ``P(bond)``.  The input is the block ``[T, F, n, ndim]`` of
``track_positions_arrays``, the second consumer of it beside ``motion.orientation_arrays``.

The reference has nothing of the kind; the rule is the project's own (``include/ctrefine.h`` has it in
full; ``tests/_shape.py`` restates it with plain loops).  No operation is contracted to a
fused multiply-add.

1. The coordinates of one (track, frame): ``C = NB + NA + 1`` of them, in this order (2, 7, 19 for
   ``n = 2, 3, 4``; :func:`shape_names`).  ``x[i, a] = pos[i, a] * mpp[a]``, rounded on its own.
   Bonds, ``NB = n (n - 1) / 2``, the pairs ``a < b`` in lexicographic order (``bond_ab``): ``bond =
   sqrt(sum over the axes, in axis order, of d * d)`` with ``d = x[b] - x[a]``, every product and sum
   rounded on its own, the root correctly rounded: NumPy's doubles bit for bit.  Angles, ``NA = n
   (n - 1) (n - 2) / 2``: for the vertex ``a`` ascending the pairs ``b < c`` of the other features in
   lexicographic order (``angle_a_bc``): ``u = x[b] - x[a]``, ``v = x[c] - x[a]``, ``dot = sum u_k
   v_k`` in axis order, ``cr = |u_0 v_1 - u_1 v_0|`` in 2D and the norm of the cross product in 3D,
   each component and each square rounded on its own; ``angle = atan2(cr, dot)`` in ``[0, pi]``;
   coincident features give what IEEE ``atan2`` gives (0), not an error.  Radius of gyration (``rg``,
   last): ``c_k = (sum_i x[i, k]) / n``, ``rg = sqrt((sum_i sum_k (x[i, k] - c_k)**2) / n)``, features
   outer, axes inner; bit for bit NumPy, like the bonds.  A frame with a non-finite ``x`` among its
   ``n ndim`` gives NaN in all ``C`` coordinates.
2. Dynamics, per track ``t``, coordinate ``c`` (value ``q``) and lag ``k``: the rows are the frames
   ``b`` with ``q[b]`` and ``q[b + k]`` both finite, ``d = q[b + k] - q[b]``; ``n`` counts them,
   ``mean_d``, ``mean_d2``, ``mean_d4 = mean((d d)**2)`` are their means, NaN where ``n == 0`` or the
   lag is beyond the video; ``flex = mean_d2 * 0.5 * fps / k``, the scaling of ``diffusion_tensor``:
   the joint flexibility of an angle, the breathing diffusivity of a bond.  The pooled outputs are the
   same from the sums of the tracks added in track order.  Static moments per ``(t, c)`` over the
   frames with a finite ``q``: ``n_frames``, ``mean``, ``var = mean((q - mean)**2)`` in two passes,
   ``min``, ``max``.  A rigid cluster has ``var`` of its bonds and angles at the localisation noise and
   ``flex -> 0`` at long lags.  No float atomics and a fixed order of the sums: a (track, coordinate,
   lag) gives the same bytes alone, inside a batch of tracks, inside a sweep of lags and on any stream.
3. Distributions: ``B = ceil(bond_max / bond_dr) <= _abi.SHAPE_MAX_BOND_BINS`` bond bins with the edges
   ``np.arange(B + 1) * bond_dr``, ``A = angle_bins <= _abi.SHAPE_MAX_ANGLE_BINS`` angle bins with the
   edges ``np.linspace(0, pi, A + 1)``, computed on the host and handed over; a value is in bin ``b``
   iff ``edges[b] <= v < edges[b + 1]``, decided by comparison with the edges; the last angle bin is
   closed at pi; bonds and ``rg`` at or above the last edge count in ``above``; a NaN is nowhere.  All
   counts are int64 and exact, and on every row ``count.sum() + above == n``, the frames that entered.
   ``density = count / (n * width)`` with the widths ``bond_dr`` and ``pi / A``.

Slots follow the order of ``particle``, so between tracks they are arbitrary: which bond of a trimer is
``bond_01`` differs from track to track.  The counts and the means are returned so that a caller can
pool slots.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import collections
import math

import numpy as np

from . import _abi, _tables
from .motion import _lag_list
from .static import _scales

Shape = collections.namedtuple('Shape', ['coords', 'names'])
ShapeDynamics = collections.namedtuple('ShapeDynamics', [
    'lags', 'names', 'n', 'mean_d', 'mean_d2', 'mean_d4', 'flex', 'pooled_n', 'pooled_mean_d', 'pooled_mean_d2',
    'pooled_mean_d4', 'pooled_flex', 'n_frames', 'mean', 'var', 'min', 'max'])
ShapeHistogram = collections.namedtuple('ShapeHistogram', [
    'names_bond', 'names_angle', 'bond_edges', 'angle_edges', 'count_bond', 'above', 'count_angle', 'n', 'density_bond',
    'density_angle'])

STATS = ('n', 'mean_d', 'mean_d2', 'mean_d4', 'flex')


def _check_geometry(cluster_size, ndim):
    if isinstance(ndim, bool) or ndim not in (2, 3):
        raise ValueError("ndim must be 2 or 3, not %r" % (ndim,))
    if isinstance(cluster_size, bool) or cluster_size not in (2, 3, 4):
        raise ValueError("cluster_size must be 2, 3 or 4, not %r" % (cluster_size,))
    return int(cluster_size), int(ndim)


def shape_names(cluster_size):
    """The names of the ``C`` coordinates of rule 1, in their order: ``bond_ab`` for ``a < b``, ``angle_a_bc``
    for the vertex ``a`` and ``b < c``, ``rg``."""
    n, _ = _check_geometry(cluster_size, 2)
    bonds = ['bond_%d%d' % (a, b) for a in range(n) for b in range(a + 1, n)]
    angles = ['angle_%d_%d%d' % (a, b, c) for a in range(n) for b in range(n) for c in range(b + 1, n)
              if a not in (b, c)]
    return tuple(bonds + angles + ['rg'])


def _block(pos, cluster_size, ndim, mpp):
    """the checks the three calls share: (pos, as_tensor, n, ndim, T, F, scale, names)"""
    n, ndim = _check_geometry(cluster_size, ndim)
    as_tensor = _tables.is_tensor(pos)
    if not as_tensor:
        pos = np.asarray(pos)
        if pos.dtype.kind not in 'fiu':
            raise ValueError("pos must hold numbers, not %s" % pos.dtype)
        pos = np.ascontiguousarray(pos, dtype=np.float64)
    if len(pos.shape) != 4 or pos.shape[2] != n or pos.shape[3] != ndim:
        raise ValueError("pos must be [T, F, cluster_size = %d, ndim = %d], not %s" % (n, ndim, tuple(pos.shape)))
    scale = _scales(mpp, ndim)
    return pos, as_tensor, n, ndim, int(pos.shape[0]), int(pos.shape[1]), scale, shape_names(n)


def _set_block(d, n, ndim, n_tracks, n_frames, scale, pos_t):
    d.ndim, d.cluster_size, d.n_tracks, d.n_frames = ndim, n, n_tracks, n_frames
    for a in range(ndim):
        d.mpp[a] = float(scale[a])
    d.pos = pos_t.data_ptr() or None


def _out(as_tensor, *tensors):
    return tensors if as_tensor else tuple(x.cpu().numpy() for x in tensors)


def shape_arrays(pos, cluster_size, ndim, mpp=1., device=0):
    """The shape coordinates of every (track, frame) (``ctr_shape_device``; rule 1 of the module).

    pos: ``[T, F, cluster_size, ndim]`` float64 in pixels, (z,) y, x, the block of
    ``track_positions_arrays``: NaN where the cluster is not complete.  cluster_size 2, 3 or 4, ndim 2
    or 3; the 2D tetramer is accepted.  mpp: microns per pixel, a number or one per axis.
    Returns ``Shape(coords [T, F, C], names)``: an ndarray for an ndarray ``pos``, a tensor on
    ``cuda:device`` (no host copy, no wait) for a tensor."""
    pos, as_tensor, n, ndim, n_tracks, n_frames, scale, names = _block(pos, cluster_size, ndim, mpp)
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        coords = torch.empty((n_tracks, n_frames, len(names)), dtype=torch.float64, device=dev)
        if n_tracks * n_frames:
            d = _abi.Shape()
            _set_block(d, n, ndim, n_tracks, n_frames, scale, pos_t)
            d.coords = coords.data_ptr()
            eng.on_current_stream(eng.shape_device, d, dev=dev)
        return Shape(_out(as_tensor, coords)[0], names)


def dynamics_descriptor(cluster_size, ndim, n_tracks, n_frames, n_lags, fps=1.):
    """An ``_abi.ShapeDynamics`` with its scalars (no pointers): what ``_lib.shape_plan`` takes."""
    d = _abi.ShapeDynamics()
    d.ndim, d.cluster_size, d.n_tracks, d.n_frames, d.n_lags, d.fps = ndim, cluster_size, n_tracks, n_frames, n_lags, fps
    for a in range(_abi.MAX_NDIM):
        d.mpp[a] = 1.
    return d


def shape_dynamics_arrays(pos, cluster_size, ndim, lagtime, mpp=1., fps=1., device=0):
    """Displacement statistics of the shape coordinates over a sweep of lags, and their static moments
    (``ctr_shape_dynamics_device``; rule 2 of the module).

    pos, cluster_size, ndim, mpp as for :func:`shape_arrays`.  lagtime: an int or a sequence of ints
    ``>= 1``, in frames (a scalar is a sweep of one); fps: frames per second.
    Returns ``ShapeDynamics(lags int64 [L], names, n int64 [T, C, L], mean_d, mean_d2, mean_d4, flex,
    pooled_n int64 [C, L], pooled_mean_d, pooled_mean_d2, pooled_mean_d4, pooled_flex, n_frames int64
    [T, C], mean, var, min, max)``: ndarrays for an ndarray ``pos``, tensors on ``cuda:device`` (no host
    copy, no wait) for a tensor.  Where ``n == 0`` the means are NaN."""
    _, lags = _lag_list(lagtime)
    if not (isinstance(fps, (int, float, np.integer, np.floating)) and math.isfinite(fps) and fps > 0):
        raise ValueError("fps must be positive")
    pos, as_tensor, n, ndim, n_tracks, n_frames, scale, names = _block(pos, cluster_size, ndim, mpp)
    C, L = len(names), len(lags)
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        lag_t = torch.from_numpy(lags).to(dev)
        i64 = dict(dtype=torch.int64, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        cnt = torch.empty((n_tracks, C, L), **i64)
        mean_d, mean_d2, mean_d4, flex = (torch.empty((n_tracks, C, L), **f64) for _ in range(4))
        pooled_n = torch.empty((C, L), **i64)
        pooled = [torch.empty((C, L), **f64) for _ in range(4)]
        present = torch.empty((n_tracks, C), **i64)
        moments = [torch.empty((n_tracks, C), **f64) for _ in range(4)]
        d = _abi.ShapeDynamics()
        _set_block(d, n, ndim, n_tracks, n_frames, scale, pos_t)
        d.n_lags, d.fps, d.lags = L, float(fps), lag_t.data_ptr() or None
        d.n, d.mean_d, d.mean_d2 = cnt.data_ptr() or None, mean_d.data_ptr() or None, mean_d2.data_ptr() or None
        d.mean_d4, d.flex = mean_d4.data_ptr() or None, flex.data_ptr() or None
        d.pooled_n = pooled_n.data_ptr() or None
        d.pooled_mean_d, d.pooled_mean_d2, d.pooled_mean_d4, d.pooled_flex = (x.data_ptr() or None for x in pooled)
        d.count = present.data_ptr() or None
        d.mean, d.var, d.min, d.max = (x.data_ptr() or None for x in moments)
        eng.on_current_stream(eng.shape_dynamics_device, d, dev=dev)
        out = _out(as_tensor, lag_t, cnt, mean_d, mean_d2, mean_d4, flex, pooled_n, *pooled, present, *moments)
        return ShapeDynamics(out[0], names, *out[1:])


def bins(bond_max, bond_dr, angle_bins):
    """rule 3: ``(B, bond_edges [B + 1], A, angle_edges [A + 1], angle_width)``, the edges float64 ndarrays"""
    bond_max, bond_dr = _tables.positive(bond_max, 'bond_max'), _tables.positive(bond_dr, 'bond_dr')
    if bond_max / bond_dr > _abi.SHAPE_MAX_BOND_BINS:
        raise ValueError("bond_max / bond_dr gives more than %d bins" % _abi.SHAPE_MAX_BOND_BINS)
    n_bond = max(int(math.ceil(bond_max / bond_dr)), 1)      # 1 where the quotient underflows to 0
    if isinstance(angle_bins, bool) or int(angle_bins) != angle_bins or not 1 <= angle_bins <= _abi.SHAPE_MAX_ANGLE_BINS:
        raise ValueError("angle_bins must be an integer in [1, %d], not %r" % (_abi.SHAPE_MAX_ANGLE_BINS, angle_bins))
    n_angle = int(angle_bins)
    return (n_bond, np.arange(n_bond + 1, dtype=np.float64) * bond_dr, n_angle, np.linspace(0., np.pi, n_angle + 1),
            np.pi / n_angle)


def shape_histogram_arrays(pos, cluster_size, ndim, bond_max, bond_dr, angle_bins, mpp=1., per_track=False, device=0):
    """The distributions of the shape coordinates (``ctr_shape_histogram_device``; rule 3 of the module).

    pos, cluster_size, ndim, mpp as for :func:`shape_arrays`.  bond_max, bond_dr: the reach and the bin
    width of the bonds and of ``rg``, in the units of ``pos * mpp``; angle_bins: the bins of ``[0, pi]``.
    Returns ``ShapeHistogram(names_bond, names_angle, bond_edges [B + 1], angle_edges [A + 1], count_bond int64
    [NB + 1, B] (rg last), above int64 [NB + 1], count_angle int64 [NA, A], n int64 [1], density_bond,
    density_angle)``; ``per_track=True`` puts a leading ``T`` on the counts, ``above``, ``n`` and the
    densities.  ``P(angle)`` is the free-energy landscape of a joint; the first peak of ``P(bond)`` is the
    ``dist`` of ``constraints``.  ndarrays for an ndarray ``pos``, tensors (no host copy, no wait) for a tensor."""
    n_bond, bond_edges, n_angle, angle_edges, angle_width = bins(bond_max, bond_dr, angle_bins)
    pos, as_tensor, n, ndim, n_tracks, n_frames, scale, names = _block(pos, cluster_size, ndim, mpp)
    nb, na = n * (n - 1) // 2, len(names) - 1 - n * (n - 1) // 2
    lead = (n_tracks,) if per_track else ()
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        be_t, ae_t = torch.from_numpy(bond_edges).to(dev), torch.from_numpy(angle_edges).to(dev)
        i64 = dict(dtype=torch.int64, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        count_bond, density_bond = torch.empty(lead + (nb + 1, n_bond), **i64), torch.empty(lead + (nb + 1, n_bond), **f64)
        above = torch.empty(lead + (nb + 1,), **i64)
        count_angle, density_angle = torch.empty(lead + (na, n_angle), **i64), torch.empty(lead + (na, n_angle), **f64)
        entered = torch.empty(lead or (1,), **i64)
        d = _abi.ShapeHistogram()
        _set_block(d, n, ndim, n_tracks, n_frames, scale, pos_t)
        d.per_track, d.bond_bins, d.angle_bins = int(bool(per_track)), n_bond, n_angle
        d.bond_dr, d.angle_width = float(bond_dr), float(angle_width)
        d.bond_edges, d.angle_edges = be_t.data_ptr(), ae_t.data_ptr()
        d.count_bond, d.above, d.n = count_bond.data_ptr() or None, above.data_ptr() or None, entered.data_ptr() or None
        d.density_bond = density_bond.data_ptr() or None
        d.count_angle, d.density_angle = count_angle.data_ptr() or None, density_angle.data_ptr() or None
        eng.on_current_stream(eng.shape_histogram_device, d, dev=dev)
        out = _out(as_tensor, be_t, ae_t, count_bond, above, count_angle, entered, density_bond, density_angle)
        return ShapeHistogram(names[:nb] + names[-1:], names[nb:-1], *out)


def _table_block(f, cluster_size, min_frames, pos_columns, t_column, device):
    from .cluster_tracks import track_positions
    block, track_ids, first = track_positions(f, cluster_size, min_frames, pos_columns, t_column, device)
    return block, track_ids, first, int(block.shape[3])


def shape_df(f, cluster_size, mpp=1., min_frames=1, pos_columns=None, t_column='frame', device=0):
    """The shape coordinates of a linked, labelled table: a DataFrame indexed by ``(cluster_track,
    frame)`` with the columns :func:`shape_names`, the complete frames only.

    f: the DataFrame that :func:`clustertracking_amd.cluster_tracks` takes (``particle`` and
    ``cluster`` columns); the tracks are those of ``cluster_tracks.track_positions(f, cluster_size,
    min_frames, pos_columns, t_column)``, the coordinates :func:`shape_arrays` of its block."""
    import pandas as pd
    n, _ = _check_geometry(cluster_size, 2)
    block, track_ids, first, ndim = _table_block(f, n, min_frames, pos_columns, t_column, device)
    res = shape_arrays(block, n, ndim, mpp, device)
    whole = np.isfinite(block).all((2, 3))
    t, b = np.nonzero(whole)
    index = pd.MultiIndex.from_arrays([track_ids[t], b + first], names=['cluster_track', t_column])
    return pd.DataFrame(res.coords[t, b], index=index, columns=list(res.names))


def flexibility(f, cluster_size, lagtime, mpp=1., fps=1., min_frames=1, pos_columns=None, t_column='frame', device=0):
    """The displacement statistics of the shape coordinates of a linked, labelled table: a DataFrame
    indexed by ``(cluster_track, lag)`` whose columns are a MultiIndex ``(coordinate, stat)`` with the
    stats ``n``, ``mean_d``, ``mean_d2``, ``mean_d4``, ``flex`` of :func:`shape_dynamics_arrays`.

    f, cluster_size, min_frames, pos_columns, t_column as for :func:`shape_df`; lagtime, mpp, fps as for
    :func:`shape_dynamics_arrays`, which also returns the pooled outputs and the static moments."""
    import pandas as pd
    n, _ = _check_geometry(cluster_size, 2)
    _lag_list(lagtime)
    block, track_ids, _, ndim = _table_block(f, n, min_frames, pos_columns, t_column, device)
    res = shape_dynamics_arrays(block, n, ndim, lagtime, mpp, fps, device)
    T, C, L = res.n.shape
    index = pd.MultiIndex.from_product([track_ids, res.lags], names=['cluster_track', 'lag'])
    columns = pd.MultiIndex.from_product([res.names, STATS], names=['coordinate', 'stat'])
    values = np.stack([getattr(res, s).astype(np.float64) for s in STATS], -1)        # [T, C, L, S]
    return pd.DataFrame(values.transpose(0, 2, 1, 3).reshape(T * L, C * len(STATS)), index=index, columns=columns)
