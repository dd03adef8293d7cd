"""Orientation and diffusion tensor of tracked clusters on the MI355X: the last stage of the
reference's pipeline (reference ``clustertracking/motion.py``), behind :func:`link_arrays`.

The rule is the reference's, restated (``include/ctrefine.h`` has it in full):

* orientation (``motion.py:40-162``): per frame the coordinates of the cluster's features, ordered
  by ``particle``, times ``mpp`` and reversed to x, y(, z); for every permutation of the features
  (the reference's tables: 2, 6, 12 entries for sizes 2, 3, 4) a centre of mass with the weights
  ``sizes**ndim`` -- which are NOT permuted with the coordinates -- and a right-handed basis of rows
  x, y, z.  A frame in which the cluster is not complete is NaN; so is a degenerate basis
  (coincident features, a collinear 3D trimer, a 3D dimer along ``[1, 0, 0]``): the reference's
  ``check_orthonormality`` assertion is not reproduced.  The 3D dimer's azimuth, which the
  reference draws from ``np.random`` per call, is the caller's ``angles``.
* diffusion tensor (``motion.py:165-198``): per permutation and frame ``b`` the 6-vector of the
  translation ``bases[b] (pos[b + lag] - pos[b])`` and the rotation
  ``0.5 sum_i e_i x (bases[b] bases[b + lag, i])``; rows with a non-finite component are dropped,
  the rest are pooled over the permutations; ``tensor = mean(x x^T) 0.5 fps / lag``.  Here one
  call takes every track and a whole sweep of lags, and a lag beyond the video gives a NaN tensor
  and count 0 instead of a warning.

The reference's ``diffusion_tensor_ci`` (``motion.py:201-216``), the bootstrap interval of that tensor,
is :func:`clustertracking_amd.motion_ci.diffusion_tensor_ci`, a module of its own.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import numpy as np

from . import _abi, _tables

# reference motion.py:137-145, in its order
PERMUTATIONS = {
    2: ((0, 1), (1, 0)),
    3: ((0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0), (0, 2, 1), (1, 0, 2)),
    4: ((0, 1, 2, 3), (0, 2, 3, 1), (0, 3, 1, 2), (1, 0, 2, 3), (1, 2, 3, 0), (1, 3, 0, 2),
        (2, 0, 1, 3), (2, 1, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2), (3, 1, 2, 0), (3, 2, 0, 1)),
}


def _check_geometry(cluster_size, ndim):
    if ndim not in (2, 3):
        raise ValueError("ndim must be 2 or 3, not %r" % (ndim,))
    if int(cluster_size) != cluster_size or not 1 <= cluster_size <= 4:
        raise ValueError("cluster_size must be 2, 3 or 4, not %r" % (cluster_size,))
    if cluster_size == 1:
        raise NotImplementedError("the orientation of a single particle (cluster_size=1) is random in the "
                                  "reference and is not implemented")
    if ndim == 2 and cluster_size == 4:
        raise NotImplementedError("the orientation of a 2D tetramer is not implemented (the reference "
                                  "refuses it too)")


def _weights(sizes, cluster_size, ndim):
    if sizes is None:
        return np.ones(cluster_size)
    sizes = np.asarray(sizes, dtype=np.float64).reshape(-1)
    if len(sizes) != cluster_size:
        raise ValueError("sizes must have cluster_size = %d entries, not %d" % (cluster_size, len(sizes)))
    if not np.isfinite(sizes).all():
        raise ValueError("sizes must be finite")
    return sizes ** ndim


def orientation_arrays(pos, cluster_size, ndim, mpp=1., sizes=None, angles=None, device=0):
    """Centre of mass and bases of tracked clusters (``ctr_orientation_device``).

    pos: ``[T, F, cluster_size, ndim]`` float64 in pixels, (z,) y, x, the features of a cluster in
    the order of their ``particle``; NaN where the cluster is not complete in a frame.  sizes:
    ``cluster_size`` feature sizes, the weights of the centre of mass are ``sizes**ndim`` (default:
    equal).  angles: ``[T, P, F]`` radians, required for 3D dimers (the azimuth the reference draws
    at random), ignored otherwise.
    Returns ``(com [T, F, 3], bases [T, P, F, 3, 3])`` in x, y, z order, the rows of a basis x, y, z;
    ndarrays for an ndarray ``pos``, tensors on ``cuda:device`` (no host copy) for a tensor."""
    _check_geometry(cluster_size, ndim)
    cluster_size = int(cluster_size)
    n_perm = len(PERMUTATIONS[cluster_size])
    as_tensor = _tables.is_tensor(pos)
    if not as_tensor:
        pos = np.asarray(pos, dtype=np.float64)
    if pos.ndim != 4 or pos.shape[2] != cluster_size or pos.shape[3] != ndim:
        raise ValueError("pos must be [T, F, cluster_size = %d, ndim = %d], not %s"
                         % (cluster_size, ndim, tuple(pos.shape)))
    n_tracks, n_frames = int(pos.shape[0]), int(pos.shape[1])
    weights = _weights(sizes, cluster_size, ndim)
    if not np.isfinite(mpp):
        raise ValueError("mpp must be finite")
    needs_angles = ndim == 3 and cluster_size == 2
    if needs_angles:
        if angles is None:
            raise ValueError("angles is required for 3D dimers: [T, P, F] radians, the azimuth that the "
                             "reference draws at random")
        if not _tables.is_tensor(angles):
            angles = np.asarray(angles, dtype=np.float64)
        if tuple(angles.shape) != (n_tracks, n_perm, n_frames):
            raise ValueError("angles must be [T, P, F] = %s, not %s"
                             % ((n_tracks, n_perm, n_frames), tuple(angles.shape)))
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        ang_t = _tables.on_device(angles, dev, torch.float64, 'angles') if needs_angles else None
        com = torch.empty((n_tracks, n_frames, 3), dtype=torch.float64, device=dev)
        bases = torch.empty((n_tracks, n_perm, n_frames, 3, 3), dtype=torch.float64, device=dev)
        if n_tracks * n_frames:
            d = _abi.Orientation()
            d.ndim, d.cluster_size, d.n_tracks, d.n_frames, d.mpp = ndim, cluster_size, n_tracks, n_frames, float(mpp)
            for k in range(cluster_size):
                d.weights[k] = float(weights[k])
            d.pos, d.com, d.bases = pos_t.data_ptr(), com.data_ptr(), bases.data_ptr()
            d.angles = ang_t.data_ptr() if needs_angles else None
            eng.on_current_stream(eng.orientation_device, d, dev=dev)
        if as_tensor:
            return com, bases
        return com.cpu().numpy(), bases.cpu().numpy()


def orientation_df(f, cluster_size=2, mpp=1., ndim=None, sizes=None, angles=None, track_column=None, device=0):
    """The reference's ``orientation_df`` on the MI355X (:func:`orientation_arrays`).

    f: DataFrame with ``frame``, ``cluster``, ``particle`` and the position columns.  Frames are
    counted from ``f['frame'].min()``; a frame contributes where a ``(frame, cluster)`` group has
    exactly ``cluster_size`` rows, and of several such groups in one frame the last one in sorted
    order wins, as in the reference.  Returns ``(com [length, 3], bases [P, length, 3, 3])``; angles
    (3D dimers) is ``[P, length]``.
    With ``track_column`` the groups are ``(track, frame, cluster)`` (the reference takes one track
    per call), the results gain a leading axis over the sorted track ids, angles is
    ``[T, P, length]``, and ``(com, bases, track_ids)`` is returned."""
    if ndim is None:
        ndim = 3 if 'z' in f else 2
    _check_geometry(cluster_size, ndim)
    pos_columns = ['y', 'x'] if ndim == 2 else ['z', 'y', 'x']
    cluster_size = int(cluster_size)
    n_perm = len(PERMUTATIONS[cluster_size])
    if len(f) == 0:
        raise ValueError("an empty table has no frames")
    start = int(f['frame'].min())
    length = int(f['frame'].max() - start) + 1
    keys = ([track_column] if track_column is not None else []) + ['frame', 'cluster']
    f = f.sort_values(keys + ['particle'], kind='stable')
    if track_column is not None:
        track_ids, track_of = np.unique(f[track_column].values, return_inverse=True)
    else:
        track_ids, track_of = None, np.zeros(len(f), dtype=np.int64)
    n_tracks = 1 if track_ids is None else len(track_ids)
    frame_of = f['frame'].values.astype(np.int64) - start
    cluster_of = f['cluster'].values
    coords = f[pos_columns].values.astype(np.float64)
    # the groups of the sorted table, and those of exactly cluster_size rows
    new = np.r_[True, (track_of[1:] != track_of[:-1]) | (frame_of[1:] != frame_of[:-1])
                | (cluster_of[1:] != cluster_of[:-1])]
    first = np.flatnonzero(new)
    count = np.diff(np.r_[first, len(f)])
    first = first[count == cluster_size]
    dense = np.full((n_tracks, length, cluster_size, ndim), np.nan)
    rows = first[:, None] + np.arange(cluster_size)[None, :]
    dense[track_of[first], frame_of[first]] = coords[rows]      # a repeated (track, frame): the last group stays
    if angles is not None and track_column is None:
        angles = np.asarray(angles, dtype=np.float64)
        if angles.shape != (n_perm, length):
            raise ValueError("angles must be [P, length] = %s, not %s" % ((n_perm, length), angles.shape))
        angles = angles[None]
    com, bases = orientation_arrays(dense, cluster_size, ndim, mpp, sizes, angles, device)
    if track_column is None:
        return com[0], bases[0]
    return com, bases, track_ids


def _lag_list(lagtime):
    scalar = np.ndim(lagtime) == 0
    lags = np.atleast_1d(np.asarray(lagtime))
    if lags.ndim != 1 or lags.dtype.kind not in 'iu' and not np.all(lags == np.floor(lags)):
        raise ValueError("lagtime must be an integer or a sequence of integers")
    lags = lags.astype(np.int64)
    if (lags < 1).any():
        raise ValueError("lagtime must be >= 1 (frames)")
    return scalar, lags


def diffusion_inputs(positions, orientations, lagtime, fps, ndim):
    """The arguments that :func:`diffusion_tensor` and ``motion_ci.diffusion_tensor_ci`` share, checked:
    ``(positions, orientations, as_tensor, scalar_lag, lags, tracked, n_tracks, n_frames, n_perm)``."""
    if ndim not in (2, 3):
        raise ValueError("ndim must be 2 or 3, not %r" % (ndim,))
    scalar_lag, lags = _lag_list(lagtime)
    if not (np.isfinite(fps) and fps > 0):
        raise ValueError("fps must be positive")
    as_tensor = _tables.is_tensor(positions) or _tables.is_tensor(orientations)
    if not _tables.is_tensor(positions):
        positions = np.asarray(positions, dtype=np.float64)
    if not _tables.is_tensor(orientations):
        orientations = np.asarray(orientations, dtype=np.float64)
    psh, osh = tuple(positions.shape), tuple(orientations.shape)
    tracked = len(psh) == 3
    if len(psh) not in (2, 3) or psh[-1] != 3:
        raise ValueError("positions must be [F, 3] or [T, F, 3], not %s" % (psh,))
    if osh[-2:] != (3, 3) or len(osh) not in ((5,) if tracked else (3, 4)):
        raise ValueError("orientations must be %s, not %s"
                         % ("[T, P, F, 3, 3]" if tracked else "[F, 3, 3] or [P, F, 3, 3]", osh))
    n_frames = psh[-2]
    n_tracks = psh[0] if tracked else 1
    n_perm = osh[-4] if len(osh) >= 4 else 1
    if osh[-3] != n_frames or (tracked and osh[0] != n_tracks):
        raise ValueError("positions %s and orientations %s do not describe the same tracks and frames" % (psh, osh))
    if n_perm < 1:
        raise ValueError("orientations hold no permutation")
    return positions, orientations, as_tensor, scalar_lag, lags, tracked, n_tracks, n_frames, n_perm


def diffusion_tensor(positions, orientations, lagtime=1, fps=1., ndim=3, pool_tracks=False, return_counts=False,
                     device=0):
    """Diffusion tensor from positions and bases (``ctr_diffusion_device``), for every track and
    every lag of a sweep in one call.

    positions: ``[F, 3]`` or ``[T, F, 3]``; orientations: ``[F, 3, 3]``, ``[P, F, 3, 3]`` or, with
    tracked positions, ``[T, P, F, 3, 3]`` (what :func:`orientation_arrays` returns).  lagtime: an
    int (frames), or a sequence, which adds a lag axis; ``lag >= F`` gives a NaN tensor.  ndim 2
    keeps x, y translation and z rotation (3 x 3), ndim 3 gives 6 x 6.
    Returns ``tensor [T][, n_lags], D, D``: with the reference's argument shapes the reference's
    shape.  ``pool_tracks``: the mean over the rows of all tracks (the count-weighted mean of the
    per-track tensors) instead of the track axis.  ``return_counts``: also the number of rows that
    entered each mean, int64 ``[T][, n_lags]``.  ndarrays in give ndarrays, tensors on
    ``cuda:device`` give tensors (no host copy)."""
    positions, orientations, as_tensor, scalar_lag, lags, tracked, n_tracks, n_frames, n_perm = diffusion_inputs(
        positions, orientations, lagtime, fps, ndim)
    D = 3 if ndim == 2 else 6
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(positions, dev, torch.float64, 'positions')
        ori_t = _tables.on_device(orientations, dev, torch.float64, 'orientations')
        lag_t = torch.from_numpy(lags).to(dev)
        tensor = torch.empty((n_tracks, len(lags), D, D), dtype=torch.float64, device=dev)
        counts = torch.empty((n_tracks, len(lags)), dtype=torch.int64, device=dev)
        if n_tracks * len(lags):
            d = _abi.Diffusion()
            d.ndim, d.n_perm, d.n_tracks, d.n_frames, d.n_lags, d.fps = ndim, n_perm, n_tracks, n_frames, len(lags), float(fps)
            d.lags, d.positions, d.bases = lag_t.data_ptr(), pos_t.data_ptr() or None, ori_t.data_ptr() or None
            d.tensor, d.n_samples = tensor.data_ptr(), counts.data_ptr()
            eng.on_current_stream(eng.diffusion_device, d, dev=dev)
        if tracked and pool_tracks:
            # mean over the pooled rows = count-weighted mean of the per-track means
            w = counts.to(torch.float64)[:, :, None, None]
            total = counts.sum(0)
            tensor = torch.where(w > 0, tensor * w, torch.zeros_like(tensor)).sum(0) / total.to(torch.float64)[:, None, None]
            counts = total
            tracked = False
        if not tracked:
            tensor, counts = tensor.reshape(tensor.shape[-3:]), counts.reshape(counts.shape[-1:])
        if scalar_lag:
            tensor, counts = tensor.select(-3, 0), counts.select(-1, 0)
        if not as_tensor:
            tensor, counts = tensor.cpu().numpy(), counts.cpu().numpy()
            if counts.ndim == 0:
                counts = int(counts)
    return (tensor, counts) if return_counts else tensor


def friction_tensor(diff_tens):
    """The friction tensor of a diffusion tensor: its inverse, on the host (as the reference's; for
    physical units multiply by eta / (kB T))."""
    d = np.asarray(diff_tens, dtype=np.float64)
    n = int(round(d.size ** 0.5))
    return np.linalg.inv(d.reshape(n, n))
