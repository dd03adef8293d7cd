"""Cluster tracks on the MI355X: which particles form one cluster over time, and the dense block of
tracked clusters that :func:`clustertracking_amd.motion.orientation_arrays` takes.  The step between
``find_link`` / ``link_arrays`` (a ``particle`` per feature) plus ``find_clusters`` (a ``cluster`` per
feature and frame) and the motion stage.

The rule is this project's own (``include/ctrefine.h`` has it in full; the reference's
``orientation_df`` assumes one cluster per table):

1. the rows of one frame with the same ``cluster`` value are a *complete group* when there are
   exactly ``cluster_size`` of them, all linked (``particle >= 0``) and of pairwise different
   particles; a group of any other size is no evidence;
2. two particles are *bonded* when they share a complete group in at least ``min_frames`` frames;
3. the connected components of the bond graph with at least two particles are the *tracks*,
   numbered by ascending smallest particle id;
4. for a track and a frame, the rows of the frame whose particle is a member -- whatever their
   ``cluster`` value -- are counted in ``present``; where that equals ``cluster_size`` their positions
   fill ``pos[k, t]`` in ascending (particle, row) order, anywhere else the cell is NaN
   (``present < cluster_size``: incomplete, ``present > cluster_size``: a conflict).

The ``cluster`` labels matter to 1 and 2 only: a dimer that touches a neighbour in a frame, or drifts
beyond ``separation``, keeps that frame.  ``motion.orientation_df(track_column=...)`` groups by
``(track, frame, cluster)`` and decides differently on such frames.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import collections

import numpy as np

from . import _abi, _lib, _tables

ClusterTracks = collections.namedtuple('ClusterTracks', ['track_of_particle', 'n_tracks', 'n_members', 'status'])
TrackPositions = collections.namedtuple('TrackPositions', ['pos', 'present'])

#: rounds between two looks of the host at the word of the last hook (0: all rounds queued blind)
CHECK_EVERY = 2


def _check_sizes(cluster_size, min_frames=1):
    if isinstance(cluster_size, bool) or int(cluster_size) != cluster_size or not 2 <= cluster_size <= 4:
        raise ValueError("cluster_size must be 2, 3 or 4, not %r" % (cluster_size,))
    if isinstance(min_frames, bool) or int(min_frames) != min_frames or min_frames < 1:
        raise ValueError("min_frames must be an integer >= 1, not %r" % (min_frames,))
    return int(cluster_size), int(min_frames)


def descriptor(phase, cluster_size, min_frames, n_frames, n_features, n_particles, check_every=0):
    """An ``_abi.ClusterTracks`` with its scalars (no pointers)."""
    d = _abi.ClusterTracks()
    d.phase, d.cluster_size, d.check_every, d.min_frames = phase, cluster_size, check_every, min_frames
    d.n_frames, d.n_features, d.n_particles = n_frames, n_features, n_particles
    return d


def round_bound(n_particles):
    """``(max_rounds, jumps_per_round)`` of the components for ``n_particles`` (``ctr_cluster_tracks_plan``)."""
    return _lib.cluster_tracks_plan(descriptor(_abi.TRACKS_COMPONENTS, 2, 1, 0, 0, int(n_particles)))[1:]


def cluster_tracks_arrays(frame_offset, particle, cluster, cluster_size, min_frames=1, device=0, n_particles=None,
                          check_every=None, return_rounds=False):
    """Tracks of clusters from linked, labelled rows (``ctr_cluster_tracks_device``).

    frame_offset ``[T + 1]``, rows ``[off[t], off[t + 1])`` are frame t; particle ``[N]``, dense ids
    ``0 .. P - 1``, negative = unlinked; cluster ``[N]``, any integers, equal within a frame = the same
    cluster.  All int64; ndarrays, or tensors on ``cuda:device`` (what ``find_link_arrays`` returns).
    n_particles: P; default ``particle.max() + 1``, which for a tensor is one more host read
    (``find_link_arrays`` returns it as ``n_tracks``).  check_every: rounds between two looks of the
    host at one word (default 2), 0 queues the whole round bound blind; the same bytes either way.
    Returns ``ClusterTracks(track_of_particle int32 [P], n_tracks, n_members int32 [n_tracks],
    status)``: ndarrays for ndarrays, tensors for tensors (``n_tracks`` and ``status`` are ints: one
    host copy of three words).  status: 0, ``_abi.TRACKS_BAD_TABLE`` (offsets not monotone within N, a
    particle >= P: nothing was followed, no track) or ``_abi.TRACKS_ROUNDS`` (the components did not
    settle within the round bound: no track).  return_rounds: also the rounds that hooked anything."""
    cluster_size, min_frames = _check_sizes(cluster_size, min_frames)
    check_every = CHECK_EVERY if check_every is None else int(check_every)
    if check_every < 0:
        raise ValueError("check_every must be >= 0")
    as_tensor = _tables.is_tensor(particle)
    frame_offset, n_frames = _tables.offsets(frame_offset)
    particle = _tables.column(particle, None, 'particle')
    n = int(particle.shape[0])
    cluster = _tables.column(cluster, n, 'cluster')
    particle, n_particles = _tables.particles(particle, n, n_particles)
    with _tables.stage(device) as (eng, dev):
        import torch
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        par_t = _tables.on_device(particle, dev, torch.int64, 'particle')
        clu_t = _tables.on_device(cluster, dev, torch.int64, 'cluster')
        if n_particles is None:
            n_particles = _tables.count_particles(par_t, n)
        keys = torch.empty(n * (cluster_size - 1), dtype=torch.int64, device=dev)
        track_of = torch.empty(n_particles, dtype=torch.int32, device=dev)
        members = torch.empty(n_particles // 2, dtype=torch.int32, device=dev)
        words = torch.zeros(4, dtype=torch.int32, device=dev)      # n_tracks, status, n_rounds
        d = descriptor(_abi.TRACKS_PAIRS, cluster_size, min_frames, n_frames, n, n_particles, check_every)
        d.frame_offset, d.particle, d.cluster = off_t.data_ptr(), par_t.data_ptr() or None, clu_t.data_ptr() or None
        d.keys = keys.data_ptr() or None
        d.status = words[1:].data_ptr()
        eng.on_current_stream(eng.cluster_tracks_device, d, dev=dev)
        keys = torch.sort(keys).values       # plumbing: equal keys side by side
        d.phase = _abi.TRACKS_COMPONENTS
        d.keys = keys.data_ptr() or None
        d.track_of_particle, d.n_members = track_of.data_ptr() or None, members.data_ptr() or None
        d.n_tracks, d.n_rounds = words.data_ptr(), words[2:].data_ptr()
        eng.on_current_stream(eng.cluster_tracks_device, d, dev=dev)
        n_tracks, status, n_rounds = (int(v) for v in words[:3].cpu())
        members = members[:n_tracks]
        if not as_tensor:
            track_of, members = track_of.cpu().numpy(), members.cpu().numpy()
    res = ClusterTracks(track_of, n_tracks, members, status)
    return (res, n_rounds) if return_rounds else res


def track_positions_arrays(pos, frame_offset, particle, track_of_particle, n_tracks, cluster_size, device=0):
    """The dense block of tracked clusters (``ctr_track_positions_device``).

    pos float64 ``[N, ndim]``; frame_offset, particle as in :func:`cluster_tracks_arrays`;
    track_of_particle int32 ``[P]`` and n_tracks from it.  Returns ``TrackPositions(pos [n_tracks, T,
    cluster_size, ndim], present int32 [n_tracks, T])``: ndarrays for an ndarray ``pos``, tensors on
    ``cuda:device`` (no host copy) for a tensor; such a ``pos`` goes straight into
    ``motion.orientation_arrays``.  A refused table (offsets, a particle >= P, a track >= n_tracks)
    raises ``ValueError`` for ndarrays; for tensors it leaves every cell NaN and ``present`` 0."""
    cluster_size, _ = _check_sizes(cluster_size)
    as_tensor = _tables.is_tensor(pos)
    pos, n, ndim = _tables.positions(pos)
    frame_offset, n_frames = _tables.offsets(frame_offset)
    particle = _tables.column(particle, n, 'particle')
    track_of_particle = _tables.column(track_of_particle, None, 'track_of_particle', np.int32)
    n_particles = int(track_of_particle.shape[0])
    if isinstance(n_tracks, bool) or int(n_tracks) != n_tracks or n_tracks < 0 or 2 * n_tracks > n_particles:
        raise ValueError("n_tracks must be an integer in [0, P / 2], not %r" % (n_tracks,))
    n_tracks = int(n_tracks)
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        par_t = _tables.on_device(particle, dev, torch.int64, 'particle')
        trk_t = _tables.on_device(track_of_particle, dev, torch.int32, 'track_of_particle')
        out = torch.empty((n_tracks, n_frames, cluster_size, ndim), dtype=torch.float64, device=dev)
        present = torch.empty((n_tracks, n_frames), dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        d = _abi.TrackPositions()
        d.ndim, d.cluster_size, d.n_frames, d.n_features = ndim, cluster_size, n_frames, n
        d.n_particles, d.n_tracks = n_particles, n_tracks
        d.frame_offset, d.particle = off_t.data_ptr(), par_t.data_ptr() or None
        d.track_of_particle, d.pos = trk_t.data_ptr() or None, pos_t.data_ptr() or None
        d.present, d.pos_out, d.status = present.data_ptr() or None, out.data_ptr() or None, status.data_ptr()
        eng.on_current_stream(eng.track_positions_device, d, dev=dev)
        return TrackPositions(*_tables.results(
            as_tensor, status, _abi.TRACKS_OK, "track_positions_arrays: frame_offset must rise within [0, N], particle "
            "must be below P and track_of_particle below n_tracks", out, present))


def _tracks_of_table(f, cluster_size, min_frames, pos_columns, t_column, device):
    cluster_size, min_frames = _check_sizes(cluster_size, min_frames)
    order, offset, first, ids, dense, _, pos, cluster = _tables.frame_sorted(f, pos_columns, t_column, extra=('cluster',))
    res = cluster_tracks_arrays(offset, dense, cluster, cluster_size, min_frames, device, n_particles=len(ids))
    if res.status != _abi.TRACKS_OK:
        raise _lib.EngineError("cluster_tracks: the components did not settle within the round bound (status %d)"
                               % res.status)
    block = track_positions_arrays(pos, offset, dense, res.track_of_particle, res.n_tracks, cluster_size, device)
    return order, dense, first, res, block


def cluster_tracks(f, cluster_size, min_frames=1, pos_columns=None, t_column='frame', device=0):
    """A copy of ``f`` with a ``cluster_track`` column (int64; -1 where the particle has no track).

    f: the DataFrame that ``find_clusters`` or ``refine_leastsq`` returns, with a ``particle`` column
    (ids of any integer type: they are mapped through their sorted unique values) and a ``cluster``
    column.  ``attrs`` of the result carries ``n_tracks``, ``n_conflict`` and ``n_incomplete``: the
    (track, frame) cells with more, and with fewer, than ``cluster_size`` member rows, frames counted
    from ``f[t_column].min()`` to its maximum."""
    order, dense, _, res, block = _tracks_of_table(f, cluster_size, min_frames, pos_columns, t_column, device)
    column = np.empty(len(f), dtype=np.int64)
    column[order] = res.track_of_particle[dense]
    out = f.copy()
    out['cluster_track'] = column
    out.attrs['n_tracks'] = res.n_tracks
    out.attrs['n_conflict'] = int((block.present > int(cluster_size)).sum())
    out.attrs['n_incomplete'] = int((block.present < int(cluster_size)).sum())
    return out


def track_positions(f, cluster_size, min_frames=1, pos_columns=None, t_column='frame', device=0):
    """``(pos [n_tracks, length, cluster_size, ndim], track_ids, first_frame)`` of the table's cluster
    tracks: the block that ``motion.orientation_arrays`` takes.  Frames are counted from
    ``first_frame = f[t_column].min()`` and missing frames are empty (NaN), as in ``orientation_df``;
    ``track_ids`` are the values of :func:`cluster_tracks`'s column, ``0 .. n_tracks - 1``."""
    _, _, first, res, block = _tracks_of_table(f, cluster_size, min_frames, pos_columns, t_column, device)
    return block.pos, np.arange(res.n_tracks, dtype=np.int64), first
