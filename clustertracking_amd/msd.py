"""Mean squared displacement of linked particles on the MI355X, of every particle and of the
ensemble, against lag time.  What a user of the reference computes with trackpy (``msd``, ``imsd``,
``emsd``) before trusting ``motion.diffusion_tensor``: it calibrates the monomer's D, it shows
whether ``subtract_drift`` worked (a residual drift ``v`` adds ``|v|**2 k**2`` at lag ``k``) and it
tells stuck particles from free ones before ``cluster_tracks``.

The rule is this project's dense restatement of trackpy's published ``msd`` / ``imsd`` / ``emsd``
with gaps (``include/ctrefine.h`` has it in full; ``tests/_msd.py`` restates it):

1. of several rows of one frame with the same id ``>= 0`` only the lowest row exists;
2. rows ``i`` (frame ``t``) and ``j`` (frame ``t + k``) with ``particle[i] == particle[j] == p >= 0``
   are a pair of ``(p, k)``; a missing frame in between makes no difference;
3. ``d = (pos[j] - pos[i]) * mpp`` per coordinate;
4. ``n[p, k]`` is the number of pairs;
5. ``mean_d[p, k, a]`` is the mean of ``d_a``;
6. ``mean_d2[p, k, a]`` is the mean of ``d_a**2``;
7. ``msd[p, k]`` is the sum of ``mean_d2[p, k, a]`` over the coordinates;
8. ``lagt[k] = k / fps`` for ``k = 1 .. max_lagtime``;
9. where ``n == 0`` the means and ``msd`` are NaN: ``k`` beyond the track's span, a particle with
   one row, an id without rows;
10. the ensemble: the same four quantities over the pairs of all particles pooled, i.e. the mean of
    the per-particle values weighted by ``n``; its ``n`` is int64.

Where this differs from trackpy: the result has a row for every lag up to ``max_lagtime``, NaN where
the track (or every track) is too short, where trackpy cuts the table at the longest lag present;
``n`` is the count of pairs, not trackpy's estimate ``N`` of independent measurements; the table
forms densify the frames as ``drift`` does.  Where a lag has a pair the values are trackpy's.
Parity with trackpy itself is not pinned by a test: it is not a dependency.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import collections
import math

import numpy as np

from . import _abi, _tables

MSD = collections.namedtuple('MSD', ['lagt', 'msd', 'mean_d', 'mean_d2', 'n', 'status'])
EMSD = collections.namedtuple('EMSD', ['lagt', 'msd', 'mean_d', 'mean_d2', 'n', 'status'])

_REFUSED = "frame_offset must rise within [0, N] and particle must be below n_particles"


def _scales(mpp, fps, ndim):
    """(mpp per axis, fps) as floats"""
    scale = np.asarray(mpp, dtype=np.float64)
    if scale.ndim == 0:
        scale = np.repeat(scale, ndim)
    if scale.shape != (ndim,) or not np.isfinite(scale).all():
        raise ValueError("mpp must be a finite number or one per axis (%d), not %r" % (ndim, mpp))
    if isinstance(fps, bool) or not isinstance(fps, (int, float, np.integer, np.floating)) \
            or not math.isfinite(fps) or fps <= 0:
        raise ValueError("fps must be a positive number, not %r" % (fps,))
    return [float(x) for x in scale], float(fps)


def _selection(particles, n_particles):
    """None, a tensor as it is, or an ascending int64 ndarray of ids within [0, P) (P where it is known)"""
    if particles is None or _tables.is_tensor(particles):
        if particles is not None and particles.dim() != 1:
            raise ValueError("particles must be one-dimensional, not %s" % (tuple(particles.shape),))
        return particles
    particles = np.asarray(particles)
    if particles.ndim != 1 or (particles.size and particles.dtype.kind not in 'iu'):
        raise ValueError("particles must be a one-dimensional list of integer ids")
    particles = np.ascontiguousarray(particles, dtype=np.int64)
    if particles.size and ((np.diff(particles) <= 0).any() or particles[0] < 0):
        raise ValueError("particles must be ascending ids >= 0")
    _below(particles, n_particles)
    return particles


def _below(particles, n_particles):
    if n_particles is not None and isinstance(particles, np.ndarray) and particles.size and particles[-1] >= n_particles:
        raise ValueError("particles must be ascending ids below n_particles = %d, not %d" % (n_particles, particles[-1]))


def _inputs(pos, frame_offset, particle, max_lagtime, mpp, fps, n_particles):
    max_lagtime = _tables.integer(max_lagtime, 1, 'max_lagtime')
    if max_lagtime > 2 ** 31 - 3:
        raise ValueError("max_lagtime must be an integer below 2^31 - 2")
    pos, n, ndim = _tables.positions(pos)
    scale, fps = _scales(mpp, fps, ndim)
    frame_offset, n_frames = _tables.offsets(frame_offset)
    particle, n_particles = _tables.particles(particle, n, n_particles)
    return pos, n, ndim, frame_offset, n_frames, particle, n_particles, max_lagtime, scale, fps


def _device_table(pos, frame_offset, particle, n, n_particles, dev):
    """the three tables on the device, the rows in a stable ascending sort by particle, and P"""
    import torch
    pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
    off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
    par_t = _tables.on_device(particle, dev, torch.int64, 'particle')
    if n_particles is None:
        n_particles = _tables.count_particles(par_t, n)
    # rows are in frame order: one stable sort by particle gives (particle, frame, row) order
    order = torch.sort(par_t, stable=True)[1] if n else par_t
    return pos_t, off_t, par_t, order, n_particles


def _lag_times(max_lagtime, fps, dev):
    """clause 8 on the device: k / fps as a division of two tensors (by a Python number torch multiplies
    with the reciprocal, which is not the rounded quotient)"""
    import torch
    return torch.arange(1, max_lagtime + 1, dtype=torch.float64, device=dev) / torch.full((), fps, dtype=torch.float64, device=dev)


def _fill(d, ndim, max_lagtime, n_frames, n, n_particles, scale, pos_t, off_t, par_t, order):
    d.ndim, d.max_lagtime, d.n_frames, d.n_features, d.n_particles = ndim, max_lagtime, n_frames, n, n_particles
    for a in range(ndim):
        d.mpp[a] = scale[a]
    d.pos, d.frame_offset = pos_t.data_ptr() or None, off_t.data_ptr()
    d.particle, d.order = par_t.data_ptr() or None, order.data_ptr() or None


def msd_arrays(pos, frame_offset, particle, max_lagtime=100, mpp=1., fps=1., particles=None, n_particles=None, device=0):
    """The mean squared displacement of every particle (``ctr_msd_device``; clauses 1 to 9 of the
    module's rule, trackpy's ``msd`` / ``imsd`` on arrays).

    pos float64 ``[N, ndim]``, ndim 2 or 3; frame_offset int64 ``[T + 1]``; particle int64 ``[N]``,
    dense ids ``0 .. P - 1``, negative = unlinked: what ``find_link_arrays``, ``link_arrays``,
    ``filter_stubs_arrays`` and ``subtract_drift_arrays`` produce, as ndarrays or as tensors on
    ``cuda:device``.  mpp: microns per pixel, a number or one per axis; fps: frames per second.
    particles: the ids to report, an ascending int64 list (``M`` rows; an id without rows is a row of
    NaN); the default is all ``P`` of them, ``P * max_lagtime * (12 + 16 * ndim)`` bytes of result --
    2.4 GB for the 540 730 particles of a 1250-frame video at 100 lags, so give the ids that
    ``filter_stubs_arrays`` keeps.  A tensor of ids is not checked on the host.  n_particles: P;
    default ``particle.max() + 1``, which for a tensor is one host read; with tensors and a given P
    there is no host copy and no synchronisation.

    Returns ``MSD(lagt float64 [L], msd [M, L], mean_d [M, L, ndim], mean_d2 [M, L, ndim], n int32
    [M, L], status)``: ndarrays and an int for ndarrays, tensors (status: int32 ``[1]``) for a tensor
    ``pos``.  A refused table (offsets not monotone within N, a particle >= P) raises ``ValueError``
    for ndarrays; for tensors status is ``_abi.MSD_BAD_TABLE``, the means NaN and n 0.  Unlike
    trackpy's ``imsd`` there is a row for every lag, NaN where the track is too short, and ``n``
    counts pairs.  The same bytes on every call."""
    pos, n, ndim, frame_offset, n_frames, particle, n_particles, max_lagtime, scale, fps = _inputs(
        pos, frame_offset, particle, max_lagtime, mpp, fps, n_particles)
    as_tensor = _tables.is_tensor(pos)
    particles = _selection(particles, n_particles)
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t, off_t, par_t, order, n_particles = _device_table(pos, frame_offset, particle, n, n_particles, dev)
        _below(particles, n_particles)
        select = None if particles is None else _tables.on_device(particles, dev, torch.int64, 'particles')
        m = n_particles if select is None else int(select.shape[0])
        msd = torch.empty((m, max_lagtime), dtype=torch.float64, device=dev)
        mean_d = torch.empty((m, max_lagtime, ndim), dtype=torch.float64, device=dev)
        mean_d2 = torch.empty((m, max_lagtime, ndim), dtype=torch.float64, device=dev)
        count = torch.empty((m, max_lagtime), dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lagt = _lag_times(max_lagtime, fps, dev)
        d = _abi.Msd()
        _fill(d, ndim, max_lagtime, n_frames, n, n_particles, scale, pos_t, off_t, par_t, order)
        d.n_select = m
        d.select = None if select is None else (select.data_ptr() or None)
        d.msd, d.mean_d, d.mean_d2 = msd.data_ptr() or None, mean_d.data_ptr() or None, mean_d2.data_ptr() or None
        d.n, d.status = count.data_ptr() or None, status.data_ptr()
        eng.on_current_stream(eng.msd_device, d, dev=dev)
        out = _tables.results(as_tensor, status, _abi.MSD_OK, "msd_arrays: " + _REFUSED, lagt, msd, mean_d, mean_d2, count)
        return MSD(*out, status if as_tensor else _abi.MSD_OK)


def emsd_arrays(pos, frame_offset, particle, max_lagtime=100, mpp=1., fps=1., n_particles=None, device=0):
    """The mean squared displacement of the ensemble (``ctr_emsd_device``; clause 10 of the module's
    rule, trackpy's ``emsd`` on arrays): every pair of every particle pooled.

    Arguments as for :func:`msd_arrays`.  Returns ``EMSD(lagt [L], msd [L], mean_d [L, ndim], mean_d2
    [L, ndim], n int64 [L], status)``, ndarrays or tensors as there; a refused table raises
    ``ValueError`` for ndarrays and gives NaN and 0 for tensors.  Nothing proportional to ``P * L`` is
    allocated: a workgroup takes ``_abi.MSD_CHUNK`` consecutive ids, a second kernel adds the chunks'
    sums in chunk order, the same bytes on every call.  Unlike trackpy's ``emsd`` there is a row for
    every lag and ``n`` counts pairs."""
    pos, n, ndim, frame_offset, n_frames, particle, n_particles, max_lagtime, scale, fps = _inputs(
        pos, frame_offset, particle, max_lagtime, mpp, fps, n_particles)
    as_tensor = _tables.is_tensor(pos)
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t, off_t, par_t, order, n_particles = _device_table(pos, frame_offset, particle, n, n_particles, dev)
        msd = torch.empty(max_lagtime, dtype=torch.float64, device=dev)
        mean_d = torch.empty((max_lagtime, ndim), dtype=torch.float64, device=dev)
        mean_d2 = torch.empty((max_lagtime, ndim), dtype=torch.float64, device=dev)
        count = torch.empty(max_lagtime, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lagt = _lag_times(max_lagtime, fps, dev)
        d = _abi.Emsd()
        _fill(d, ndim, max_lagtime, n_frames, n, n_particles, scale, pos_t, off_t, par_t, order)
        d.msd, d.mean_d, d.mean_d2 = msd.data_ptr(), mean_d.data_ptr(), mean_d2.data_ptr()
        d.n, d.status = count.data_ptr(), status.data_ptr()
        eng.on_current_stream(eng.emsd_device, d, dev=dev)
        out = _tables.results(as_tensor, status, _abi.MSD_OK, "emsd_arrays: " + _REFUSED, lagt, msd, mean_d, mean_d2, count)
        return EMSD(*out, status if as_tensor else _abi.MSD_OK)


def _checked(mpp, fps, max_lagtime, f, pos_columns):
    """argument errors of the table forms that do not need the table sorted"""
    _tables.integer(max_lagtime, 1, 'max_lagtime')
    ndim = len(pos_columns) if pos_columns is not None else (3 if 'z' in f else 2)
    if ndim in (2, 3):
        _scales(mpp, fps, ndim)


def imsd(f, mpp, fps, max_lagtime=100, pos_columns=None, t_column='frame', device=0):
    """The mean squared displacement of every particle of a linked table, as trackpy's ``imsd``: a
    DataFrame indexed by the lag time in seconds (``lagt``) with one column per particle.

    f: a DataFrame with a ``particle`` column; the ids are used as they are (mapped through their
    sorted unique values, so every id is a particle and a column), the frames from ``f[t_column]``'s
    minimum to its maximum as ``drift`` densifies them.  Unlike trackpy's ``imsd`` the table has a row
    for every lag up to ``max_lagtime``, NaN where a track is too short."""
    import pandas as pd
    _checked(mpp, fps, max_lagtime, f, pos_columns)
    _, offset, _, ids, dense, pos_columns, pos = _tables.frame_sorted(f, pos_columns, t_column)
    res = msd_arrays(pos, offset, dense, max_lagtime, mpp, fps, n_particles=len(ids), device=device)
    return pd.DataFrame(res.msd.T, index=pd.Index(res.lagt, name='lagt'), columns=pd.Index(ids, name='particle'))


def emsd(f, mpp, fps, max_lagtime=100, detail=False, pos_columns=None, t_column='frame', device=0):
    """The mean squared displacement of the ensemble of a linked table, as trackpy's ``emsd``: a Series
    ``msd`` indexed by ``lagt``, or with ``detail=True`` a DataFrame indexed by the lag in frames with
    ``<x>``, ``<x^2>`` for every position column, ``msd``, ``N`` (the count of pairs, where trackpy
    gives an estimate of the independent measurements) and ``lagt``.  Unlike trackpy's ``emsd`` there
    is a row for every lag up to ``max_lagtime``, NaN where no track is long enough."""
    import pandas as pd
    _checked(mpp, fps, max_lagtime, f, pos_columns)
    _, offset, _, ids, dense, pos_columns, pos = _tables.frame_sorted(f, pos_columns, t_column)
    res = emsd_arrays(pos, offset, dense, max_lagtime, mpp, fps, n_particles=len(ids), device=device)
    if not detail:
        return pd.Series(res.msd, index=pd.Index(res.lagt, name='lagt'), name='msd')
    out = pd.DataFrame(index=pd.RangeIndex(1, len(res.lagt) + 1, name='lag'))
    for a, col in enumerate(pos_columns):
        out['<%s>' % col] = res.mean_d[:, a]
    for a, col in enumerate(pos_columns):
        out['<%s^2>' % col] = res.mean_d2[:, a]
    out['msd'], out['N'], out['lagt'] = res.msd, res.n, res.lagt
    return out
