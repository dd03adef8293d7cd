"""Bootstrap confidence interval of the diffusion tensor on the MI355X: the reference's
``motion.diffusion_tensor_ci`` (reference ``clustertracking/motion.py:201-216``), which hands the
pooled displacement rows of :func:`clustertracking_amd.motion.diffusion_tensor` to
``scikits.bootstrap.ci``.

That package is not a dependency; its ``ci`` (methods ``'bca'`` and ``'pi'``) is restated from its
published source (``include/ctrefine.h`` has the rule in full), with a counter-based
index generator in place of ``np.random`` (:func:`bootstrap_indices` gives the same indices on the
host).  Resampling, sorting, bias correction, acceleration and ranks run on the device, for every
track and lag of a call; parity with the package itself is not pinned.

The functions live here and not in :mod:`clustertracking_amd.motion` because that module's
interface is pinned without them (``tests/test_motion_rule.py``).  There is no CPU fallback: without
the library or a GPU :func:`diffusion_tensor_ci` raises ``EngineError``; argument errors are raised
before that.
"""
import statistics

import numpy as np

from . import _abi, _tables
from .motion import diffusion_inputs

_MASK64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _mix64(z):
    """the finaliser of splitmix64, in Python integers"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def _check_seed(seed):
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) <= _MASK64:
        raise ValueError("seed must be an integer in [0, 2**64)")
    return int(seed)


def bootstrap_indices(n_samples, n, seed=0):
    """The resampling indices of :func:`diffusion_tensor_ci` on the host: int64 ``[n_samples, n]``,
    ``idx[b, k] = floor(r n / 2**64)`` with ``r = mix64(mix64(seed) + ((b << 32) + k + 1) *
    0x9E3779B97F4A7C15 mod 2**64)`` -- a function of ``(seed, b, k, n)`` alone, in exact integers
    (uint64 arithmetic that wraps, the 128-bit product in 32-bit halves)."""
    n_samples, n, seed = int(n_samples), int(n), _check_seed(seed)
    if n_samples < 0 or not 0 <= n < 2 ** 31:
        raise ValueError("n_samples must be >= 0 and n in [0, 2**31)")
    u = np.uint64
    b = np.arange(n_samples, dtype=np.uint64)[:, None]
    k = np.arange(n, dtype=np.uint64)[None, :]
    z = u(_mix64(seed)) + ((b << u(32)) + k + u(1)) * u(_GOLDEN)
    z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
    r = z ^ (z >> u(31))
    hi, lo = r >> u(32), r & u(0xFFFFFFFF)
    return ((hi * u(n) + ((lo * u(n)) >> u(32))) >> u(32)).astype(np.int64)


_CI_METHODS = {'bca': _abi.CI_BCA, 'pi': _abi.CI_PI}


def _ci_alphas(alpha):
    """scikits.bootstrap: a scalar alpha gives [alpha / 2, 1 - alpha / 2], a sequence is taken as it is"""
    if np.ndim(alpha) == 0:
        a = float(alpha)
        if not 0. < a < 1.:
            raise ValueError("alpha must lie inside (0, 1), not %r" % (alpha,))
        return [a / 2., 1. - a / 2.]
    alphas = [float(a) for a in np.asarray(alpha, dtype=np.float64).reshape(-1)]
    if not 1 <= len(alphas) <= _abi.DIFFUSION_CI_MAX_ALPHA:
        raise ValueError("alpha must hold 1 to %d probabilities, not %d" % (_abi.DIFFUSION_CI_MAX_ALPHA, len(alphas)))
    if not all(0. < a < 1. for a in alphas):
        raise ValueError("every alpha must lie inside (0, 1)")
    return alphas


def diffusion_tensor_ci(positions, orientations, lagtime=1, fps=1., ndim=3, alpha=0.05, n_samples=10000,
                        method='bca', seed=0, pool_tracks=False, return_details=False, device=0, **unsupported):
    """Bootstrap confidence interval of the diffusion tensor (``ctr_diffusion_ci_device``): the
    reference's ``diffusion_tensor_ci``, for every track and every lag of a sweep in one call.

    positions, orientations, lagtime, fps, ndim and pool_tracks as for :func:`clustertracking_amd.motion.diffusion_tensor`
    (``pool_tracks`` resamples the concatenated rows of all tracks).  alpha: a scalar gives the
    percentiles ``[alpha / 2, 1 - alpha / 2]``, a sequence of up to 8 probabilities is taken as it
    is.  n_samples resamples (at most 16384) drawn by the counter-based generator of
    :func:`bootstrap_indices` from ``seed``; method ``'bca'`` (bias-corrected and accelerated) or
    ``'pi'`` (percentile), as ``scikits.bootstrap.ci`` defines them.
    Returns ``interval [T][, n_lags], K, D, D`` (K = 2 for a scalar alpha: low, high -- with the
    reference's argument shapes the reference's ``(2, D, D)``); no rows give NaN.
    ``return_details``: also a dict of ``tensor`` (the statistic of the rows themselves), ``counts``
    (rows), ``z0`` (bias correction), ``a`` (acceleration) and ``ranks`` (int64, the positions of the
    interval among the sorted resamples; 0 or ``n_samples - 1`` means the interval ran into the end).
    ndarrays in give ndarrays, tensors on ``cuda:device`` give tensors on the current stream (no host
    copy, no synchronisation)."""
    for name in unsupported:
        if name in ('multi', 'output', 'epsilon', 'statfunction', 'statfunc', 'statistic'):
            raise NotImplementedError("diffusion_tensor_ci: %r of scikits.bootstrap.ci is not implemented" % name)
        raise TypeError("diffusion_tensor_ci() got an unexpected keyword argument %r" % name)
    if method == 'abc':
        raise NotImplementedError("method 'abc' of scikits.bootstrap.ci is not implemented")
    if method not in _CI_METHODS:
        raise ValueError("method must be 'bca' or 'pi', not %r" % (method,))
    alphas = _ci_alphas(alpha)
    if isinstance(n_samples, bool) or int(n_samples) != n_samples or n_samples < 1:
        raise ValueError("n_samples must be an integer >= 1")
    if n_samples > _abi.DIFFUSION_CI_MAX_SAMPLES:
        raise ValueError("n_samples must be at most %d" % _abi.DIFFUSION_CI_MAX_SAMPLES)
    seed = _check_seed(seed)
    positions, orientations, as_tensor, scalar_lag, lags, tracked, n_tracks, n_frames, n_perm = diffusion_inputs(
        positions, orientations, lagtime, fps, ndim)
    pooled = bool(tracked and pool_tracks)
    D, K = 3 if ndim == 2 else 6, len(alphas)
    lead = (len(lags),) if pooled else (n_tracks, len(lags))
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(positions, dev, torch.float64, 'positions')
        ori_t = _tables.on_device(orientations, dev, torch.float64, 'orientations')
        lag_t = torch.from_numpy(lags).to(dev)
        interval = torch.empty(lead + (K, D, D), dtype=torch.float64, device=dev)
        ranks = torch.empty(lead + (K, D, D), dtype=torch.int64, device=dev)
        tensor = torch.empty(lead + (D, D), dtype=torch.float64, device=dev)
        z0, accel = torch.empty_like(tensor), torch.empty_like(tensor)
        counts = torch.empty(lead, dtype=torch.int64, device=dev)
        if counts.numel():
            d = _abi.DiffusionCI()
            d.ndim, d.n_perm, d.n_tracks, d.n_frames, d.n_lags, d.fps = ndim, n_perm, n_tracks, n_frames, len(lags), float(fps)
            d.lags, d.positions, d.bases = lag_t.data_ptr(), pos_t.data_ptr() or None, ori_t.data_ptr() or None
            d.n_samples, d.seed, d.method, d.n_alpha, d.pool_tracks = int(n_samples), seed, _CI_METHODS[method], K, int(pooled)
            normal = statistics.NormalDist()
            for q, a in enumerate(alphas):
                d.alphas[q], d.z_alpha[q] = a, normal.inv_cdf(a)
            d.interval, d.tensor, d.n_rows = interval.data_ptr(), tensor.data_ptr(), counts.data_ptr()
            d.z0, d.accel, d.ranks = z0.data_ptr(), accel.data_ptr(), ranks.data_ptr()
            eng.on_current_stream(eng.diffusion_ci_device, d, dev=dev)
        out = [interval, ranks, tensor, z0, accel, counts]
        if not tracked:
            out = [x.reshape(x.shape[1:]) for x in out]
        if scalar_lag:
            lag_axis = 1 if tracked and not pooled else 0
            out = [x.select(lag_axis, 0) for x in out]
        if not as_tensor:
            out = [x.cpu().numpy() for x in out]
            if out[5].ndim == 0:
                out[5] = int(out[5])
    interval, ranks, tensor, z0, accel, counts = out
    if return_details:
        return interval, dict(tensor=tensor, counts=counts, z0=z0, a=accel, ranks=ranks)
    return interval
