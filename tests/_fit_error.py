"""The rule of ``ct.fit_error`` (clustertracking_amd/fit_error.py, include/ctrefine.h) restated in NumPy:
plain loops over the rows and the parameters, float64, no oracle and no reference.  A helper module
like _residual.py, whose covering, box and model helpers it uses; the CPU and GPU tests of the stage
compare against it.

A :class:`Cluster` is one cluster with its masks fixed: ``objective(v)`` is F, ``gradient(v)`` its
analytic gradient and ``hessian(v)`` its analytic Hessian 2 (J^T J + Q) / (P norm) in the variables
of ``vect_from_params``.  :func:`fit_error_np` is the whole stage on ndarrays.
"""
import collections
import time

import numpy as np

import _residual
from clustertracking_amd.fitfunc import FitFunctions

OK, NOT_POSITIVE_DEFINITE, NONFINITE, EMPTY, TOO_LARGE = range(5)
MAX_ROWS, MAX_VARS = 64, 127
CONST, VAR, CLUSTER = 0, 1, 3

FitError = collections.namedtuple('FitError', [
    'params_std', 'status', 'n_vars', 'n_pix', 'cov', 'cov_offset', 'var_row', 'var_col'])


def derivatives(kind, ndim, r2, q, e):
    """g and its derivatives on arrays of r2 and q: (g, g', g'', [g_e], [g'_e], [[g_ee']]) with ' the
    derivative in r2 and e over the profile parameters"""
    k = 0.5 * ndim
    nx = len(e)
    zero = np.zeros_like(r2)
    ge, g1e = [zero.copy() for _ in range(nx)], [zero.copy() for _ in range(nx)]
    gee = [[zero.copy() for _ in range(nx)] for _ in range(nx)]
    if kind == 'gauss' or (kind == 'disc' and not e[0] > 0.):
        g = np.exp(-0.5 * ndim * r2)
        if kind == 'disc':
            g = np.where(q < 1., np.nan, g)
        return g, -k * g, k * k * g, ge, g1e, gee
    if kind == 'inv_series':
        big = nx - 1
        y, dy, ddy = np.ones_like(r2), zero.copy(), zero.copy()
        for t in range(1, nx):
            ddy = ddy * r2 + 2. * dy
            dy = dy * r2 + y
            y = y * r2 + e[t]
        g = e[0] / y
        g1 = -e[0] * dy / y ** 2
        g2 = e[0] * (2. * dy * dy / y ** 3 - ddy / y ** 2)
        pw = [None] + [r2 ** (big - t) for t in range(1, nx)]
        dpw = [None] + [(big - t) * r2 ** (big - t - 1) if big - t > 0 else zero.copy() for t in range(1, nx)]
        ge[0] = 1. / y
        g1e[0] = -dy / y ** 2
        for t in range(1, nx):
            ge[t] = -e[0] * pw[t] / y ** 2
            g1e[t] = -e[0] * (dpw[t] / y ** 2 - 2. * dy * pw[t] / y ** 3)
            gee[t][0] = gee[0][t] = -pw[t] / y ** 2
            for u in range(1, nx):
                gee[t][u] = 2. * e[0] * pw[t] * pw[u] / y ** 3
        return g, g1, g2, ge, g1e, gee
    r = np.sqrt(r2)
    clamped = False
    if kind == 'ring':
        t = e[0]
        w = (r - 1. + t) / t
        w_e, w_ee = (1. - r) / t ** 2, -2. * (1. - r) / t ** 3
        phi = -k * w * w
        p_r, p_rr = -2. * k * w / t, -2. * k / t ** 2
        p_e, p_ee = -2. * k * w * w_e, -2. * k * (w_e * w_e + w * w_ee)
        p_re = -2. * k * (w_e * t - w) / t ** 2
        flat = np.zeros(r2.shape, dtype=bool)
    else:
        assert kind == 'disc'
        clamped = e[0] >= 1.
        ds = 0.999 if clamped else e[0]
        big = 1. - ds
        u = (r - ds) / big
        u_d, u_dd = (r - 1.) / big ** 2, 2. * (r - 1.) / big ** 3
        phi = -k * u * u
        p_r, p_rr = -2. * k * u / big, -2. * k / big ** 2
        p_e, p_ee = -2. * k * u * u_d, -2. * k * (u_d * u_d + u * u_dd)
        p_re = -2. * k * (u_d / big + u / big ** 2)
        flat = ~(r2 > ds * ds) | (q < 1.)
    g = np.exp(phi)
    g_r, g_rr = g * p_r, g * (p_r * p_r + p_rr)
    g1 = g_r / (2. * r)
    g2 = g_rr / (4. * r2) - g_r / (4. * r2 * r)
    if not clamped:
        ge[0] = g * p_e
        gee[0][0] = g * (p_e * p_e + p_ee)
        g1e[0] = g * (p_r * p_e + p_re) / (2. * r)
    if kind == 'ring':
        g = np.where(q < 1., np.nan, g)
    else:
        g = np.where(flat, 1., g)
        g1, g2 = np.where(flat, 0., g1), np.where(flat, 0., g2)
        ge[0], g1e[0], gee[0][0] = np.where(flat, 0., ge[0]), np.where(flat, 0., g1e[0]), np.where(flat, 0., gee[0][0])
    return g, g1, g2, ge, g1e, gee


def modes_of(fit_function, ndim, isotropic, param_mode):
    return list(FitFunctions(fit_function, ndim, isotropic, param_mode).modes)


class Cluster(object):
    """One cluster: ``image`` float64 (z,) y, x; ``params`` [n, n_params], the rows in ascending row
    order; ``centres`` [n, ndim] of the masks; ``modes`` per column (CONST, VAR, CLUSTER)."""

    def __init__(self, image, params, centres, diameter, fit_function, modes, residual_factor=100000., fmax=None):
        self.image = np.asarray(image, dtype=np.float64)
        self.params = np.array(params, dtype=np.float64)
        self.ndim = self.image.ndim
        self.kind, self.nx, self.radius, self.isotropic, n_params = _residual.model_of(fit_function, self.ndim, diameter)
        assert self.params.shape[1] == n_params == len(modes)
        self.modes = [int(m) for m in modes]
        self.n = len(self.params)
        self.norm = (np.float64(self.image.max()) if fmax is None else np.float64(fmax)) ** 2 / residual_factor
        # the layout of vect_from_params: column by column
        self.base, at = [], 0
        for mode in self.modes:
            self.base.append(at if mode != CONST else -1)
            at += self.n if mode == VAR else 1 if mode == CLUSTER else 0
        self.nv = at
        # the covered pixels: the union of the masks, each row's mask as a selection of them
        union = np.zeros(self.image.shape, dtype=bool)
        masks = []
        for i in range(self.n):
            m = np.zeros(self.image.shape, dtype=bool)
            box = _residual.box_of(centres[i], self.radius, self.image.shape)
            if box is not None:
                grid = np.meshgrid(*[np.arange(b.start, b.stop, dtype=np.float64) for b in box], indexing='ij', sparse=True)
                m[box] = _residual.covering(grid, centres[i], self.radius)
            masks.append(m)
            union |= m
        self.n_pix = int(union.sum())
        self.coords = [c.astype(np.float64) for c in np.nonzero(union)]
        self.values = self.image[union]
        self.masks = [m[union] for m in masks]

    def variable(self, i, col):
        return -1 if self.base[col] < 0 else self.base[col] + (i if self.modes[col] == VAR else 0)

    def vect(self):
        v = np.zeros(self.nv)
        for col, mode in enumerate(self.modes):
            if mode == VAR:
                v[self.base[col]:self.base[col] + self.n] = self.params[:, col]
            elif mode == CLUSTER:
                column = self.params[:, col]
                if np.all(column == column[0]):
                    v[self.base[col]] = column[0]
                else:
                    s = 0.
                    for x in column:
                        s = s + x
                    v[self.base[col]] = s / self.n
        return v

    def table(self, v):
        """vect_to_params"""
        p = self.params.copy()
        for col, mode in enumerate(self.modes):
            if mode == VAR:
                p[:, col] = v[self.base[col]:self.base[col] + self.n]
            elif mode == CLUSTER:
                p[:, col] = v[self.base[col]]
        return p

    def finite(self):
        p = self.table(self.vect())
        return bool(np.all(np.isfinite(p[:, 1:])) and np.isfinite(p[0, 0]))

    def evaluate(self, v, second=True):
        """(F, gradient of F, A = J^T J + Q, res, J) at v; A is None without ``second``"""
        p = self.table(v)
        ndim, nd, pw = self.ndim, self.ndim, len(self.modes) - 1
        nsz = 1 if self.isotropic else ndim
        ng = ndim + nsz
        n_points = len(self.values)
        res = self.values - p[0, 0]
        first, blocks = [], []
        with np.errstate(all='ignore'):
            for i in range(self.n):
                m = self.masks[i]
                sig, e = p[i, 1], p[i, 2 + ng:]
                d, i2, size = [], [], []
                r2 = np.zeros(int(m.sum()))
                for a in range(ndim):
                    sz = p[i, 2 + ndim + (0 if self.isotropic else a)]
                    size.append(sz)
                    i2.append(1. / (sz * sz))
                    d.append(self.coords[a][m] - p[i, 2 + a])
                    r2 = r2 + (d[a] * d[a]) * i2[a]
                q = np.zeros_like(r2)
                for a in range(ndim - 1, -1, -1):
                    q = q + d[a] * d[a]
                g, g1, g2, ge, g1e, gee = derivatives(self.kind, nd, r2, q, e)
                res[m] = res[m] - sig * g
                # r2 in the geometric parameters: centres, then sizes
                r2p = [-2. * d[a] * i2[a] for a in range(ndim)]
                r2pq = [[np.zeros_like(r2) for _ in range(ng)] for _ in range(ng)]
                for a in range(ndim):
                    r2pq[a][a] = 2. * i2[a] + np.zeros_like(r2)
                if self.isotropic:
                    r2p.append(-2. * r2 / size[0])
                    for a in range(ndim):
                        r2pq[a][ndim] = r2pq[ndim][a] = 4. * d[a] * i2[a] / size[0]
                    r2pq[ndim][ndim] = 6. * r2 * i2[0]
                else:
                    for a in range(ndim):
                        r2p.append(-2. * d[a] * d[a] * i2[a] / size[a])
                        r2pq[a][ndim + a] = r2pq[ndim + a][a] = 4. * d[a] * i2[a] / size[a]
                        r2pq[ndim + a][ndim + a] = 6. * d[a] * d[a] * i2[a] * i2[a]
                dm = [g] + [sig * g1 * r2p[t] for t in range(ng)] + [sig * ge[k] for k in range(self.nx)]
                first.append(dm)
                if second:
                    h = [[None] * pw for _ in range(pw)]
                    h[0][0] = np.zeros_like(r2)
                    for t in range(ng):
                        h[0][1 + t] = h[1 + t][0] = g1 * r2p[t]
                        for u in range(ng):
                            h[1 + t][1 + u] = sig * (g2 * r2p[t] * r2p[u] + g1 * r2pq[t][u])
                    for k in range(self.nx):
                        h[0][1 + ng + k] = h[1 + ng + k][0] = ge[k]
                        for t in range(ng):
                            h[1 + t][1 + ng + k] = h[1 + ng + k][1 + t] = sig * g1e[k] * r2p[t]
                        for l in range(self.nx):
                            h[1 + ng + k][1 + ng + l] = sig * gee[k][l]
                    blocks.append(h)
            ok = ~np.isnan(res)
            jac = np.zeros((n_points, self.nv))
            if self.base[0] >= 0:
                jac[:, self.base[0]] = -1.
            for i in range(self.n):
                m = self.masks[i]
                for t in range(pw):
                    var = self.variable(i, 1 + t)
                    if var >= 0:
                        jac[m, var] = jac[m, var] - first[i][t]
            jac, r = jac[ok], res[ok]
            scale = self.n_pix * self.norm
            value = np.sum(r * r) / scale
            grad = 2. * (jac.T @ r) / scale
            mat = None
            if second:
                mat = jac.T @ jac
                for i in range(self.n):
                    keep = ok[self.masks[i]]
                    ri = res[self.masks[i]][keep]
                    for t in range(pw):
                        vt = self.variable(i, 1 + t)
                        if vt < 0:
                            continue
                        for u in range(pw):
                            vu = self.variable(i, 1 + u)
                            if vu >= 0:
                                mat[vt, vu] -= np.sum(ri * blocks[i][t][u][keep])      # d2res = -d2m
        return value, grad, mat, res, jac

    def objective(self, v):
        return self.evaluate(v, second=False)[0]

    def gradient(self, v):
        return self.evaluate(v, second=False)[1]

    def hessian(self, v):
        return 2. * self.evaluate(v)[2] / (self.n_pix * self.norm)


def cholesky(mat):
    """the lower factor by plain loops, or None where a pivot is not a positive finite number"""
    n = len(mat)
    low = np.array(mat, dtype=np.float64)
    for j in range(n):
        d = low[j, j]
        if not (d > 0. and np.isfinite(d)):
            return None
        low[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            low[i, j] = low[i, j] / low[j, j]
        for i in range(j + 1, n):
            for k in range(j + 1, i + 1):
                low[i, k] = low[i, k] - low[i, j] * low[k, j]
    return np.tril(low)


def inverse_from_factor(low):
    """(L L^T)^-1: the inverse of the factor by substitution, then its product with its transpose"""
    n = len(low)
    x = np.zeros((n, n))
    for j in range(n):
        x[j, j] = 1. / low[j, j]
        for i in range(j + 1, n):
            s = 0.
            for k in range(j, i):
                s = s + low[i, k] * x[k, j]
            x[i, j] = -s / low[i, i]
    return x.T @ x


def cluster_result(c):
    """(status, std [nv], cov [nv, nv]) of a :class:`Cluster`"""
    nan = np.full(c.nv, np.nan), np.full((c.nv, c.nv), np.nan)
    if not c.finite():
        return (NONFINITE,) + nan
    if c.n_pix == 0:
        return (EMPTY,) + nan
    mat = c.evaluate(c.vect())[2]
    low = cholesky(mat)
    if low is None:
        return (NOT_POSITIVE_DEFINITE,) + nan
    with np.errstate(all='ignore'):
        cov = c.n_pix * c.norm * inverse_from_factor(low)
        return OK, np.sqrt(np.diag(cov)), cov


def groups_of(frame_offset, cluster):
    """the clusters in the order of (frame, label): lists of rows in ascending order"""
    out = []
    for t in range(len(frame_offset) - 1):
        rows = np.arange(int(frame_offset[t]), int(frame_offset[t + 1]))
        for label in np.unique(np.asarray(cluster)[rows]):
            out.append((t, [int(r) for r in rows if cluster[r] == label]))
    return out


def fit_error_np(frames, params, frame_offset, cluster, diameter, fit_function='gauss', param_mode=None, mask_pos=None,
                 residual_factor=100000.):
    """The stage on ndarrays: ``FitError`` with the covariance, as ``ct.fit_error_arrays(want_cov=True)``."""
    frames = np.asarray(frames)
    params = np.asarray(params, dtype=np.float64)
    ndim = frames.ndim - 1
    kind, nx, radius, isotropic, n_params = _residual.model_of(fit_function, ndim, diameter)
    modes = modes_of(fit_function, ndim, isotropic, param_mode)
    n = len(params)
    centres = params[:, 2:2 + ndim] if mask_pos is None else np.asarray(mask_pos, dtype=np.float64)
    std = np.full((n, n_params), np.nan)
    status, n_vars, n_pix = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    cov, cov_offset, var_row, var_col = [], [0], [], []
    for t, rows in groups_of(frame_offset, cluster):
        nv = modes.count(VAR) * len(rows) + modes.count(CLUSTER)
        n_vars[rows] = nv
        if len(rows) > MAX_ROWS or nv > MAX_VARS:
            status[rows] = TOO_LARGE
            cov_offset.append(cov_offset[-1])
            continue
        c = Cluster(frames[t], params[rows], centres[rows], diameter, fit_function, modes, residual_factor,
                    fmax=frames[t].max())
        if not np.all(np.isfinite(centres[rows])):
            code, s, block = NONFINITE, np.full(nv, np.nan), np.full((nv, nv), np.nan)
        else:
            code, s, block = cluster_result(c)
        status[rows] = code
        n_pix[rows] = c.n_pix if code not in (NONFINITE,) else 0
        for col, mode in enumerate(modes):
            if mode == CONST:
                continue
            for k, row in enumerate(rows):
                std[row, col] = s[c.variable(k, col)]
            var_col += [col] * (len(rows) if mode == VAR else 1)
            var_row += rows if mode == VAR else [-1]
        cov.append(block.reshape(-1))
        cov_offset.append(cov_offset[-1] + nv * nv)
    return FitError(std, status, n_vars, n_pix, np.concatenate(cov) if cov else np.zeros(0),
                    np.array(cov_offset, dtype=np.int64), np.array(var_row, dtype=np.int64), np.array(var_col, dtype=np.int32))


def distance_std_np(cov, delta):
    """the delta method for |delta| between two points with the covariance ``cov`` of (a, b) stacked"""
    delta = np.asarray(delta, dtype=np.float64)
    g = np.concatenate([delta, -delta]) / np.sqrt(np.sum(delta * delta))
    return float(np.sqrt(g @ cov @ g))


# ---- inputs the CPU and GPU tests share -------------------------------------------------------------
def draw(rng, shape, fit_function, params, noise=2., dtype=np.uint8):
    """a frame with the model of ``params`` [n, n_params] (isotropic or not by its width) on a noisy background"""
    ndim = len(shape)
    n_geo = params.shape[1] - 2 - ndim
    kind = 'inv_series' if fit_function.startswith('inv_series') else fit_function
    nx = {'gauss': 0, 'ring': 1, 'disc': 1}.get(kind, int(fit_function.rsplit('_', 1)[1]) + 1 if kind == 'inv_series' else 0)
    isotropic = n_geo - nx == 1
    grid = np.indices(shape, dtype=np.float64)
    frame = np.full(shape, params[0, 0]) + rng.normal(0., noise, shape)
    with np.errstate(all='ignore'):
        for p in params:
            r2 = sum(((grid[a] - p[2 + a]) / p[2 + ndim + (0 if isotropic else a)]) ** 2 for a in range(ndim))
            q = sum((grid[a] - p[2 + a]) ** 2 for a in range(ndim))
            g = derivatives(kind, ndim, r2, np.where(q < 1., 1., q), p[len(p) - nx:])[0]
            frame += p[1] * np.nan_to_num(g, nan=1.)
    if np.dtype(dtype).kind in 'iu':
        info = np.iinfo(dtype)
        return np.clip(np.round(frame), info.min, info.max).astype(dtype)
    return frame.astype(dtype)


def timed(fn, *args, **kwargs):
    t0 = time.perf_counter()
    out = fn(*args, **kwargs)
    return out, time.perf_counter() - t0


PROFILES = [('gauss', []), ('ring', [0.45]), ('disc', [0.5]), ('inv_series_2', [1.25, 0.75, 1.5])]
# the mode mixes of the tests, by profile: the default, sizes per row, one size per cluster, one signal per
# cluster, everything but the signal constant; and the profile's own parameters per row and per cluster
MODE_MIXES = [None, dict(size='var'), dict(size='cluster'), dict(signal='cluster'),
              dict(pos='const', background='const')]
PROFILE_MIXES = {'gauss': [], 'ring': [dict(thickness='var'), dict(thickness='cluster')],
                 'disc': [dict(disc_size='var'), dict(disc_size='cluster', size='cluster')],
                 'inv_series_2': [dict(param_a='var', param_b='cluster'), dict(signal_mult='cluster', signal='const')]}


def truth(rng, fit, extra, shape, diameter, n, spread=1.1, signal=(90., 160.), background=12.):
    """params [n, n_params] of n features in a row along the last axis, their masks overlapping"""
    ndim = len(shape)
    kind, nx, radius, isotropic, n_params = _residual.model_of(fit, ndim, diameter)
    base = np.array([s / 2. for s in shape]) + rng.uniform(-0.5, 0.5, ndim)
    step = np.zeros(ndim)
    step[-1] = radius[-1] * spread
    pos = np.array([base + (k - (n - 1) / 2.) * step + rng.uniform(-0.3, 0.3, ndim) for k in range(n)])
    wide = 0.75 if kind in ('ring', 'disc') else 0.4
    sizes = rng.uniform(0.9, 1.1, (n, 1 if isotropic else ndim)) * wide * np.array(radius[:1] if isotropic else radius)
    params = np.concatenate([np.full((n, 1), background), rng.uniform(signal[0], signal[1], (n, 1)), pos, sizes,
                             np.tile(np.array(extra, dtype=np.float64), (n, 1)).reshape(n, len(extra))], axis=1)
    assert params.shape[1] == n_params
    return params


def fitted(rng, params, ndim, jitter=0.03):
    """the table a fit would return: the truth a little off in signal, position and size"""
    out = params.copy()
    out[:, 1] *= 1. + rng.uniform(-0.01, 0.01, len(out))
    out[:, 2:2 + ndim] += rng.uniform(-jitter, jitter, (len(out), ndim))
    return out


def table(rng, fit, extra, ndim, isotropic, pixel=np.uint8):
    """Two frames (32 x 32, or 12 x 24 x 24) and the table a fit of them would return: frame 0 holds
    clusters of 1, 2, 3 and 4 rows, frame 1 a pair, a window clipped on each side of each axis and a
    centre outside the frame; the rows of a frame are shuffled, so those of a cluster are not
    contiguous, and the labels of the two frames coincide.
    Returns (frames, params, frame_offset, cluster, diameter, mask_pos)."""
    shape = (32, 32) if ndim == 2 else (12, 24, 24)
    diameter = {(2, True): 9, (2, False): (7, 9), (3, True): 7, (3, False): (5, 7, 7)}[ndim, isotropic]
    _, nx, radius, _, n_params = _residual.model_of(fit, ndim, diameter)
    bands = (5., 14., 23.) if ndim == 2 else (4., 12., 20.)
    ahead = [0.] * (ndim - 2)
    frames, rows, labels, offsets = [], [], [], [0]
    for t in range(2):
        clusters = []
        if t == 0:
            for n, band, x in ((1, 0, 5.), (2, 0, shape[-1] * 0.62), (3, 1, shape[-1] * 0.45), (4, 2, shape[-1] * 0.45)):
                p = truth(rng, fit, extra, shape, diameter, n)
                p[:, 2 + ndim - 2] += bands[band] - shape[-2] / 2.
                p[:, 2 + ndim - 1] += x - shape[-1] / 2.
                clusters.append(p)
        else:
            clusters.append(truth(rng, fit, extra, shape, diameter, 2))
            mid = [s / 2. for s in shape]
            spots = []
            for a in range(ndim):
                for edge in (0.3, shape[a] - 1.3):
                    spot = list(mid)
                    spot[a] = edge
                    for b in range(ndim):
                        if b != a and ndim == 3:
                            spot[b] = mid[b] + (-6. if edge < 1. else 6.) * (1 if b > a else -1)
                    spots.append(spot)
            spots.append([-0.4 * radius[0]] + [5.5] * (ndim - 1))          # outside, part of its mask inside
            for spot in spots:
                p = truth(rng, fit, extra, shape, diameter, 1)
                p[0, 2:2 + ndim] = np.array(spot) + rng.uniform(-0.2, 0.2, ndim)
                clusters.append(p)
        true = np.concatenate(clusters)
        label = np.concatenate([[k] * len(p) for k, p in enumerate(clusters)])
        mix = rng.permutation(len(true))
        frames.append(draw(rng, shape, fit, true, dtype=pixel))
        rows.append(true[mix])
        labels.append(label[mix])
        offsets.append(offsets[-1] + len(true))
    params = fitted(rng, np.concatenate(rows), ndim)
    mask_pos = params[:, 2:2 + ndim] + rng.uniform(-0.3, 0.3, (len(params), ndim))
    return (np.stack(frames), params, np.array(offsets, dtype=np.int64), np.concatenate(labels).astype(np.int64),
            diameter, mask_pos)


def grid_table(rng, counts, shape=(96, 96), diameter=5, pitch=7):
    """one frame per entry of ``counts``, each one cluster of that many well-separated Gaussians on a grid
    of ``pitch`` pixels: (frames uint8, params, frame_offset, cluster, diameter)"""
    per_row = (shape[1] - 6) // pitch
    frames, rows, offsets = [], [], [0]
    for n in counts:
        assert n <= per_row * ((shape[0] - 6) // pitch)
        p = np.zeros((n, 5))
        p[:, 0], p[:, 1], p[:, 4] = 10., rng.uniform(100., 180., n), rng.uniform(0.95, 1.1, n)
        for k in range(n):
            p[k, 2:4] = np.array([5. + pitch * (k // per_row), 5. + pitch * (k % per_row)]) + rng.uniform(-0.4, 0.4, 2)
        frames.append(draw(rng, shape, 'gauss', p, noise=1.))
        rows.append(fitted(rng, p, 2))
        offsets.append(offsets[-1] + n)
    params = np.concatenate(rows)
    return np.stack(frames), params, np.array(offsets, dtype=np.int64), np.zeros(len(params), dtype=np.int64), diameter


def ring_dimer(rng=None):
    """a frame (uint8, 48 x 48) with two overlapping rings 5.5 px apart, their true params [2, 6] and the
    diameter the tests fit and measure them with"""
    rng = np.random.default_rng(41) if rng is None else rng
    p = np.array([[10., 150., 23.7, 21.4, 4.2, 0.45], [10., 140., 24.1, 26.9, 4.2, 0.45]])
    return draw(rng, (48, 48), 'ring', p, noise=1.5), p, 13
