"""The rule of ``ct.residual`` (clustertracking_amd/residual.py, include/ctrefine.h) restated in NumPy:
plain loops over the rows, float64, the same operations in the same order.  A helper module like
_shape.py; the CPU and GPU tests of the stage compare against it.

For pixel x of frame t and the rows i of that frame in ascending row order:
  Covering.  Row i covers x when sum(((x - mask_pos_i) / radius)**2) <= 1, evaluated as NumPy
    does: per axis a division, a product and a sum, in axis order, each rounded once; the edge is
    included.  The box of a mask is clipped to the frame: a centre outside the frame covers
    whatever part of its ellipse lies inside, a non-finite centre covers nothing.
  Per-pixel maps.  coverage(x) is the number of covering rows (int32), owner(x) the lowest
    covering row, or -1.
  Term of a row.  term_i(x) = signal_i * g(r2_i(x)), with r2 and g as the refine kernels evaluate
    them: d_a = x_a - pos_a, r2 = the sum over the axes, in axis order, of (d_a * d_a) * (1 / (size_a
    * size_a)), every operation rounded on its own.  gauss: g = exp(-0.5 ndim r2).  ring (e =
    thickness): r = sqrt(r2), num = r - 1 + e, g = exp(-0.5 ndim ((num / e) * (num / e))).  disc (e =
    disc_size): e <= 0 the Gaussian; else ds = e, or 0.999 where e >= 1; g = 1 unless r2 > ds ds,
    where u = (sqrt(r2) - ds) / (1 - ds), g = exp(u u ndim / -2).  inv_series_<N> (e[0 .. N]): g = e[0] / y,
    y = polyval([1, e[1], ..., e[N]], r2) in Horner's order.  For ring and disc these are the
    reference's r2_*_safe forms: where q = the sum of d_a d_a over the axes, last axis first, is
    below 1, g is NaN (the disc with disc_size > 0 has the value 1 there, as the reference's
    disc_func leaves it).
  Residual.  residual(x) = ((image(x) - background_owner) - term_i1) - term_i2 ... over the covering
    rows in ascending row order (fitfunc.py:443-448).
  Model.  model(x) = background_owner + s, where s starts from 0 and takes the terms of the
    covering rows in the same order.
  Outside every mask.  outside decides the residual: 0.0 ('zero'), NaN ('nan') or
    float64(image(x)) ('image'); model is 0.0, NaN or 0.0 respectively.
  Per feature [N].  n_pix: covered pixels; n_own: pixels with owner == i; n_nan: covered pixels
    whose residual is NaN; sum, sum_sq, max_abs: over its covered pixels whose residual is not NaN
    (the reference's nansum; 0 where there is none); own_sum_sq: the same over its owned pixels;
    rms = sqrt(sum_sq / n_pix), the divisor counting the NaN pixels as len(image) does there, NaN
    for n_pix == 0.  (The device adds in the fixed order given in the header; here NumPy's own.)
  Per cluster, only when cluster is given; per row [N], every row carrying its cluster's value.
    cluster_n_pix = the sum of n_own over the rows of the cluster, cluster_sum_sq = the sum of
    own_sum_sq, in ascending row order; cost = sqrt(cluster_sum_sq / cluster_n_pix) / max(frame_t).
"""
import collections
import os

import numpy as np

Residual = collections.namedtuple('Residual', [
    'residual', 'model', 'coverage', 'owner', 'n_pix', 'n_own', 'n_nan', 'sum', 'sum_sq', 'own_sum_sq', 'max_abs',
    'rms', 'cluster_n_pix', 'cluster_sum_sq', 'cost', 'scale', 'abs_sq'])

EPS = np.finfo(np.float64).eps


def model_of(fit_function, ndim, diameter):
    """(kind, profile parameters, radius, isotropic, n_params) of a call"""
    diameter = tuple(diameter) if hasattr(diameter, '__iter__') else (diameter,) * ndim
    radius = tuple(int(d) // 2 for d in diameter)
    isotropic = all(d == diameter[0] for d in diameter)
    if fit_function.startswith('inv_series_'):
        kind, nx = 'inv_series', int(fit_function.rsplit('_', 1)[1]) + 1
    else:
        kind, nx = fit_function, {'gauss': 0, 'ring': 1, 'disc': 1}[fit_function]
    return kind, nx, radius, isotropic, 2 + ndim + (1 if isotropic else ndim) + nx


def box_of(centre, radius, shape):
    """the clipped box of a mask, one pixel wider than centre -/+ radius: slices, or None where it is empty"""
    out = []
    for c, r, n in zip(centre, radius, shape):
        if not np.isfinite(c):
            return None
        lo, hi = max(c - float(r) - 1., 0.), min(c + float(r) + 1., float(n - 1))
        if not lo <= hi:
            return None
        out.append(slice(int(np.floor(lo)), int(np.ceil(hi)) + 1))
    return tuple(out)


def covering(grid, centre, radius):
    """ellipse_sum <= 1 on the pixel coordinates ``grid`` (one float64 array per axis)"""
    s = 0.
    for a in range(len(grid)):
        t = (grid[a] - centre[a]) / float(radius[a])
        s = s + t * t
    return s <= 1.


def profile(kind, ndim, r2, q, e):
    """g(r2) of the rule; q: the squared pixel distance to the centre; e: the profile parameters"""
    if kind == 'gauss':
        return np.exp(-0.5 * ndim * r2)
    if kind == 'inv_series':
        y = np.ones_like(r2)
        for t in range(1, len(e)):
            y = y * r2 + e[t]
        return e[0] / y
    if kind == 'ring':
        r = np.sqrt(r2)
        num = r - 1. + e[0]
        g = np.exp(-0.5 * ndim * ((num / e[0]) * (num / e[0])))
        g[q < 1.] = np.nan
        return g
    assert kind == 'disc'
    if e[0] > 0.:
        ds = 0.999 if e[0] >= 1. else e[0]
        g = np.where(r2 == r2, 1., np.nan)
        far = r2 > ds * ds
        u = (np.sqrt(r2[far]) - ds) / (1. - ds)
        g[far] = np.exp(u * u * ndim / -2.)
        g[q < 1.] = 1.
    else:
        g = np.exp(-0.5 * ndim * r2)
        g[q < 1.] = np.nan
    return g


def term_of(kind, ndim, isotropic, nx, grid, p):
    """signal * g(r2) of the row with the parameters p on the pixel coordinates grid, and |signal g|"""
    pos = p[2:2 + ndim]
    r2, d = 0., []
    for a in range(ndim):
        sz = p[2 + ndim + (0 if isotropic else a)]
        inv = 1. / (sz * sz)
        d.append(grid[a] - pos[a])
        r2 = r2 + (d[a] * d[a]) * inv
    q = 0.
    for a in range(ndim - 1, -1, -1):
        q = q + d[a] * d[a]
    r2, q = np.broadcast_arrays(r2, q)
    return p[1] * profile(kind, ndim, np.array(r2), np.array(q), p[len(p) - nx:])


def residual_np(frames, params, frame_offset, diameter, fit_function='gauss', mask_pos=None, cluster=None,
                outside='zero'):
    """The rule on ndarrays.  Besides the outputs of ``ct.residual_arrays`` (all of them): ``scale`` [T,
    ...] = |image| + |background| + sum |term| per pixel, and ``abs_sq`` [N] = the sum of residual**2 over
    the covered non-NaN pixels as computed here -- what the tolerances of the tests are made of."""
    frames = np.asarray(frames)
    params = np.asarray(params, dtype=np.float64)
    ndim = frames.ndim - 1
    shape = frames.shape[1:]
    kind, nx, radius, isotropic, n_params = model_of(fit_function, ndim, diameter)
    assert params.shape[1:] == (n_params,)
    n, n_frames = len(params), len(frames)
    centres = params[:, 2:2 + ndim] if mask_pos is None else np.asarray(mask_pos, dtype=np.float64)
    res = np.zeros(frames.shape)
    mdl = np.zeros(frames.shape)
    scale = np.abs(np.nan_to_num(frames.astype(np.float64), nan=0., posinf=0., neginf=0.))   # (a pixel that is no number adds nothing)
    cov = np.zeros(frames.shape, dtype=np.int32)
    own = np.full(frames.shape, -1, dtype=np.int32)
    n_pix, n_own, n_nan = (np.zeros(n, dtype=np.int64) for _ in range(3))
    s1, s2, so, mx = (np.zeros(n) for _ in range(4))
    rms = np.full(n, np.nan)
    boxes = [None] * n
    with np.errstate(all='ignore'):
        for t in range(n_frames):
            image = frames[t].astype(np.float64)
            s = np.zeros(shape)
            bg = np.zeros(shape)
            rows = range(int(frame_offset[t]), int(frame_offset[t + 1]))
            for i in rows:
                box = boxes[i] = box_of(centres[i], radius, shape)
                if box is None:
                    continue
                grid = np.meshgrid(*[np.arange(b.start, b.stop, dtype=np.float64) for b in box], indexing='ij', sparse=True)
                m = covering(grid, centres[i], radius)
                first = m & (cov[t][box] == 0)
                own[t][box][first] = i
                bg[box][first] = params[i, 0]
                res[t][box][first] = image[box][first] - params[i, 0]
                scale[t][box][first] += abs(params[i, 0])
                cov[t][box][m] += 1
                term = np.broadcast_to(term_of(kind, ndim, isotropic, nx, grid, params[i]), m.shape)
                res[t][box][m] = res[t][box][m] - term[m]
                s[box][m] = s[box][m] + term[m]
                scale[t][box][m] += np.nan_to_num(np.abs(term[m]), nan=0., posinf=0.)
            mdl[t] = bg + s
            out = cov[t] == 0
            res[t][out] = image[out] if outside == 'image' else {'zero': 0., 'nan': np.nan}[outside]
            mdl[t][out] = np.nan if outside == 'nan' else 0.
            for i in rows:
                if boxes[i] is None:
                    continue
                box = boxes[i]
                grid = np.meshgrid(*[np.arange(b.start, b.stop, dtype=np.float64) for b in box], indexing='ij', sparse=True)
                m = covering(grid, centres[i], radius)
                r = res[t][box][m]
                mine = own[t][box][m] == i
                ok = ~np.isnan(r)
                n_pix[i], n_own[i], n_nan[i] = m.sum(), mine.sum(), (~ok).sum()
                s1[i], s2[i], so[i] = r[ok].sum(), (r[ok] * r[ok]).sum(), (r[ok & mine] * r[ok & mine]).sum()
                mx[i] = np.abs(r[ok]).max() if ok.any() else 0.
        rms = np.sqrt(s2 / n_pix)
        c_n = c_sq = cost = None
        if cluster is not None:
            cluster = np.asarray(cluster)
            c_n, c_sq, cost = np.zeros(n, dtype=np.int64), np.zeros(n), np.full(n, np.nan)
            for t in range(n_frames):
                fmax = np.float64(frames[t].max()) if frames[t].size else np.nan
                for i in range(int(frame_offset[t]), int(frame_offset[t + 1])):
                    for j in range(int(cluster[i]), int(frame_offset[t + 1])):
                        if cluster[j] == cluster[i]:
                            c_n[i] += n_own[j]
                            c_sq[i] = c_sq[i] + so[j]
                    cost[i] = np.sqrt(c_sq[i] / c_n[i]) / fmax
    return Residual(res, mdl, cov, own, n_pix, n_own, n_nan, s1, s2, so, mx, rms, c_n, c_sq, cost, scale, s2.copy())


# ---- inputs the CPU and GPU tests share -------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'residual', 'residual_reference.npz')
Case = collections.namedtuple('Case', 'name fit frame params centres diameter value n_pix')

# (fit_function, profile parameters) of every profile, the disc on all three branches of disc_size
PROFILES = [('gauss', []), ('ring', [0.45]), ('disc', [0.]), ('disc', [0.5]), ('disc', [1.5]),
            ('inv_series_2', [1.25, 0.75, 1.5])]


def fixtures():
    """the cases of tests/golden/residual/residual_reference.npz (tests/golden/make_golden_residual.py)"""
    z = np.load(GOLDEN)
    out = []
    for name in z['names']:
        g = lambda key: z['%s__%s' % (name, key)]
        diameter = tuple(int(d) for d in g('diameter'))
        out.append(Case(str(name), str(g('fit')), g('frame'), g('params'), g('centres'), diameter,
                        float(g('value')), int(g('n_pix'))))
    return out


def random_cluster(rng, fit, extra, shape, diameter, n, spread=0.9):
    """(frame uint8, params [n, n_params], centres [n, ndim]) of one cluster of n features whose masks
    overlap: blobs on a noisy background, one background for the cluster, the mask centres a little off
    the positions"""
    ndim = len(shape)
    kind, nx, radius, isotropic, n_params = model_of(fit, ndim, diameter)
    base = np.array([s / 2. for s in shape]) + rng.uniform(-1, 1, ndim)
    step = np.zeros(ndim)
    step[-1] = radius[-1] * spread
    pos = np.array([base + (k - (n - 1) / 2.) * step + rng.uniform(-0.5, 0.5, ndim) for k in range(n)])
    sizes = rng.uniform(0.25, 0.4, (n, 1 if isotropic else ndim)) * np.array(radius[:1] if isotropic else radius)
    params = np.concatenate([np.full((n, 1), 8.5), rng.uniform(60, 150, (n, 1)), pos, sizes,
                             np.tile(np.array(extra, dtype=np.float64), (n, 1)).reshape(n, len(extra))], axis=1)
    assert params.shape[1] == n_params
    grid = np.indices(shape, dtype=np.float64)
    frame = rng.uniform(5, 25, shape)
    for k in range(n):
        r2 = sum(((grid[a] - pos[k, a]) / (0.35 * radius[a])) ** 2 for a in range(ndim))
        frame += params[k, 1] * np.exp(-0.5 * ndim * r2)
    frame = np.clip(np.round(frame), 0, 255).astype(np.uint8)
    return frame, params, pos + rng.uniform(-0.4, 0.4, pos.shape)


def plan_np(shape, n_frames, n_features, want_frames, has_cluster, cap=65536):
    """the launch decision of ctr_residual_device restated: (tile, chunk, n_tiles, grids, scratch_bytes)"""
    tile = (8, 32, 1) if len(shape) == 2 else (2, 8, 16)
    per_frame = int(np.prod([-(-s // t) for s, t in zip(shape, tile)]))
    n_tiles = n_frames * per_frame
    elems = n_frames * int(np.prod(shape))
    up = lambda b: -(-b // 256) * 256
    scratch = 256
    if not want_frames:
        scratch += up(8 * elems) + up(4 * elems)
    if has_cluster:
        scratch += 2 * up(8 * n_frames)
    cut = lambda n: max(1, min(n, cap))
    grids = (cut(-(-(n_frames + 1) // 256)), cut(n_tiles) if n_tiles else 0, cut(-(-n_features // 4)) if n_features else 0,
             cut(n_frames) if has_cluster and n_features else 0)
    return tile, 256, n_tiles, grids, scratch
