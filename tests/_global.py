"""Yardstick of the global fit (``ctr_refine_global_device``, include/ctrefine.h): the objective of one
problem with shared and per-feature variables and its full analytic Jacobian in NumPy, in the
reference's vector order, with the round loop and a solve by ``scipy.optimize.least_squares``
under the box at machine-precision tolerances.  It generalises ``_train.Problem`` and imports
neither the reference nor the oracle; ``tests/test_global_rule.py`` pins it to fixtures made by the
reference (``tests/golden/make_golden_global.py``), ``tests/test_gpu_refine_global.py`` holds the
device against it."""
import json
import os

import numpy as np
from scipy.optimize import least_squares

from _train import _profile, param_names

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'global', 'global_cases.npz')

CONST, VAR, GLOBAL, CLUSTER = 0, 1, 2, 3
MODE_CODES = {'const': CONST, 'var': VAR, 'global': GLOBAL, 'cluster': CLUSTER}


def modes_of(fit_function, ndim, isotropic, param_mode=None):
    """fitfunc.py:356-394: background 'cluster', signal and positions 'var', the rest 'const'"""
    names = param_names(fit_function, ndim, isotropic)
    mode = dict(signal='var', background='cluster')
    mode.update(param_mode or {})
    pos = names[2:2 + ndim]
    sizes = names[2 + ndim:2 + ndim + (1 if isotropic else ndim)]
    if 'pos' in mode:
        for c in pos:
            mode.setdefault(c, mode['pos'])
    if not isotropic and 'size' in mode:
        for c in sizes:
            mode.setdefault(c, mode['size'])
    for c in pos:
        mode.setdefault(c, 'var')
    return [MODE_CODES[mode.get(c, 'const')] for c in names]


class Problem(object):
    """One problem: frames [T, ...], the parameter rows of its features, ``feat_offset`` [C + 1] over
    those rows, ``frame_index`` [C], one mode per column.  The variables in the reference's order
    (fitfunc.py:207-263): column by column, a ``var`` column one entry per row, a ``global`` column
    one, a ``cluster`` column one per cluster."""

    def __init__(self, frames, params, feat_offset, frame_index, diameter, fit_function='gauss', modes=None,
                 residual_factor=100000.):
        self.frames = np.asarray(frames)
        self.ndim = nd = self.frames.ndim - 1
        diameter = tuple(diameter) if hasattr(diameter, '__iter__') else (diameter,) * nd
        self.radius = tuple(int(d) // 2 for d in diameter)
        self.isotropic = all(d == diameter[0] for d in diameter)
        self.fit = fit_function if fit_function in ('gauss', 'ring', 'disc') else 'inv_series'
        self.names = param_names(fit_function, nd, self.isotropic)
        self.modes = list(modes_of(fit_function, nd, self.isotropic) if modes is None else modes)
        self.params = np.array(params, dtype=np.float64)
        self.nsz = 1 if self.isotropic else nd
        self.residual_factor = float(residual_factor)
        self.feat_offset = np.asarray(feat_offset).astype(np.int64)
        self.frame_index = np.asarray(frame_index).astype(np.int64)
        n, ncl = len(self.params), len(self.frame_index)
        self.cluster_of = np.repeat(np.arange(ncl), np.diff(self.feat_offset))
        # vidx[i, k]: the variable behind column k of row i, or -1
        self.vidx = -np.ones((n, len(self.modes)), dtype=np.int64)
        at = 0
        for k, m in enumerate(self.modes):
            if m == VAR:
                self.vidx[:, k] = at + np.arange(n)
                at += n
            elif m == GLOBAL:
                self.vidx[:, k] = at
                at += 1
            elif m == CLUSTER:
                self.vidx[:, k] = at + self.cluster_of
                at += ncl
        self.nvar = at
        self.global_vars = [int(self.vidx[0, k]) for k, m in enumerate(self.modes) if m == GLOBAL] if n else []
        fmax = 0.
        for t in np.unique(self.frame_index):
            fmax = max(fmax, float(self.frames[int(t)].max()))     # refine.py:325-331
        self.norm = fmax ** 2 / self.residual_factor
        self.set_windows(self.params[:, 2:2 + nd])

    def set_windows(self, coords):
        """refine.py:366 on the mask centres ``coords``"""
        coords = np.array(coords, dtype=np.float64)
        self.coords = coords
        self.clusters = []
        self.empty = False
        rad = np.array(self.radius)
        for c in range(len(self.frame_index)):
            rows = np.arange(self.feat_offset[c], self.feat_offset[c + 1])
            image = self.frames[int(self.frame_index[c])]
            co = coords[rows]
            ci = np.round(co).astype(np.int64)
            ok = np.all((ci >= -rad) & (ci < np.array(image.shape) + rad), axis=1)
            if not ok.any():
                self.empty = True      # refine.py:33-34
                continue
            lo = np.maximum(ci[ok].min(0) - rad, 0)
            hi = np.minimum(ci[ok].max(0) + rad + 1, image.shape)
            sub = image[tuple(slice(a, b) for a, b in zip(lo, hi))]
            idx = np.indices(sub.shape)
            dist = [np.sum(((idx.T - (x - lo)) / rad) ** 2, -1).T <= 1 for x in co]
            total = np.any(dist, axis=0)
            mesh = idx[:, total].astype(np.float64) + lo[:, None]
            self.clusters.append((rows, sub[total].astype(np.float64), mesh, [d[total] for d in dist]))
            if not total.any():
                self.empty = True

    # ---- the vector -----------------------------------------------------------------------------
    def pack(self, table, reduce):
        """``table`` [N, n_params] as a vector: own entries, ``reduce`` over the cluster's or all rows"""
        out = np.empty(self.nvar)
        for k, m in enumerate(self.modes):
            if m == VAR:
                out[self.vidx[:, k]] = table[:, k]
            elif m == GLOBAL:
                out[self.vidx[0, k]] = reduce(table[:, k])
            elif m == CLUSTER:
                for c in range(len(self.frame_index)):
                    r0, r1 = self.feat_offset[c], self.feat_offset[c + 1]
                    out[self.vidx[r0, k]] = reduce(np.ascontiguousarray(table[r0:r1, k]))
        return out

    def start(self):
        return self.pack(self.params, np.mean)

    def bounds(self, low_f, high_f):
        return self.pack(low_f, np.min), self.pack(high_f, np.max)

    def rows_of(self, x):
        """the parameter table at the vector ``x`` (fitfunc.py:266-315)"""
        p = self.params.copy()
        for k, m in enumerate(self.modes):
            if m != CONST:
                p[:, k] = np.asarray(x)[self.vidx[:, k]]
        return p

    # ---- the objective --------------------------------------------------------------------------
    def residuals(self, x, jac=False):
        """the weighted residual vector r (F = r.r) and, with ``jac``, dr/dx"""
        nd, nsz = self.ndim, self.nsz
        p = self.rows_of(np.asarray(x, dtype=np.float64))
        res, J = [], []
        for rows, image, mesh, masks in self.clusters:
            wgt = 1. / np.sqrt(len(image) * self.norm)
            diff = image - p[rows[0], 0]
            dj = np.zeros((self.nvar, len(image)))
            if jac and self.vidx[rows[0], 0] >= 0:
                dj[self.vidx[rows[0], 0]] -= 1.
            for i, mask in zip(rows, masks):
                d = mesh[:, mask] - p[i, 2:2 + nd, None]
                sizes = p[i, 2 + nd:2 + nd + nsz]
                s_ax = np.repeat(sizes, nd) if self.isotropic else sizes
                with np.errstate(divide='ignore', invalid='ignore'):
                    r2 = np.sum(d ** 2 / s_ax[:, None] ** 2, axis=0)
                    raw2 = np.sum(d ** 2, axis=0)
                    extra = p[i, 2 + nd + nsz:]
                    gval, dg, de = _profile(self.fit, r2, raw2, extra, nd)
                    sig = p[i, 1]
                    diff[mask] -= sig * gval
                    if jac:
                        cols = {1: -gval}
                        for a in range(nd):
                            cols[2 + a] = sig * dg * (2. * d[a] / s_ax[a] ** 2)
                        if self.isotropic:
                            cols[2 + nd] = -sig * dg * (np.sum(d ** 2, axis=0) * (-2. / sizes[0] ** 3))
                        else:
                            for a in range(nd):
                                cols[2 + nd + a] = -sig * dg * (d[a] ** 2 * (-2. / sizes[a] ** 3))
                        for q, dq in enumerate(de):
                            cols[2 + nd + nsz + q] = -sig * dq
                        for k, val in cols.items():
                            if self.vidx[i, k] >= 0:
                                dj[self.vidx[i, k], mask] += val
            bad = np.isnan(diff)        # np.nansum (fitfunc.py:449): the pixel drops out, P keeps it
            diff = np.where(bad, 0., diff)
            res.append(diff * wgt)
            if jac:
                dj = np.where(bad[None, :] | np.isnan(dj), 0., dj)
                J.append(dj * wgt)
        r = np.concatenate(res) if res else np.zeros(0)
        if jac:
            return r, (np.concatenate(J, axis=1).T if J else np.zeros((0, self.nvar)))
        return r

    def F(self, x):
        r = self.residuals(x)
        return float(r @ r)

    def grad(self, x):
        r, J = self.residuals(x, jac=True)
        return 2. * (J.T @ r)

    def cost(self, x):
        return np.sqrt(self.F(x) / self.residual_factor)

    def projected_gradient(self, x, low, high):
        """the gradient with the components that push against an active bound removed"""
        x = np.asarray(x, dtype=np.float64)
        gr = self.grad(x)
        at_lo = (x <= low) & (gr > 0)
        at_hi = (x >= high) & (gr < 0)
        return np.where(at_lo | at_hi | (low == high), 0., gr)

    # ---- the minimiser and the rounds -----------------------------------------------------------
    def solve(self, low, high, x0=None):
        x0 = self.start() if x0 is None else np.asarray(x0, dtype=np.float64)
        low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
        x = np.minimum(np.maximum(x0, low), high)
        pinned = ~(high > low)
        # trf keeps its iterates strictly inside the box and only creeps towards an active bound: a
        # variable that ends within 1e-7 (relative) of a bound with the gradient pushing outwards is put
        # on the bound and the rest is solved again, until no further variable is pinned
        for _ in range(4):
            free = ~pinned
            eps = 1e-12 * np.maximum(1., np.abs(x))
            z0 = np.minimum(np.maximum(x, low + np.where(np.isfinite(low), eps, 0.)),
                            high - np.where(np.isfinite(high), eps, 0.))[free]
            base = x.copy()

            def full(z):
                y = base.copy()
                y[free] = z
                return y
            out = least_squares(lambda z: self.residuals(full(z)), z0,
                                jac=lambda z: self.residuals(full(z), jac=True)[1][:, free],
                                bounds=(low[free], high[free]), method='trf', xtol=2.3e-16, ftol=2.3e-16, gtol=2.3e-16,
                                max_nfev=4000)
            x = full(out.x)
            g = self.grad(x)
            tol = 1e-7 * np.maximum(1., np.abs(x))
            at_lo = free & (x - low <= tol) & (g > 0)
            at_hi = free & (high - x <= tol) & (g < 0)
            if not (at_lo | at_hi).any():
                break
            x = np.where(at_lo, low, np.where(at_hi, high, x))
            pinned = pinned | at_lo | at_hi
        return x

    def refine(self, low, high, max_iter=10, max_shift=1., x0=None):
        """refine.py:365-388: ``(x, cost, rounds)``; every round from the start, the masks on the
        last round's positions"""
        nd = self.ndim
        x0 = self.start() if x0 is None else x0
        coords = self.params[:, 2:2 + nd]
        x, rounds = x0, 0
        for _ in range(int(max_iter)):
            self.set_windows(coords)
            x = self.solve(low, high, x0)
            rounds += 1
            new = self.rows_of(x)[:, 2:2 + nd]
            if np.all(np.sum((new - coords) ** 2, 1) < max_shift ** 2):
                break
            coords = new
        return x, self.cost(x), rounds


def host_vector(prob, shared, local):
    """the engine's tables -- ``shared`` [G] and ``local`` [C, max_locals], a cluster's locals in column
    order (a cluster column one entry, a var column one per row) -- as a vector in the reference's order"""
    out = np.full(prob.nvar, np.nan)
    g = 0
    for k, m in enumerate(prob.modes):
        if m == GLOBAL:
            out[prob.vidx[0, k]] = shared[g]
            g += 1
    for c in range(len(prob.frame_index)):
        r0, r1 = prob.feat_offset[c], prob.feat_offset[c + 1]
        at = 0
        for k, m in enumerate(prob.modes):
            if m == VAR:
                out[prob.vidx[r0:r1, k]] = local[c, at:at + r1 - r0]
                at += r1 - r0
            elif m == CLUSTER:
                out[prob.vidx[r0, k]] = local[c, at]
                at += 1
    return out


def column_error(prob, table, ref_table, fmax):
    """per column, the largest absolute difference over the column's scale: the frame maximum for
    background and signal, 1 px for positions, the reference value itself for the other columns"""
    nd = prob.ndim
    out = np.zeros(table.shape[1])
    for k in range(table.shape[1]):
        diff = np.abs(table[:, k] - ref_table[:, k])
        scale = fmax if k < 2 else (1. if k < 2 + nd else np.abs(ref_table[:, k]))
        out[k] = float(np.max(np.where(diff > 0, diff / scale, 0.))) if len(diff) else 0.
    return out


def load_cases():
    """{name: dict} of tests/golden/global/global_cases.npz"""
    z = np.load(GOLDEN, allow_pickle=False)
    cases = {}
    for name in json.loads(str(z['names'])):
        cases[name] = {key[len(name) + 1:]: z[key] for key in z.files if key.startswith(name + '/')}
        cases[name]['call'] = json.loads(str(cases[name]['call']))
    return cases


def case_modes(case):
    call = case['call']
    nd = case['frames'].ndim - 1
    dia = call['diameter'] if hasattr(call['diameter'], '__iter__') else (call['diameter'],) * nd
    return modes_of(call['fit_function'], nd, all(d == dia[0] for d in dia), call.get('param_mode'))


def problem_of(case):
    call = case['call']
    return Problem(case['frames'], case['params'], case['feat_offset'], case['frame_index'], call['diameter'],
                   call['fit_function'], modes=case_modes(case), residual_factor=call.get('residual_factor', 100000.))


def variable_scales(prob, x, fmax):
    """the scale of every variable, as :func:`column_error` measures its column: the frame maximum for
    background and signal, 1 px for positions, the value itself for sizes and profile columns"""
    nd = prob.ndim
    scale = np.abs(np.asarray(x, dtype=np.float64)).copy()
    for k, m in enumerate(prob.modes):
        if m != CONST and k < 2 + nd:
            scale[np.unique(prob.vidx[:, k])] = fmax if k < 2 else 1.
    return scale


def conditioning(prob, x, fmax):
    """ratio of the largest to the smallest singular value of the Jacobian at ``x``, its columns in the
    units of :func:`variable_scales`: how much further than sqrt(eps) a minimiser that judges steps by
    F stays from the minimum along the flattest direction"""
    sv = np.linalg.svd(prob.residuals(x, jac=True)[1] * variable_scales(prob, x, fmax), compute_uv=False)
    return float(sv[0] / sv[-1]) if len(sv) and sv[-1] > 0 else float('inf')
