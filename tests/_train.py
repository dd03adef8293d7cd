"""Yardstick of the training stage (``ctr_train_device``, include/ctrefine.h): the objective of one
training problem and its analytic gradient in NumPy, written from the rule, minimised with
``scipy.optimize.least_squares`` under the box at machine-precision tolerances.  It imports
neither the reference nor the oracle; ``tests/test_train_rule.py`` pins it to fixtures made by the
reference (``tests/golden/make_golden_train.py``), ``tests/test_gpu_train.py`` holds the device
against it."""
import json
import os

import numpy as np
from scipy.optimize import least_squares

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'train', 'train_cases.npz')

CONST, GLOBAL = 0, 2


def param_names(fit_function, ndim, isotropic):
    pos = ['z', 'y', 'x'][-ndim:]
    sizes = ['size'] if isotropic else ['size_' + c for c in pos]
    if fit_function == 'gauss':
        extra = []
    elif fit_function == 'ring':
        extra = ['thickness']
    elif fit_function == 'disc':
        extra = ['disc_size']
    else:
        order = int(fit_function.rsplit('_', 1)[1])
        extra = ['signal_mult'] + ['param_' + chr(97 + i) for i in range(order)]
    return ['background', 'signal'] + pos + sizes + extra


def default_modes(fit_function, ndim, isotropic):
    """positions, signal and background constant, the rest global"""
    names = param_names(fit_function, ndim, isotropic)
    return [CONST if k < 2 + ndim else GLOBAL for k in range(len(names))]


def _profile(fit, r2, raw2, extra, ndim):
    """value, d/dr2 and [d/d extra] of the radial profile; NaN inside r2_*_safe's hole"""
    if fit == 'gauss':
        g = np.exp(-0.5 * ndim * r2)
        return g, -0.5 * ndim * g, []
    if fit == 'ring':
        t = extra[0]
        r2 = np.where(raw2 < 1., np.nan, r2)
        r = np.sqrt(r2)
        num = r - 1 + t
        g = np.exp(-0.5 * ndim * (num / t) ** 2)
        return g, g * (-0.5 * ndim / (r * t ** 2)) * num, [g * ndim * (num ** 2 / t ** 3 - num / t ** 2)]
    if fit == 'disc':
        ds = extra[0]
        r2 = np.where(raw2 < 1., np.nan, r2)
        if ds <= 0:
            g = np.exp(-0.5 * ndim * r2)
            return g, -0.5 * ndim * g, [np.zeros_like(g)]
        clamped = ds >= 1.
        if clamped:
            ds = 0.999
        g = np.ones_like(r2)
        dg = np.zeros_like(r2)
        de = np.zeros_like(r2)
        with np.errstate(invalid='ignore'):
            out = r2 > ds ** 2     # a NaN compares False: the value stays 1 there (fitfunc.py:121-131)
        r = np.sqrt(r2[out])
        w = 1. - ds
        u = (r - ds) / w
        f = np.exp(u * u * ndim / -2.)
        g[out] = f
        dg[out] = f * (-ndim * u / w) / (2. * r)
        de[out] = 0. if clamped else f * (-ndim * u) * ((r - 1.) / (w * w))
        return g, dg, [de]
    # inv_series_<N>: extra[0] / polyval([1, extra[1], ...], r2)
    c = np.array(extra, dtype=np.float64)
    c[0] = 1.
    y = np.polyval(c, r2)
    dy = np.polyval(np.polyder(c), r2) if len(c) > 1 else np.zeros_like(r2)
    n = len(c) - 1
    g = extra[0] / y
    de = [1. / y] + [-extra[0] * r2 ** (n - k) / y ** 2 for k in range(1, n + 1)]
    return g, -extra[0] * dy / y ** 2, de


class Problem(object):
    """One training problem: frames [T, ...], the parameter rows of its features, ``feat_offset``
    [C + 1] over those rows, ``frame_index`` [C]."""

    def __init__(self, frames, params, feat_offset, frame_index, diameter, fit_function='gauss', modes=None,
                 residual_factor=100000.):
        frames = np.asarray(frames)
        self.ndim = nd = frames.ndim - 1
        diameter = tuple(diameter) if hasattr(diameter, '__iter__') else (diameter,) * nd
        self.radius = tuple(int(d) // 2 for d in diameter)
        self.isotropic = all(d == diameter[0] for d in diameter)
        self.fit = fit_function if fit_function in ('gauss', 'ring', 'disc') else 'inv_series'
        self.names = param_names(fit_function, nd, self.isotropic)
        self.modes = list(default_modes(fit_function, nd, self.isotropic) if modes is None else modes)
        self.cols = [k for k, m in enumerate(self.modes) if m == GLOBAL]
        self.params = np.array(params, dtype=np.float64)
        self.nsz = 1 if self.isotropic else nd
        self.residual_factor = float(residual_factor)
        feat_offset = np.asarray(feat_offset)
        fmax = 0.
        for t in np.unique(frame_index):
            fmax = max(fmax, float(frames[int(t)].max()))     # refine.py:325-331
        self.norm = fmax ** 2 / self.residual_factor
        self.clusters = []
        self.empty = False
        rad = np.array(self.radius)
        for c in range(len(frame_index)):
            rows = np.arange(feat_offset[c], feat_offset[c + 1])
            image = frames[int(frame_index[c])]
            coords = self.params[rows, 2:2 + nd]
            ci = np.round(coords).astype(np.int64)
            ok = np.all((ci >= -rad) & (ci < np.array(image.shape) + rad), axis=1)
            if not ok.any():
                self.empty = True      # refine.py:33-34
                continue
            lo = np.maximum(ci[ok].min(0) - rad, 0)
            hi = np.minimum(ci[ok].max(0) + rad + 1, image.shape)
            sub = image[tuple(slice(a, b) for a, b in zip(lo, hi))]
            idx = np.indices(sub.shape)
            dist = [np.sum(((idx.T - (co - lo)) / rad) ** 2, -1).T <= 1 for co in coords]
            total = np.any(dist, axis=0)
            mesh = idx[:, total].astype(np.float64) + lo[:, None]
            self.clusters.append((rows, sub[total].astype(np.float64), mesh, [d[total] for d in dist]))
            if not total.any():
                self.empty = True

    def start(self):
        return np.array([np.mean(self.params[:, k]) for k in self.cols])

    def _rows(self, g):
        p = self.params.copy()
        for v, k in enumerate(self.cols):
            p[:, k] = g[v]
        return p

    def residuals(self, g, jac=False):
        """the weighted residual vector r (F = r.r) and, with ``jac``, dr/dg"""
        nd, nsz = self.ndim, self.nsz
        p = self._rows(np.asarray(g, dtype=np.float64))
        res, J = [], []
        slot = {k: v for v, k in enumerate(self.cols)}
        for rows, image, mesh, masks in self.clusters:
            wgt = 1. / np.sqrt(len(image) * self.norm)
            diff = image - p[rows[0], 0]
            dj = np.zeros((len(self.cols), len(image)))
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
                        if self.isotropic:
                            dsz = [np.sum(d ** 2, axis=0) * (-2. / sizes[0] ** 3)]
                        else:
                            dsz = [d[a] ** 2 * (-2. / sizes[a] ** 3) for a in range(nd)]
                        for q in range(nsz):
                            k = 2 + nd + q
                            if k in slot:
                                dj[slot[k], mask] -= sig * dg * dsz[q]
                        for q, dq in enumerate(de):
                            k = 2 + nd + nsz + q
                            if k in slot:
                                dj[slot[k], mask] -= sig * dq
            bad = np.isnan(diff)        # np.nansum (fitfunc.py:449): the pixel drops out, P keeps it
            diff = np.where(bad, 0., diff)
            res.append(diff * wgt)
            if jac:
                dj = np.where(bad[None, :] | np.isnan(dj), 0., dj)
                J.append(dj * wgt)
        r = np.concatenate(res) if res else np.zeros(0)
        if jac:
            return r, (np.concatenate(J, axis=1).T if J else np.zeros((0, len(self.cols))))
        return r

    def F(self, g):
        r = self.residuals(g)
        return float(r @ r)

    def grad(self, g):
        r, J = self.residuals(g, jac=True)
        return 2. * (J.T @ r)

    def cost(self, g):
        return np.sqrt(self.F(g) / self.residual_factor)

    def projected_gradient(self, g, low, high):
        """the gradient with the components that push against an active bound removed"""
        g = np.asarray(g, dtype=np.float64)
        gr = self.grad(g)
        at_lo = (g <= low) & (gr > 0)
        at_hi = (g >= high) & (gr < 0)
        return np.where(at_lo | at_hi, 0., gr)

    def solve(self, low, high, x0=None):
        x0 = self.start() if x0 is None else np.asarray(x0, dtype=np.float64)
        low, high = np.asarray(low, dtype=np.float64), np.asarray(high, dtype=np.float64)
        eps = 1e-12 * np.maximum(1., np.abs(x0))
        x0 = np.minimum(np.maximum(x0, low + np.where(np.isfinite(low), eps, 0.)),
                        high - np.where(np.isfinite(high), eps, 0.))
        out = least_squares(lambda g: self.residuals(g), x0, jac=lambda g: self.residuals(g, jac=True)[1],
                            bounds=(low, high), method='trf', xtol=2.3e-16, ftol=2.3e-16, gtol=2.3e-16,
                            max_nfev=2000)
        return out.x


def load_cases():
    """{name: dict} of tests/golden/train/train_cases.npz"""
    z = np.load(GOLDEN, allow_pickle=False)
    cases = {}
    for name in json.loads(str(z['names'])):
        cases[name] = {key[len(name) + 1:]: z[key] for key in z.files if key.startswith(name + '/')}
        cases[name]['call'] = json.loads(str(cases[name]['call']))
    return cases


def problem_of(case):
    call = case['call']
    return Problem(case['frames'], case['params'], case['feat_offset'], case['frame_index'], call['diameter'],
                   call['fit_function'], residual_factor=call.get('residual_factor', 100000.))
