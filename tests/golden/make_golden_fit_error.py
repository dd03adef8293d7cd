"""Generate tests/golden/fit_error/fit_error_cases.npz from the REFERENCE: its objective
(``FitFunctions.get_residual``, fitfunc.py:421-489) at a fitted point of small clusters, its gradient
where it has one, and a Hessian from central differences.

Run in the build container only (needs /root/reference; see oracle/refshim.py):

    python tests/golden/make_golden_fit_error.py

The file holds data only: per case the frame, the parameter rows of the one cluster, the call (JSON),
the packed vector of ``vect_from_params``, ``F``, the reference's gradient (gauss and ring; the disc and
inv_series profiles have none, fitfunc.py:452-453) and ``hessian``.  Where the reference has a
Jacobian, the Hessian is its central difference with the step ``STEP_J`` (relative to max(1, |v|)),
made symmetric; where it has none, the second central difference of F itself with ``STEP_F``.
``hessian_from`` says which.  The inputs come from tests/_fit_error.py (``truth``, ``draw``, ``fitted``);
every cluster is positive definite in its restatement (checked here, and again by the test).
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402,F401  (loads the reference through oracle/refshim.py)
from make_golden import ct_refine, FitFunctions, vect_from_params  # noqa: E402
import _fit_error as rule  # noqa: E402

STEP_J = 1e-6
STEP_F = 1e-4


class Reader(object):
    def __init__(self, frames):
        self.frames = frames
        self.frame_shape = frames.shape[1:]

    def __getitem__(self, i):
        return self.frames[i]


def run_case(name, frame, params, call):
    ndim = frame.ndim
    diameter = call['diameter']
    dia = tuple(diameter) if hasattr(diameter, '__iter__') else (diameter,) * ndim
    radius = tuple(int(d) // 2 for d in dia)
    isotropic = all(d == dia[0] for d in dia)
    fit = call['fit_function']
    ff = FitFunctions(fit, ndim, isotropic, call.get('param_mode'))
    n = len(params)
    groups = [[np.arange(n)]]
    frames = frame[None]
    norm = float(frame.max()) ** 2 / 100000.
    vect = vect_from_params(params, ff.modes, groups, operation=np.mean)
    sub, meshes, masks = ct_refine.prepare_subimages(params[:, 2:2 + ndim], groups, np.zeros(n, dtype=int), Reader(frames), radius)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        residual, jacobian = ff.get_residual(sub, meshes, masks, params, groups, norm)
        nv = len(vect)
        step = lambda h: h * np.maximum(1., np.abs(vect))
        case = {'frame': frame, 'params': params, 'call': np.array(json.dumps(call)), 'vect': vect,
                'F': np.array(residual(vect))}
        hess = np.zeros((nv, nv))
        if jacobian is not None:
            case['grad'] = np.array(jacobian(vect))
            h = step(STEP_J)
            for k in range(nv):
                e = np.zeros(nv)
                e[k] = h[k]
                hess[:, k] = (jacobian(vect + e) - jacobian(vect - e)) / (2. * h[k])
            hess = 0.5 * (hess + hess.T)
            case['hessian_from'] = np.array('jacobian')
        else:
            h = step(STEP_F)
            f0 = residual(vect)
            for i in range(nv):
                ei = np.zeros(nv)
                ei[i] = h[i]
                hess[i, i] = (residual(vect + ei) - 2. * f0 + residual(vect - ei)) / (h[i] * h[i])
                for j in range(i):
                    ej = np.zeros(nv)
                    ej[j] = h[j]
                    hess[i, j] = hess[j, i] = (residual(vect + ei + ej) - residual(vect + ei - ej) - residual(vect - ei + ej)
                                               + residual(vect - ei - ej)) / (4. * h[i] * h[j])
            case['hessian_from'] = np.array('objective')
    case['hessian'] = hess
    # the condition of the fixture: positive definite in the restatement
    modes = rule.modes_of(fit, ndim, isotropic, call.get('param_mode'))
    c = rule.Cluster(frame, params, params[:, 2:2 + ndim], diameter, fit, modes)
    status, std, _ = rule.cluster_result(c)
    assert status == rule.OK, (name, status)
    mine = c.hessian(c.vect())
    print('%-22s nv=%2d P=%3d F=%.6g  restatement vs reference: F %.1e hessian %.1e (of the largest entry)' % (
        name, nv, c.n_pix, case['F'], abs(c.objective(c.vect()) - case['F']) / case['F'],
        np.abs(mine - hess).max() / np.abs(hess).max()))
    return case


def main():
    cases = {}
    rng = np.random.default_rng(2024)

    def add(name, shape, fit, extra, n, diameter, param_mode=None, move=None):
        ndim = len(shape)
        true = rule.truth(rng, fit, extra, shape, diameter, n)
        if move is not None:
            true[:, 2:2 + ndim] += np.array(move) - true[:, 2:2 + ndim].mean(axis=0)
        frame = rule.draw(rng, shape, fit, true)
        params = rule.fitted(rng, true, ndim)
        call = dict(diameter=diameter, fit_function=fit)
        if param_mode:
            call['param_mode'] = param_mode
        cases[name] = run_case(name, frame, params, call)

    add('gauss2d_pair', (32, 32), 'gauss', [], 2, 9)
    add('gauss3d_aniso_single', (12, 24, 24), 'gauss', [], 1, (5, 7, 7))
    add('ring2d_pair_var', (32, 32), 'ring', [0.45], 2, 9, dict(thickness='var'))
    add('ring2d_pair_cluster', (32, 32), 'ring', [0.45], 2, 9, dict(thickness='cluster'))
    add('disc2d_pair', (32, 32), 'disc', [0.5], 2, 9, dict(disc_size='var'))
    add('inv2_2d_pair', (32, 32), 'inv_series_2', [1.25, 0.75, 1.5], 2, 9, dict(signal_mult='const', param_a='var', param_b='var'))
    add('gauss2d_corner', (32, 32), 'gauss', [], 1, 9, move=[1.3, 29.8])

    out = {'names': np.array(json.dumps(list(cases)))}
    for name, case in cases.items():
        for key, val in case.items():
            out[name + '/' + key] = val
    os.makedirs(os.path.join(HERE, 'fit_error'), exist_ok=True)
    path = os.path.join(HERE, 'fit_error', 'fit_error_cases.npz')
    np.savez_compressed(path, **out)
    print('%s: %d cases, %.1f KB' % (path, len(cases), os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
