"""``ct.fit_error`` on the MI355X (ctr_fit_error_device) against the NumPy restatement of its rule
(tests/_fit_error.py): every <ND, ISO, FIT> instantiation, the parameter modes, the pixel types, the
size classes and the caps, the statuses, the engine's own Gaussian errors, the same bytes on every
call, and the use the stage exists for: the error of the distance of two overlapping rings.

Bounds.  The device and the restatement form the same sums in different orders and factor the same
matrix, so their difference is rounding amplified by the condition of A.  It was measured on the
cases of this file (the figures are printed by every test): the worst relative difference of a std
was 8.5e-14 and of a covariance entry, relative to sqrt(cov_ii cov_jj), 1.7e-13 (both on inv_series_2, 3D,
with param_a per row and param_b per cluster; most cases stay below 1e-14); with the margin of
eight that the residual stage takes, REL_STD and REL_COV.  Against the engine's own ``params_std``
(pinned to the oracle at 1e-6) the worst was 5.4e-16; with a margin of ten, REL_ENGINE."""
import importlib

import numpy as np
import pytest

import _fit_error as rule
import clustertracking_amd as ct

pytestmark = pytest.mark.gpu
fit_error = importlib.import_module('clustertracking_amd.fit_error')

REL_STD = 8 * 8.5e-14
REL_COV = 8 * 1.7e-13
REL_ENGINE = 10 * 5.4e-16
EXTRA = dict(rule.PROFILES)
SEEN = {'std': 0., 'cov': 0.}


def compare(got, want, what):
    """status, n_vars and n_pix equal; params_std and cov within the bounds; prints the figures"""
    np.testing.assert_array_equal(got.status, want.status, err_msg=what)
    np.testing.assert_array_equal(got.n_vars, want.n_vars, err_msg=what)
    np.testing.assert_array_equal(got.n_pix, want.n_pix, err_msg=what)
    assert np.array_equal(np.isnan(got.params_std), np.isnan(want.params_std)), what
    ok = ~np.isnan(want.params_std)
    d_std = np.max(np.abs(got.params_std[ok] - want.params_std[ok]) / want.params_std[ok]) if ok.any() else 0.
    d_cov = 0.
    if got.cov is not None:
        np.testing.assert_array_equal(got.cov_offset, want.cov_offset, err_msg=what)
        np.testing.assert_array_equal(got.var_row, want.var_row, err_msg=what)
        np.testing.assert_array_equal(got.var_col, want.var_col, err_msg=what)
        assert np.array_equal(np.isnan(got.cov), np.isnan(want.cov)), what
        for c in range(len(want.cov_offset) - 1):
            a, b = want.cov_offset[c:c + 2]
            nv = int(round(np.sqrt(b - a)))
            w, g = want.cov[a:b].reshape(nv, nv), got.cov[a:b].reshape(nv, nv)
            if nv == 0 or np.isnan(w).any():
                continue
            assert np.array_equal(g, g.T), what
            scale = np.sqrt(np.outer(np.diag(w), np.diag(w)))
            d_cov = max(d_cov, np.max(np.abs(g - w) / scale))
    SEEN['std'], SEEN['cov'] = max(SEEN['std'], d_std), max(SEEN['cov'], d_cov)
    print('%s: rows %d, statuses %s, worst relative difference std %.2e cov %.2e (so far %.2e, %.2e)'
          % (what, len(want.status), np.bincount(want.status, minlength=5).tolist(), d_std, d_cov, SEEN['std'], SEEN['cov']))
    assert d_std <= REL_STD and d_cov <= REL_COV, (what, d_std, d_cov)


def run(frames, params, offs, cluster, diameter, fit, mode, mask_pos, what):
    got = ct.fit_error_arrays(frames, params, offs, cluster, diameter, fit, mode, mask_pos, want_cov=True)
    want = rule.fit_error_np(frames, params, offs, cluster, diameter, fit, mode, mask_pos)
    compare(got, want, what)
    return got, want


# ---- 1. the device against the restatement -------------------------------------------------------------------
@pytest.mark.parametrize('iso', [True, False], ids=['iso', 'aniso'])
@pytest.mark.parametrize('ndim', [2, 3])
@pytest.mark.parametrize('fit', list(EXTRA))
def test_every_instantiation_against_restatement(fit, ndim, iso, engine):
    """clusters of 1 to 4 rows that are not contiguous, two frames with the same labels, windows clipped on
    each side and axis and a centre outside; masks on the positions and off them; the default modes and the
    profile's own parameters free"""
    rng = np.random.default_rng(100 + 10 * ndim + iso)
    frames, params, offs, cluster, diameter, mask_pos = rule.table(rng, fit, EXTRA[fit], ndim, iso)
    got, want = run(frames, params, offs, cluster, diameter, fit, None, mask_pos, '%s %dD %s, masks given' % (fit, ndim, iso))
    assert 2 * (want.status == rule.OK).sum() > len(params)          # (a window cut by the frame edge may leave too little)
    run(frames, params, offs, cluster, diameter, fit, None, None, '%s %dD %s, masks on the positions' % (fit, ndim, iso))
    for mode in rule.PROFILE_MIXES[fit]:
        run(frames, params, offs, cluster, diameter, fit, mode, None, '%s %dD %s, %s' % (fit, ndim, iso, mode))


@pytest.mark.parametrize('mode', rule.MODE_MIXES[1:], ids=['sizes-var', 'size-cluster', 'signal-cluster', 'signal-only'])
def test_parameter_modes(mode, engine):
    for fit, ndim, iso in (('gauss', 2, True), ('ring', 2, False), ('gauss', 3, False)):
        rng = np.random.default_rng(7)
        frames, params, offs, cluster, diameter, mask_pos = rule.table(rng, fit, EXTRA[fit], ndim, iso)
        run(frames, params, offs, cluster, diameter, fit, mode, mask_pos, '%s %dD %s, %s' % (fit, ndim, iso, mode))


def test_cluster_variable_takes_the_mean_of_unequal_rows(engine):
    rng = np.random.default_rng(9)
    frames, params, offs, cluster, diameter, _ = rule.table(rng, 'gauss', [], 2, True)
    run(frames, params, offs, cluster, diameter, 'gauss', dict(size='cluster', signal='cluster'), None, 'unequal rows of a cluster variable')


@pytest.mark.parametrize('pixel', [np.uint8, np.uint16, np.float64], ids=['u8', 'u16', 'f64'])
def test_pixel_types(pixel, engine):
    rng = np.random.default_rng(11)
    frames, params, offs, cluster, diameter, mask_pos = rule.table(rng, 'disc', EXTRA['disc'], 2, True, pixel=pixel)
    assert frames.dtype == pixel
    if pixel == np.float64:
        frames[0, 14, 14] = np.nan          # a NaN pixel: counted in P, in no sum
    run(frames, params, offs, cluster, diameter, 'disc', None, mask_pos, 'disc, %s' % np.dtype(pixel).name)


# ---- 2. the size classes and the caps ------------------------------------------------------------------------
def test_tile_and_cap_edges(engine):
    rng = np.random.default_rng(13)
    frames, params, offs, cluster, diameter = rule.grid_table(rng, [5, 42, 43])
    got, _ = run(frames, params, offs, cluster, diameter, 'gauss', None, None, '5, 42 and 43 rows')
    assert got.n_vars[[0, 5, 47]].tolist() == [16, 127, 130]
    assert got.status[[0, 5, 47]].tolist() == [fit_error.OK, fit_error.OK, fit_error.TOO_LARGE]
    got, _ = run(frames[:1], params[:5], offs[:2], cluster[:5], diameter, 'gauss', dict(size='cluster'), None, '5 rows, 17 variables')
    assert got.n_vars.tolist() == [17] * 5 and (got.status == fit_error.OK).all()
    frames, params, offs, cluster, diameter = rule.grid_table(rng, [64, 65])
    got, _ = run(frames, params, offs, cluster, diameter, 'gauss', dict(pos='const'), None, '64 and 65 rows, the signals alone')
    assert got.n_vars[[0, 64]].tolist() == [65, 66]
    assert got.status[[0, 64]].tolist() == [fit_error.OK, fit_error.TOO_LARGE]
    assert np.isnan(got.params_std[64:]).all() and got.cov_offset[2] == got.cov_offset[1]


# ---- 3. statuses as data ------------------------------------------------------------------------------------
def test_statuses_are_data_and_leave_the_other_clusters_alone(engine):
    rng = np.random.default_rng(17)
    frames, params, offs, cluster, diameter, _ = rule.table(rng, 'gauss', [], 2, True)
    clean = ct.fit_error_arrays(frames, params, offs, cluster, diameter, want_cov=True)
    n0 = int(offs[1])
    zero = np.flatnonzero(cluster[:n0] == 1)[0]           # a row of the pair: no signal, free positions
    nan = np.flatnonzero(cluster[:n0] == 2)[0]            # a row of the triple
    away = n0 + np.flatnonzero(cluster[n0:] == 1)[0]      # a single of frame 1, moved far outside
    bad = params.copy()
    bad[zero, 1] = 0.
    bad[nan, 4] = np.nan
    bad[away, 2:4] = [-40., 70.]
    got, want = run(frames, bad, offs, cluster, diameter, 'gauss', None, None, 'no signal, a NaN size, a cluster outside')
    assert got.status[zero] == fit_error.NOT_POSITIVE_DEFINITE and got.status[nan] == fit_error.NONFINITE
    assert got.status[away] == fit_error.EMPTY and got.n_pix[away] == 0
    touched = np.zeros(len(params), dtype=bool)
    touched[:n0] = np.isin(cluster[:n0], [1, 2])
    touched[away] = True
    for name in ('params_std', 'status', 'n_vars', 'n_pix'):
        assert getattr(got, name)[~touched].tobytes() == getattr(clean, name)[~touched].tobytes(), name
    assert np.isnan(got.params_std[touched]).all()


# ---- 4. the tie to the pinned path ---------------------------------------------------------------------------
def test_agrees_with_the_engines_own_gaussian_errors(engine):
    rng = np.random.default_rng(19)
    true = np.concatenate([rule.truth(rng, 'gauss', [], (32, 32), 9, n) + shift for n, shift in
                           ((1, [0, 0, -9., -9., 0]), (2, [0, 0, -8., 5., 0]), (2, [0, 0, 7., -4., 0]), (1, [0, 0, 9., 9., 0]))])
    frames = rule.draw(rng, (32, 32), 'gauss', true)[None]
    offs = np.array([0, len(true)], dtype=np.int64)
    start = true[:, 2:4] + rng.uniform(-0.2, 0.2, (len(true), 2))
    res = ct.refine_arrays(frames, start, offs, 9, signal=true[:, 1], size=true[:, 4], background=12., compute_error=True, max_iter=1)
    got = ct.fit_error_arrays(frames, res.params, offs, res.cluster, 9, mask_pos=start)
    index = np.unique(res.cluster, return_inverse=True)[1].reshape(-1)
    ok = (np.asarray(res.status)[index] == 0) & (got.status == fit_error.OK)
    print('rows of converged clusters: %d of %d' % (ok.sum(), len(ok)))
    assert ok.any()
    assert np.array_equal(np.isnan(got.params_std[ok]), np.isnan(res.params_std[ok]))
    fin = ok[:, None] & ~np.isnan(res.params_std)
    worst = np.max(np.abs(got.params_std[fin] - res.params_std[fin]) / res.params_std[fin])
    print('worst relative difference to the engine\'s own params_std: %.2e' % worst)
    assert worst <= REL_ENGINE


# ---- 5. the same bytes ---------------------------------------------------------------------------------------
def test_same_bytes_again_alone_on_another_stream_and_without_a_host_read(engine, monkeypatch):
    import torch
    rng = np.random.default_rng(23)
    frames, params, offs, cluster, diameter, mask_pos = rule.table(rng, 'ring', EXTRA['ring'], 2, True)
    call = lambda *a, **k: ct.fit_error_arrays(*a, fit_function='ring', param_mode=dict(thickness='var'), **k)
    first = call(frames, params, offs, cluster, diameter, mask_pos=mask_pos, want_cov=True)
    again = call(frames, params, offs, cluster, diameter, mask_pos=mask_pos, want_cov=True)
    for f in fit_error.FitError._fields:
        assert getattr(first, f).tobytes() == getattr(again, f).tobytes(), f
    # the triple of frame 0 alone
    rows = np.flatnonzero(cluster[:offs[1]] == 2)
    alone = call(frames[:1], params[rows], [0, len(rows)], cluster[rows], diameter, mask_pos=mask_pos[rows], want_cov=True)
    for f in ('params_std', 'status', 'n_vars', 'n_pix'):
        assert getattr(alone, f).tobytes() == getattr(first, f)[rows].tobytes(), f
    assert alone.cov.tobytes() == first.cov[first.cov_offset[2]:first.cov_offset[3]].tobytes()
    dev = torch.device('cuda', 0)
    tens = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (frames, params, offs, cluster, mask_pos)]
    n_clusters = len(first.cov_offset) - 1
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize(dev)

    def refuse(*a, **k):
        raise AssertionError('a host read')
    with monkeypatch.context() as m:
        for name in ('item', 'cpu', 'numpy', 'tolist', '__bool__', '__int__', '__float__', '__index__'):
            m.setattr(torch.Tensor, name, refuse)
        with torch.cuda.stream(stream):
            other = call(tens[0], tens[1], tens[2], tens[3], diameter, mask_pos=tens[4], n_clusters=n_clusters)
    stream.synchronize()
    assert isinstance(other.params_std, torch.Tensor) and other.params_std.device == dev and other.cov is None
    for f in ('params_std', 'status', 'n_vars', 'n_pix'):
        assert getattr(other, f).cpu().numpy().tobytes() == getattr(first, f).tobytes(), f
    wrong = call(tens[0], tens[1], tens[2], tens[3], diameter, mask_pos=tens[4], n_clusters=n_clusters - 1)
    assert (wrong.status.cpu().numpy() == fit_error.BAD_TABLE).all() and np.isnan(wrong.params_std.cpu().numpy()).all()


# ---- 6. end to end -------------------------------------------------------------------------------------------
def test_ring_dimer_gets_its_errors_and_the_error_of_its_bond(engine):
    pd = pytest.importorskip('pandas')
    frame, true, diameter = rule.ring_dimer()
    f = pd.DataFrame(dict(y=true[:, 2] + [0.2, -0.1], x=true[:, 3] + [-0.2, 0.1], signal=true[:, 1], size=true[:, 4], frame=0))
    fitted = ct.refine_leastsq(f, ct.ArrayReader(frame[None]), diameter, fit_function='ring', param_val=dict(thickness=0.45, background=10.),
                               compute_error=True)
    assert not np.isnan(fitted['cost']).any() and np.isnan(fitted[['y_std', 'x_std', 'signal_std']].values).all()
    out = ct.fit_error(fitted, ct.ArrayReader(frame[None]), diameter, fit_function='ring')
    assert (out['std_status'] == fit_error.OK).all() and list(out.index) == list(fitted.index)
    std = out[['background_std', 'signal_std', 'y_std', 'x_std']].values
    assert np.isfinite(std).all() and (std > 0).all() and np.isnan(out['size_std']).all() and np.isnan(out['thickness_std']).all()
    ff = ct.FitFunctions('ring', 2, True)
    params = out[[c for c in ff.params]].values
    res = ct.fit_error_arrays(frame[None], params, [0, 2], out['cluster'].values.astype(np.int64), diameter, 'ring', want_cov=True)
    np.testing.assert_array_equal(res.params_std[:, 1:4], out[['signal_std', 'y_std', 'x_std']].values)
    bond = ct.fit_error.distance_std(res, params, 0, 1)
    rss = np.sqrt(np.sum(res.params_std[:, 2:4] ** 2))
    want = rule.fit_error_np(frame[None], params, [0, 2], [0, 0], diameter, 'ring')
    block = want.cov.reshape(7, 7)
    where = [int(np.flatnonzero((want.var_row == r) & (want.var_col == c))[0]) for r in (0, 1) for c in (2, 3)]
    bond_np = rule.distance_std_np(block[np.ix_(where, where)], params[0, 2:4] - params[1, 2:4])
    print('error of the bond %.4f px (restatement %.4f), root sum of squares of the positions %.4f px' % (bond, bond_np, rss))
    assert 0 < bond < rss and abs(bond - bond_np) <= 4 * REL_COV * bond_np
    assert np.isnan(ct.fit_error.distance_std(res, params, 0, 0))
