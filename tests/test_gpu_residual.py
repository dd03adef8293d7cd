"""clustertracking_amd.residual on the device against the NumPy restatement (tests/_residual.py) at the
shapes where the kernels can go wrong: frames of 37 x 53 and 5 x 19 x 23 (no multiple of a tile), an
empty frame in the middle and at the end, every dispatched instantiation (four profiles x 2D / 3D x
isotropic / anisotropic) and every pixel type, masks that straddle tiles, lie on the frame's edge, outside
it or nowhere, overlapping rows and clusters, a frame with more rows than two chunks, every option, the
reference's fixtures, grids capped below the work, the byte identities, and the chain from
``refine_arrays`` to ``locate_arrays``.

Tolerances.  Exact: coverage, owner, n_pix, n_own, n_nan, cluster_n_pix, the NaN sets, and every pixel of
an inv_series call and outside the masks (the same operations in the same order, contraction off).
Bounded, for the profiles through exp or sqrt (the device library and NumPy may differ by about one unit
in the last place per call, their argument r2 being bit-equal): per pixel ``|d residual| <= 8 eps (|image|
+ |background| + sum |term|)``, the same for the model; sum_sq, own_sum_sq and cluster_sum_sq within ``(8 +
n_pix) eps`` times the sum of residual**2 (the factor, and n_pix eps for the order of the summation); sum
within 8 eps times the sum of the pixel scales plus n_pix eps sum |residual|; max_abs within 8 eps times the
largest pixel scale; rms and cost, square roots of such a sum, within (8 + n_pix) eps relative.  The factor
is derived, not measured; the largest difference seen is printed in units of the scale.
"""
import importlib

import numpy as np
import pytest

import _residual as R
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib, device

pytestmark = pytest.mark.gpu
residual = importlib.import_module('clustertracking_amd.residual')

EPS = R.EPS
SHAPES = {2: (37, 53), 3: (5, 19, 23)}
DIAMETERS = {(2, True): 9, (2, False): (7, 11), (3, True): 5, (3, False): (3, 7, 5)}
EXTRA = {'gauss': [], 'ring': [0.45], 'disc': [0.5], 'inv_series_2': [1.25, 0.75, 1.5]}
PIXELS = [np.uint8, np.uint16, np.int16, np.int32, np.float32, np.float64]
SEEN = {'pixel': 0., 'sum': 0.}


def make_frames(rng, n_frames, shape, pix):
    pix = np.dtype(pix)
    if pix.kind == 'f':
        return rng.uniform(-20, 200, (n_frames,) + shape).astype(pix)
    lo = -50 if pix.kind == 'i' else 0
    return rng.randint(lo, 200, (n_frames,) + shape).astype(pix)


def make_table(rng, ndim, fit, extra, iso, counts, moved=True, specials=True):
    """params, mask_pos, frame_offset and cluster of a table with ``counts[t]`` random rows in frame t; with
    ``specials`` the first frame with rows also gets the edge cases of the masks"""
    shape, diameter = SHAPES[ndim], DIAMETERS[ndim, iso]
    _, nx, radius, _, n_params = R.model_of(fit, ndim, diameter)
    tile = (8, 32) if ndim == 2 else (2, 8, 16)
    rows, offs = [], [0]
    for t, k in enumerate(counts):
        pos = [rng.uniform(0, np.array(shape) - 1.) for _ in range(k)]
        for j in range(1, k, 3):
            pos[j] = pos[j - 1] + rng.uniform(-1, 1, ndim) * np.array(radius) * 0.8    # overlapping masks
        if specials and k and not rows:
            pos += [np.array(tile, dtype=np.float64),                   # straddles four (2D) or eight (3D) tiles
                    np.array(tile, dtype=np.float64) + 0.4,              # and another row on the same pixels
                    np.array(tile, dtype=np.float64) - 0.3,              # three rows on one pixel
                    np.array([float(tile[0])] + [float(radius[a]) + 2 for a in range(1, ndim)]),   # two tiles
                    np.array([float(s // 2) for s in shape]),            # integer centre: pixels at exactly the radius
                    np.array([-0.5 * radius[0]] + [float(s // 3) for s in shape[1:]]),   # outside, part of it inside
                    np.array([float(s // 3) for s in shape[:-1]] + [shape[-1] - 1. + 0.6 * radius[-1]]),
                    np.array([-(radius[0] + 1.5)] + [3.] * (ndim - 1)),  # more than a radius outside: no pixel
                    np.array([np.nan] + [3.] * (ndim - 1)),              # covers nothing
                    np.array([3.] * (ndim - 1) + [np.inf])]
        rows += pos
        offs.append(len(rows))
    n = len(rows)
    centres = np.array(rows).reshape(n, ndim)
    pos = centres + rng.uniform(-0.5, 0.5, centres.shape) if moved else centres.copy()
    pos[~np.isfinite(pos)] = 3.
    sizes = rng.uniform(0.3, 0.5, (n, 1 if iso else ndim)) * np.array(radius[:1] if iso else radius)
    params = np.concatenate([rng.uniform(0, 20, (n, 1)), rng.uniform(20, 100, (n, 1)), pos, sizes,
                             np.tile(np.array(extra, dtype=np.float64), (n, 1)).reshape(n, len(extra))], axis=1)
    assert params.shape == (n, n_params)
    if not moved:
        params[:, 2:2 + ndim] = centres
    cluster = np.arange(n, dtype=np.int64)
    for t in range(len(counts)):
        for i in range(offs[t] + 1, offs[t + 1]):
            if rng.rand() < 0.6:
                cluster[i] = cluster[i - 1]          # consecutive rows of a frame: the smallest row labels them
    return params, (centres if moved else None), np.array(offs, dtype=np.int64), cluster, diameter


def assert_same(got, want, fit, frames, table, what=''):
    """every output of ``got`` (ndarrays) against the restatement ``want`` by the tolerances of the module;
    table: the frame offsets, the centres and radius of the masks and the cluster labels of the call"""
    for name in ('coverage', 'owner', 'n_pix', 'n_own', 'n_nan', 'cluster_n_pix'):
        g, w = getattr(got, name), getattr(want, name)
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        np.testing.assert_array_equal(g, w, err_msg='%s %s' % (what, name))
    outside = want.coverage == 0
    exact = fit.startswith('inv_series')
    worst = 0.
    for name in ('residual', 'model'):
        g, w = getattr(got, name), getattr(want, name)
        if g is None:
            continue
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg='%s NaN set of %s' % (what, name))
        np.testing.assert_array_equal(g[outside], w[outside], err_msg='%s %s outside' % (what, name))
        if exact:
            np.testing.assert_array_equal(g, w, err_msg='%s %s' % (what, name))
        ok = ~np.isnan(w) & ~outside
        if ok.any():
            ratio = (np.abs(g[ok] - w[ok]) / (EPS * want.scale[ok])).max()
            worst = max(worst, ratio)
            assert ratio <= 8, (what, name, ratio)
    n = np.maximum(want.n_pix, 1).astype(np.float64)
    worst_sum = 0.
    # the scales of a row's sums, from the restatement's maps
    for name, scale in (('sum_sq', want.abs_sq), ('own_sum_sq', want.abs_sq)):
        d = np.abs(getattr(got, name) - getattr(want, name))
        assert (d <= (8 + n) * EPS * scale).all(), (what, name, (d / np.maximum(EPS * scale, 1e-300)).max())
        worst_sum = max(worst_sum, (d / np.maximum((8 + n) * EPS * scale, 1e-300)).max())
    np.testing.assert_array_equal(np.isnan(got.rms), np.isnan(want.rms))
    ok = ~np.isnan(want.rms)
    assert (np.abs(got.rms - want.rms)[ok] <= ((8 + n) * EPS * want.rms)[ok]).all(), (what, 'rms')
    pix_scale, abs_sum = np.zeros(len(n)), np.zeros(len(n))
    max_scale = np.zeros(len(n))
    centres = table
    for i in range(len(n)):
        t = np.searchsorted(centres['offset'], i, side='right') - 1
        box = R.box_of(centres['centres'][i], centres['radius'], frames.shape[1:])
        if box is None:
            continue
        grid = np.meshgrid(*[np.arange(b.start, b.stop, dtype=np.float64) for b in box], indexing='ij', sparse=True)
        m = R.covering(grid, centres['centres'][i], centres['radius'])
        sc, r = want.scale[t][box][m], want.residual[t][box][m]
        pix_scale[i], abs_sum[i] = sc.sum(), np.nansum(np.abs(r))
        max_scale[i] = sc.max() if sc.size else 0.
    assert (np.abs(got.sum - want.sum) <= 8 * EPS * pix_scale + n * EPS * abs_sum).all(), (what, 'sum')
    assert (np.abs(got.max_abs - want.max_abs) <= 8 * EPS * max_scale).all(), (what, 'max_abs')
    if want.cost is not None and got.cost is not None:
        c_scale = np.array([want.abs_sq[table['cluster'] == table['cluster'][i]].sum() for i in range(len(n))])
        c_n = np.maximum(want.cluster_n_pix, 1).astype(np.float64)
        assert (np.abs(got.cluster_sum_sq - want.cluster_sum_sq) <= (8 + c_n) * EPS * c_scale).all(), (what, 'cluster_sum_sq')
        np.testing.assert_array_equal(np.isnan(got.cost), np.isnan(want.cost))
        ok = ~np.isnan(want.cost)
        assert (np.abs(got.cost - want.cost)[ok] <= ((8 + c_n) * EPS * np.abs(want.cost))[ok]).all(), (what, 'cost')
    SEEN['pixel'], SEEN['sum'] = max(SEEN['pixel'], worst), max(SEEN['sum'], worst_sum)
    print('%s: largest pixel difference %.3f eps scale (bound 8), largest sum_sq difference %.4f of its bound'
          % (what, worst, worst_sum))


def run(frames, params, offs, diameter, fit, mask_pos, cluster, what='', **kw):
    """the device and the restatement on the same table; asserts they agree; returns both"""
    ndim = frames.ndim - 1
    got = ct.residual_arrays(frames, params, offs, diameter, fit, mask_pos, cluster, want_model=True, **kw)
    want = R.residual_np(frames, params, offs, diameter, fit, mask_pos, cluster, kw.get('outside', 'zero'))
    table = dict(offset=np.asarray(offs), centres=params[:, 2:2 + ndim] if mask_pos is None else mask_pos,
                 radius=R.model_of(fit, ndim, diameter)[2], cluster=np.arange(len(params)) if cluster is None else np.asarray(cluster))
    assert got.status.tolist() == [_abi.RESID_OK]
    assert_same(got, want, fit, frames, table, what)
    return got, want


# ---- every dispatched instantiation, every pixel type --------------------------------------------------
INST = [(fit, ndim, iso) for fit in EXTRA for ndim in (2, 3) for iso in (True, False)]


@pytest.mark.parametrize('fit,ndim,iso', INST, ids=['%s-%dd-%s' % (f, d, 'iso' if i else 'aniso') for f, d, i in INST])
def test_every_instantiation_against_restatement(fit, ndim, iso, engine):
    k = INST.index((fit, ndim, iso))
    rng = np.random.RandomState(100 + k)
    pix = PIXELS[k % len(PIXELS)]                                   # each of the six at least twice over the 16
    frames = make_frames(rng, 4, SHAPES[ndim], pix)
    params, mask_pos, offs, cluster, diameter = make_table(rng, ndim, fit, EXTRA[fit], iso, [9, 0, 7, 0])
    got, want = run(frames, params, offs, diameter, fit, mask_pos, cluster, what='%s %dd %s %s' % (fit, ndim, iso, np.dtype(pix)))
    # the edge cases are in the table: rows without a pixel, clipped rows, three rows on a pixel, two clusters on one
    assert (want.n_pix == 0).sum() >= 3 and np.isnan(got.rms[want.n_pix == 0]).all() and want.coverage.max() >= 3
    assert (want.coverage[1] == 0).all() and (want.coverage[3] == 0).all()
    multi = want.coverage >= 2
    assert multi.any() and (got.owner[multi] >= 0).all()
    labels = np.asarray(cluster)
    assert any(labels[a] != labels[b] for a in range(len(labels)) for b in range(a)
               if ((want.owner == b) & multi).any() and want.n_pix[a] > want.n_own[a] and a < offs[1] and b < offs[1])


@pytest.mark.parametrize('pix', PIXELS, ids=[np.dtype(p).name for p in PIXELS])
def test_every_pixel_type(pix, engine):
    rng = np.random.RandomState(7)
    frames = make_frames(rng, 4, SHAPES[2], pix)
    params, mask_pos, offs, cluster, diameter = make_table(rng, 2, 'gauss', [], True, [6, 0, 5, 0])
    run(frames, params, offs, diameter, 'gauss', mask_pos, cluster, what=np.dtype(pix).name)


def test_disc_on_all_branches_and_nan_pixels(engine):
    rng = np.random.RandomState(11)
    frames = make_frames(rng, 4, SHAPES[2], np.float64)
    frames[0, 5, 7] = np.nan                                          # a NaN pixel of the image
    for e in (0., 0.5, 1.5):
        params, mask_pos, offs, cluster, diameter = make_table(rng, 2, 'disc', [e], True, [8, 0, 6, 0])
        params[0, 2:4] = mask_pos[0] = (5.2, 7.3)
        got, want = run(frames, params, offs, diameter, 'disc', mask_pos, cluster, what='disc %g' % e)
        assert want.n_nan.sum() > 0 and np.isnan(got.cost).any()      # the frame maximum is NaN there


def test_integer_centre_covers_the_pixels_at_exactly_the_radius(engine):
    frames = np.full((1,) + SHAPES[2], 10, dtype=np.uint8)
    params = np.array([[2., 50., 18., 26., 1.5]])
    got, want = run(frames, params, [0, 1], 9, 'gauss', None, np.zeros(1, dtype=np.int64), what='by hand')
    assert got.coverage[0, 14, 26] == got.coverage[0, 22, 26] == got.coverage[0, 18, 22] == got.coverage[0, 18, 30] == 1
    assert got.coverage[0, 13, 26] == 0 and got.n_pix[0] == 49 and got.residual[0, 18, 26] == 10. - 2. - 50.


# ---- empty tables ----------------------------------------------------------------------------------------
def test_no_rows_and_no_frames(engine):
    frames = make_frames(np.random.RandomState(3), 2, SHAPES[2], np.uint8)
    for outside in ('zero', 'nan', 'image'):
        got = ct.residual_arrays(frames, np.zeros((0, 5)), [0, 0, 0], 9, outside=outside, want_model=True,
                                 cluster=np.zeros(0, dtype=np.int64))
        want = R.residual_np(frames, np.zeros((0, 5)), [0, 0, 0], 9, outside=outside)
        np.testing.assert_array_equal(got.residual, want.residual)
        np.testing.assert_array_equal(got.model, want.model)
        assert (got.owner == -1).all() and (got.coverage == 0).all() and got.n_pix.shape == (0,) and got.cost.shape == (0,)
    got = ct.residual_arrays(frames[:0], np.zeros((0, 5)), [0], 9, want_model=True)
    assert got.residual.shape == (0,) + SHAPES[2] and got.rms.shape == (0,) and got.cost is None
    got = ct.residual_arrays(np.zeros((0,) + SHAPES[3], dtype=np.float32), np.zeros((0, 8)), [0], (3, 7, 5), want_frames=False)
    assert got.residual is None and got.owner is None and got.n_pix.shape == (0,)


# ---- chunks ------------------------------------------------------------------------------------------------
def test_more_rows_than_two_chunks_in_one_tile(engine):
    """one frame of 24 x 24 with 2 * 256 + 1 rows whose masks all meet the first tile: three chunks, the
    owner from the first, the terms in row order across them"""
    rng = np.random.RandomState(5)
    n = 2 * _abi.RESID_CHUNK + 1
    frames = make_frames(rng, 1, (24, 24), np.uint16)
    centres = np.stack([rng.uniform(3., 4.5, n), rng.uniform(3., 20., n)], axis=1)
    params = np.concatenate([rng.uniform(0, 20, (n, 1)), rng.uniform(1, 3, (n, 1)), centres, rng.uniform(0.8, 1.2, (n, 1))], axis=1)
    cluster = (np.arange(n) // 3 * 3).astype(np.int64)
    got, want = run(frames, params, [0, n], 5, 'gauss', None, cluster, what='chunks')
    assert want.coverage[0, :8].max() > _abi.RESID_CHUNK / 8 and (want.coverage[0, 8:] == 0).all()
    late = want.owner[0] >= _abi.RESID_CHUNK                      # pixels whose first row comes in a later chunk
    assert want.coverage.max() > 40 and (got.owner[0][late] == want.owner[0][late]).all()


# ---- options -----------------------------------------------------------------------------------------------
def test_options(engine):
    rng = np.random.RandomState(13)
    frames = make_frames(rng, 4, SHAPES[3], np.int16)
    params, mask_pos, offs, cluster, diameter = make_table(rng, 3, 'ring', [0.45], False, [6, 0, 5, 0])
    full = {}
    for outside in ('zero', 'nan', 'image'):
        full[outside], _ = run(frames, params, offs, diameter, 'ring', mask_pos, cluster, what='outside ' + outside, outside=outside)
    stats = [f for f in residual.Residual._fields if f not in ('residual', 'model', 'coverage', 'owner')]
    for want_model in (False, True):
        for want_frames in (False, True):
            got = ct.residual_arrays(frames, params, offs, diameter, 'ring', mask_pos, cluster, want_model=want_model,
                                     want_frames=want_frames)
            assert (got.model is None) == (not want_model) and (got.residual is None) == (not want_frames)
            assert (got.coverage is None) == (got.owner is None) == (not want_frames)
            for f in stats:
                assert getattr(got, f).tobytes() == getattr(full['zero'], f).tobytes(), f
            if want_model:
                assert got.model.tobytes() == full['zero'].model.tobytes()
    none = ct.residual_arrays(frames, params, offs, diameter, 'ring')       # the positions are the centres, no cluster
    assert none.cost is None and none.cluster_n_pix is None and none.cluster_sum_sq is None
    want = R.residual_np(frames, params, offs, diameter, 'ring')
    np.testing.assert_array_equal(none.coverage, want.coverage)
    np.testing.assert_array_equal(none.n_own, want.n_own)


def test_refused_tables(engine):
    import torch
    dev = torch.device('cuda', 0)
    frames = torch.zeros((2, 16, 16), dtype=torch.uint8, device=dev)
    params = torch.tensor([[0., 1., 5., 5., 2.]] * 3, dtype=torch.float64, device=dev)
    bad = ct.residual_arrays(frames, params, torch.tensor([0, 3, 2], device=dev), 7)
    assert bad.status.tolist() == [_abi.RESID_BAD_TABLE]
    bad = ct.residual_arrays(frames, params, torch.tensor([0, 2, 3], device=dev), 7, cluster=torch.tensor([0, 0, 1], device=dev))
    assert bad.status.tolist() == [_abi.RESID_BAD_CLUSTER] and bad.n_pix.tolist() == [29, 29, 29]
    assert torch.isnan(bad.cost[2]) and not torch.isnan(bad.cost[:2]).any()
    with pytest.raises(ValueError, match='smallest row'):
        ct.residual_arrays(frames.cpu().numpy(), params.cpu().numpy(), [0, 2, 3], 7, cluster=[0, 1, 2][::-1])
    with pytest.raises(ValueError, match='float64'):
        ct.residual_arrays(frames, params.float(), torch.tensor([0, 2, 3], device=dev), 7)


# ---- the reference's fixtures ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.fixtures(), ids=[c.name for c in R.fixtures()])
def test_reference_fixture_on_the_device(case, engine):
    n = len(case.params)
    cluster = np.zeros(n, dtype=np.int64)
    got, want = run(case.frame[None], case.params, [0, n], case.diameter, case.fit, case.centres, cluster, what=case.name)
    assert got.cluster_n_pix[0] == case.n_pix
    value = got.cluster_sum_sq[0] / got.cluster_n_pix[0]
    assert abs(value - case.value) <= 1e-12 * case.value, (value, case.value)


# ---- grids capped below the work ----------------------------------------------------------------------
def test_every_grid_stride_loop_takes_a_second_trip(engine):
    rng = np.random.RandomState(17)
    frames = make_frames(rng, 4, SHAPES[2], np.uint8)
    params, mask_pos, offs, cluster, diameter = make_table(rng, 2, 'gauss', [], True, [9, 0, 7, 0])
    free = ct.residual_arrays(frames, params, offs, diameter, 'gauss', mask_pos, cluster, want_model=True)
    cap = 2
    plan = _lib.residual_plan(residual.descriptor(SHAPES[2], np.uint8, 4, len(params), diameter, has_cluster=True, max_grid=cap))
    assert plan.grids[1] == cap < plan.n_tiles and plan.grids[2] * 4 < len(params) and plan.grids[3] == cap < 4
    capped = ct.residual_arrays(frames, params, offs, diameter, 'gauss', mask_pos, cluster, want_model=True, _max_grid=cap)
    with engine.stage_max_grid(1):
        one = ct.residual_arrays(frames, params, offs, diameter, 'gauss', mask_pos, cluster, want_model=True)
    for f in residual.Residual._fields:
        assert getattr(capped, f).tobytes() == getattr(free, f).tobytes() == getattr(one, f).tobytes(), f
    # the check kernel: more offsets than one workgroup of 256 reads in a trip
    n_frames = 300
    small = make_frames(rng, n_frames, (8, 8), np.uint8)
    offs = np.arange(n_frames + 1, dtype=np.int64)
    par = np.concatenate([np.zeros((n_frames, 1)), np.ones((n_frames, 1)), rng.uniform(2, 5, (n_frames, 2)), np.full((n_frames, 1), 1.5)], axis=1)
    assert _lib.residual_plan(residual.descriptor((8, 8), np.uint8, n_frames, n_frames, 5, max_grid=1)).grids[0] == 1
    got = ct.residual_arrays(small, par, offs, 5, _max_grid=1)
    want = R.residual_np(small, par, offs, 5)
    np.testing.assert_array_equal(got.owner, want.owner)
    import torch
    bad = torch.from_numpy(offs).cuda()
    bad[290] = 295                                                   # falls afterwards: found on the second trip
    res = ct.residual_arrays(torch.from_numpy(small).cuda(), torch.from_numpy(par).cuda(), bad, 5, _max_grid=1)
    assert res.status.tolist() == [_abi.RESID_BAD_TABLE]


# ---- the same bytes ---------------------------------------------------------------------------------------
def test_same_bytes_again_alone_and_on_another_stream(engine):
    import torch
    rng = np.random.RandomState(19)
    frames = make_frames(rng, 4, SHAPES[3], np.float32)
    params, mask_pos, offs, cluster, diameter = make_table(rng, 3, 'disc', [0.5], True, [8, 0, 7, 0])
    call = lambda *a, **k: ct.residual_arrays(*a, want_model=True, **k)
    first = call(frames, params, offs, diameter, 'disc', mask_pos, cluster)
    again = call(frames, params, offs, diameter, 'disc', mask_pos, cluster)
    for f in residual.Residual._fields:
        assert getattr(first, f).tobytes() == getattr(again, f).tobytes(), f
    # frame 2 alone: its rows renumbered from 0
    a, b = int(offs[2]), int(offs[3])
    alone = call(frames[2:3], params[a:b], [0, b - a], diameter, 'disc', mask_pos[a:b], cluster[a:b] - a)
    for f in ('residual', 'model', 'coverage'):
        assert getattr(alone, f)[0].tobytes() == getattr(first, f)[2].tobytes(), f
    np.testing.assert_array_equal(np.where(alone.owner[0] >= 0, alone.owner[0] + a, -1), first.owner[2])
    for f in residual.Residual._fields[4:-1]:
        assert getattr(alone, f).tobytes() == getattr(first, f)[a:b].tobytes(), f
    dev = torch.device('cuda', 0)
    tens = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (frames, params, offs, mask_pos, cluster)]
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        other = call(tens[0], tens[1], tens[2], diameter, 'disc', tens[3], tens[4])
    stream.synchronize()
    assert isinstance(other.residual, torch.Tensor) and other.residual.device == dev
    for f in residual.Residual._fields:
        assert getattr(other, f).cpu().numpy().tobytes() == getattr(first, f).tobytes(), f


# ---- the chain ----------------------------------------------------------------------------------------------
def chain_layout():
    """12 dimers in each of two frames of 64 x 96, their features 5 px apart (one cluster at separation 9,
    diameter 9), the clusters 20 px apart: generic positions, so that no mask pixel lies near its edge"""
    rng = np.random.RandomState(23)
    pos, frame_of = [], []
    for t in range(2):
        for cy in (12., 32., 52.):
            for cx in (14., 36., 58., 80.):
                c = np.array([cy, cx]) + rng.uniform(-1.5, 1.5, 2)
                ang = rng.uniform(0, np.pi)
                d = 2.5 * np.array([np.sin(ang), np.cos(ang)])
                pos += [c - d, c + d]
                frame_of += [t, t]
    return np.array(pos), np.array(frame_of), (64, 96)


def cost_bound(want, rows, t):
    """The relative bound on the difference of two costs of the cluster of ``rows`` in frame t that were
    computed from the same pixels by different kernels: cost goes with the root of S = sum r**2, so d cost /
    cost = dS / 2S, and dS <= 2 sum |r| 8 eps scale from the pixel bound of the module, plus n eps S for the
    order of the summation."""
    m = np.isin(want.owner[t], rows)
    r, sc = want.residual[t][m], want.scale[t][m]
    return 8 * EPS * (np.abs(r) * sc).sum() / (r * r).sum() + m.sum() * EPS


def test_chain_refine_then_residual(engine):
    pos, frame_of, shape = chain_layout()
    n = len(pos)
    frames = device.draw_frames(shape, frame_of, pos, 2., 200, n_frames=2, noise=0., dtype=np.uint8)
    offs = np.array([0, n // 2, n], dtype=np.int64)
    res = ct.refine_arrays(frames.cpu().numpy(), pos, offs, 9, signal=200., size=2.)
    assert (res.cluster_size == 2).all() and not np.isnan(res.cost).any()
    out = ct.residual_arrays(frames.cpu().numpy(), res.params, offs, 9, cluster=res.cluster)
    start = R.residual_np(frames.cpu().numpy(), np.concatenate([res.params[:, :2], pos, res.params[:, 4:]], axis=1), offs, 9)
    fitted = R.residual_np(frames.cpu().numpy(), res.params, offs, 9)
    rounds = np.repeat(res.n_rounds, np.diff(res.feat_offset))       # per row in batch order = row order here (clusters of consecutive rows)
    same = np.array([(start.coverage == fitted.coverage)[t][tuple(R.box_of(pos[i], (5, 5), shape))].all()
                     for i, t in enumerate(frame_of)])
    roots = np.unique(res.cluster)
    ok = np.array([same[res.cluster == c].all() and (rounds[res.cluster == c] == 1).all() for c in roots])
    print('clusters whose mask did not move: %d of %d' % (ok.sum(), len(roots)))
    assert 2 * ok.sum() >= len(roots)
    for c in roots[ok]:
        assert abs(out.cost[c] - res.cost[c]) <= cost_bound(fitted, np.flatnonzero(res.cluster == c), frame_of[c]) * res.cost[c], \
            (c, out.cost[c], res.cost[c])
    # with the start positions as the centres of the masks every cluster of one round qualifies
    at_start = ct.residual_arrays(frames.cpu().numpy(), res.params, offs, 9, mask_pos=pos, cluster=res.cluster)
    want = R.residual_np(frames.cpu().numpy(), res.params, offs, 9, mask_pos=pos)
    one = np.array([(rounds[res.cluster == c] == 1).all() for c in roots])
    assert 2 * one.sum() >= len(roots)
    for c in roots[one]:
        assert abs(at_start.cost[c] - res.cost[c]) <= cost_bound(want, np.flatnonzero(res.cluster == c), frame_of[c]) * res.cost[c], \
            (c, at_start.cost[c], res.cost[c])


def test_use_case_missed_feature_is_the_residual_blob(engine):
    import torch
    pos = np.array([[20.3, 20.6], [20.3 + 3.6, 20.6 + 4.8]])          # 6 px apart
    frames = device.draw_frames((48, 48), [0, 0], pos, 2., 180, n_frames=1, noise=0., dtype=np.uint8)
    params = torch.tensor([[0., 180., pos[0, 0], pos[0, 1], 2.]], dtype=torch.float64, device=frames.device)
    offs = torch.tensor([0, 1], device=frames.device)
    out = ct.residual_arrays(frames, params, offs, 17)
    assert isinstance(out.residual, torch.Tensor) and out.residual.dtype == torch.float64
    r = out.residual[0].cpu().numpy()
    mask = out.coverage[0].cpu().numpy() == 1
    at = np.unravel_index(np.argmax(np.where(mask, r, -np.inf)), r.shape)
    assert at == tuple(np.round(pos[1]).astype(int)) and mask[at]
    found, off, _ = ct.find.locate_arrays(out.residual, 5)
    assert off.tolist()[0] == 0 and any((p == np.round(pos[1])).all() for p in found)


def test_table_form(engine):
    pd = pytest.importorskip('pandas')
    rng = np.random.RandomState(29)
    frames = make_frames(rng, 3, SHAPES[2], np.uint8)
    params, _, offs, cluster, diameter = make_table(rng, 2, 'gauss', [], True, [5, 0, 4], moved=False, specials=False)
    f = pd.DataFrame(params, columns=['background', 'signal', 'y', 'x', 'size'])
    f['frame'] = np.repeat([0, 2], [5, 4])
    f['cluster'] = cluster + 100
    f = f.iloc[[5, 0, 6, 1, 2, 7, 3, 8, 4]]                           # the frames interleaved; the rows of a frame keep their order
    want = R.residual_np(frames[[0, 2]], params, [0, 5, 9], diameter, 'gauss', cluster=cluster)
    got, block = ct.residual(f, ct.ArrayReader(frames), diameter, cluster_column='cluster', return_frames=True)
    assert list(got.index) == list(f.index)
    got = got.sort_index()
    assert list(got.columns[-5:]) == ['res_rms', 'res_max', 'res_n', 'res_nan', 'res_cost'] and block.shape == (2,) + SHAPES[2]
    np.testing.assert_array_equal(got['res_n'].values, want.n_pix)
    np.testing.assert_allclose(got['res_rms'].values, want.rms, rtol=200 * EPS)
    np.testing.assert_allclose(got['res_cost'].values, want.cost, rtol=400 * EPS)
    np.testing.assert_allclose(block, want.residual, rtol=0, atol=8 * EPS * want.scale.max())
    plain = ct.residual(f, ct.ArrayReader(frames), diameter)
    assert 'res_cost' not in plain and list(plain.index) == list(f.index)
