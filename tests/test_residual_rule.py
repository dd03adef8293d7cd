"""clustertracking_amd.residual without a GPU: the NumPy restatement of its rule (tests/_residual.py)
against hand-computed pixels, against every case of tests/golden/residual/residual_reference.npz (the
reference's ``prepare_subimage`` and ``FitFunctions.get_residual(..., norm=1.)``) and, where the reference
is present, against a fresh run of it on random clusters of every profile; the argument refusals, raised
before the engine is touched; the entry points declared, exported and mirrored; ``ctr_residual_plan``
equal to its restatement at its edges.

Tolerances: ``cluster_n_pix`` exact; ``cluster_sum_sq / cluster_n_pix`` to rtol 1e-12 of the reference's
value (both are float64 sums of a few hundred squares in different orders: n eps ~ 1e-13 at the most).
"""
import ctypes
import importlib
import os
import re
import sys
import warnings
import zlib

import numpy as np
import pytest

import _cases
import _residual as R
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib

sys.path.insert(0, os.path.join(_cases.ROOT, 'oracle'))
import refshim  # noqa: E402

residual = importlib.import_module('clustertracking_amd.residual')    # ct.residual is the function
FIXTURES = R.fixtures()


def _cluster_value(frame, params, centres, diameter, fit):
    n = len(params)
    out = R.residual_np(frame[None], params, [0, n], diameter, fit, mask_pos=centres, cluster=np.zeros(n, dtype=np.int64))
    assert (out.cluster_n_pix == out.cluster_n_pix[0]).all() and (out.cluster_sum_sq == out.cluster_sum_sq[0]).all()
    assert out.cluster_n_pix[0] == (out.coverage > 0).sum() == out.n_own.sum()
    return out.cluster_sum_sq[0] / out.cluster_n_pix[0], int(out.cluster_n_pix[0]), out


# ---- the rule on pixels counted by hand -------------------------------------------------------------
def test_one_gaussian_by_hand():
    frame = np.full((1, 7, 9), 10, dtype=np.uint8)
    frame[0, 3, 4] = 60
    params = np.array([[2., 50., 3., 4., 1.5]])                  # background, signal, y, x, size
    out = R.residual_np(frame, params, [0, 1], 5, 'gauss', cluster=[0])
    # radius 2 around an integer centre: the 13 pixels with dy^2 + dx^2 <= 4, the four at exactly the radius included
    assert out.n_pix[0] == out.n_own[0] == 13 and out.coverage.sum() == 13 and out.n_nan[0] == 0
    assert out.coverage[0, 1, 4] == out.coverage[0, 5, 4] == out.coverage[0, 3, 2] == out.coverage[0, 3, 6] == 1
    assert out.coverage[0, 1, 3] == 0 and out.owner[0, 1, 3] == -1 and out.owner[0, 3, 4] == 0
    assert out.residual[0, 3, 4] == 60. - 2. - 50. and out.model[0, 3, 4] == 52.
    g = np.exp(-0.5 * 2 * (1. / 2.25))
    assert out.residual[0, 3, 5] == (10. - 2.) - 50. * g and out.model[0, 3, 5] == 2. + 50. * g
    assert out.residual[0, 0, 0] == 0. and out.model[0, 0, 0] == 0.
    assert out.max_abs[0] == np.abs(out.residual).max() and out.cost[0] == out.rms[0] / 60.
    assert abs(out.sum_sq[0] - (out.residual ** 2).sum()) <= 13 * R.EPS * out.sum_sq[0]


def test_overlap_follows_the_lowest_row_and_outside_values():
    frame = np.arange(7 * 12, dtype=np.float32).reshape(1, 7, 12)
    params = np.array([[1., 20., 3., 4., 1.2], [5., 30., 3., 6., 1.2], [9., 40., 3.5, 5., 1.2]])
    z = R.residual_np(frame, params, [0, 3], 5, 'gauss', cluster=[0, 0, 2], outside='zero')
    assert z.coverage[0, 3, 5] == 3 and z.owner[0, 3, 5] == 0 and z.owner[0, 3, 8] == 1 and z.owner[0, 5, 5] == 2
    t = [p[1] * np.exp(-0.5 * 2 * (((3 - p[2]) ** 2) * (1. / (p[4] * p[4])) + ((5 - p[3]) ** 2) * (1. / (p[4] * p[4])))) for p in params]
    assert z.residual[0, 3, 5] == ((frame[0, 3, 5] - 1.) - t[0]) - t[1] - t[2]
    assert z.model[0, 3, 5] == 1. + ((0. + t[0]) + t[1] + t[2])
    assert z.n_own.sum() == (z.coverage > 0).sum() and z.n_pix.sum() == z.coverage.sum()
    assert list(z.cluster_n_pix) == [z.n_own[0] + z.n_own[1]] * 2 + [z.n_own[2]]
    assert z.cluster_sum_sq[0] == z.cluster_sum_sq[1] == z.own_sum_sq[0] + z.own_sum_sq[1]
    nan = R.residual_np(frame, params, [0, 3], 5, 'gauss', outside='nan')
    img = R.residual_np(frame, params, [0, 3], 5, 'gauss', outside='image')
    out = z.coverage == 0
    assert np.isnan(nan.residual[out]).all() and np.isnan(nan.model[out]).all() and not np.isnan(nan.residual[~out]).any()
    assert (img.residual[out] == frame[out]).all() and (img.model[out] == 0.).all()
    assert (img.residual[~out] == z.residual[~out]).all() and img.cluster_n_pix is None


def test_centres_outside_the_frame_and_not_finite():
    frame = np.ones((1, 8, 8), dtype=np.int16)
    params = np.array([[0., 1., -1.5, 3., 1.], [0., 1., -4., 3., 1.], [0., 1., np.nan, 3., 1.], [0., 1., 3., np.inf, 1.]])
    out = R.residual_np(frame, params, [0, 4], 7, 'gauss')
    assert out.n_pix[0] == 8 and list(out.n_pix[1:]) == [0, 0, 0]       # 5 pixels of row 0 and 3 of row 1 of the frame
    assert np.isnan(out.rms[1:]).all() and (out.sum_sq[1:] == 0).all() and out.rms[0] == out.rms[0]


def test_ring_and_disc_within_one_pixel_of_the_centre():
    frame = np.full((1, 9, 9), 7, dtype=np.uint16)
    ring = R.residual_np(frame, np.array([[1., 5., 4.2, 4.1, 2., 0.5]]), [0, 1], 7, 'ring')
    near = (np.arange(9)[:, None] - 4.2) ** 2 + (np.arange(9)[None] - 4.1) ** 2 < 1.
    assert ring.n_nan[0] == near.sum() == 3 and (np.isnan(ring.residual[0]) == near).all() and ring.n_pix[0] > 20
    assert abs(ring.rms[0] - np.sqrt(np.nansum(ring.residual ** 2) / ring.n_pix[0])) <= 27 * R.EPS * ring.rms[0]   # the order of the sum
    disc = R.residual_np(frame, np.array([[1., 5., 4.2, 4.1, 2., 0.5]]), [0, 1], 7, 'disc')
    assert disc.n_nan[0] == 0 and (disc.residual[0][near] == 7. - 1. - 5.).all()
    disc0 = R.residual_np(frame, np.array([[1., 5., 4.2, 4.1, 2., 0.]]), [0, 1], 7, 'disc')
    assert (np.isnan(disc0.residual[0]) == near).all()


# ---- the reference -----------------------------------------------------------------------------------
def test_fixture_covers_what_it_should():
    fits = {c.fit for c in FIXTURES}
    assert fits == {'gauss', 'ring', 'disc', 'inv_series_2'} and 12 <= len(FIXTURES) <= 16
    assert {c.frame.ndim for c in FIXTURES} == {2, 3} and {len(c.params) for c in FIXTURES} == {2, 3, 4}
    assert all(c.frame.shape in ((32, 32), (12, 24, 24)) for c in FIXTURES) and os.path.getsize(R.GOLDEN) < 200 * 1024
    discs = sorted(c.params[0, -1] for c in FIXTURES if c.fit == 'disc')
    assert discs[0] == 0. and 0. < discs[1] < 1. and discs[2] >= 1.
    assert any(len(set(c.diameter)) > 1 for c in FIXTURES) and any(len(set(c.diameter)) == 1 for c in FIXTURES)


@pytest.mark.parametrize('case', FIXTURES, ids=[c.name for c in FIXTURES])
def test_restatement_reproduces_the_fixture(case):
    value, n_pix, out = _cluster_value(case.frame, case.params, case.centres, case.diameter, case.fit)
    print(case.name, 'n_pix', n_pix, 'value', value, 'reference', case.value, 'relative', abs(value - case.value) / case.value)
    assert n_pix == case.n_pix
    assert abs(value - case.value) <= 1e-12 * case.value
    if case.name == 'gauss_2d_edge':
        assert (out.n_pix < 81).all()              # clipped: a whole mask of radius 5 has 81 pixels
    if case.name == 'ring_2d_near_pixel':
        assert out.n_nan.sum() > 0


LIVE = [(fit, extra, shape, diameter) for fit, extra in R.PROFILES
        for shape, diameter in (((32, 32), 9), ((30, 34), (7, 11)), ((12, 24, 24), 7), ((12, 24, 24), (5, 9, 7)))]


@pytest.mark.skipif(not refshim.available(), reason='the reference is not present')
@pytest.mark.parametrize('fit,extra,shape,diameter', LIVE, ids=['%s%s-%dd-%s' % (f, ''.join('_%g' % v for v in e[:1]), len(s), 'iso' if np.isscalar(d) else 'aniso') for f, e, s, d in LIVE])
def test_restatement_reproduces_the_live_reference(fit, extra, shape, diameter):
    refshim.load()
    from clustertracking import refine as ref_refine
    from clustertracking.fitfunc import FitFunctions, vect_from_params
    ndim = len(shape)
    _, _, radius, isotropic, _ = R.model_of(fit, ndim, diameter)
    rng = np.random.RandomState(zlib.crc32(repr((fit, extra, shape, diameter)).encode()))
    for n in (2, 3, 4):
        frame, params, centres = R.random_cluster(rng, fit, extra, shape, diameter, n)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sub, mesh, masks = ref_refine.prepare_subimage(centres, frame, radius)
            ff = FitFunctions(fit, ndim, isotropic)
            fun, _ = ff.get_residual([sub], [mesh], [masks], params, None, 1.)
            want = float(fun(vect_from_params(params, ff.modes, None, operation=np.mean)))
        value, n_pix, _ = _cluster_value(frame, params, centres, diameter, fit)
        assert n_pix == len(sub)
        assert abs(value - want) <= 1e-12 * want, (n, value, want)


# ---- refusals before any device work -----------------------------------------------------------------
def test_argument_refusals_need_no_engine(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError('the engine was looked up before the arguments were checked')
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    frames = np.zeros((2, 16, 16), dtype=np.uint8)
    params = np.zeros((3, 5))
    off = [0, 2, 3]
    call = lambda *a, **k: ct.residual_arrays(*a, **k)
    with pytest.raises(NotImplementedError):
        call(frames, params, off, 7, fit_function=dict(name='mine', params=[], func=None))
    for bad in ('lorentz', 'inv_series', 'inv_series_x'):
        with pytest.raises(ValueError, match='Unknown fit function'):
            call(frames, params, off, 7, fit_function=bad)
    with pytest.raises(ValueError, match='CTR_MAX_PARAMS'):
        call(frames, np.zeros((3, 15)), off, 7, fit_function='inv_series_9')
    with pytest.raises(ValueError, match='CTR_MAX_PARAMS'):
        call(np.zeros((2, 4, 16, 16)), np.zeros((3, 14)), off, (5, 7, 7), fit_function='inv_series_5')
    with pytest.raises(ValueError, match='params must be'):
        call(frames, np.zeros((3, 6)), off, 7)
    with pytest.raises(ValueError, match='params must be'):
        call(frames, np.zeros((3, 5)), off, (7, 9))               # anisotropic: two size columns
    with pytest.raises(ValueError, match='ndim 2 or 3'):
        call(np.zeros((2, 16)), params, off, 7)
    with pytest.raises(ValueError, match='frame_offset'):
        call(frames, params, [0, 3], 7)
    with pytest.raises(ValueError, match='frame_offset'):
        call(frames, params, [0, 3, 2], 7)
    with pytest.raises(ValueError, match='frame_offset'):
        call(frames, params, [1, 2, 3], 7)
    with pytest.raises(ValueError, match='mask_pos'):
        call(frames, params, off, 7, mask_pos=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='mask_pos'):
        call(frames, params, off, 7, mask_pos=np.zeros((3, 3)))
    with pytest.raises(ValueError, match='cluster'):
        call(frames, params, off, 7, cluster=np.zeros(2, dtype=np.int64))
    with pytest.raises(ValueError, match='cluster'):
        call(frames, params, off, 7, cluster=np.zeros(3))
    for bad in ('edge', None, 0):
        with pytest.raises(ValueError, match='outside'):
            call(frames, params, off, 7, outside=bad)
    with pytest.raises(ValueError, match='diameter'):
        call(frames, params, off, 1)


def test_table_form_refusals(monkeypatch):
    pd = pytest.importorskip('pandas')
    monkeypatch.setattr(_lib, 'default_engine', lambda *a, **k: (_ for _ in ()).throw(AssertionError('engine')))
    f = pd.DataFrame(dict(y=[4., 5.], x=[4., 9.], signal=[10., 10.], frame=[0, 0]))
    reader = ct.ArrayReader(np.zeros((1, 16, 16), dtype=np.uint8))
    with pytest.raises(ValueError, match="no 'size' column"):
        ct.residual(f, reader, 7)
    with pytest.raises(NotImplementedError):
        ct.residual(f, reader, 7, fit_function=dict())
    with pytest.raises(ValueError, match='outside'):
        ct.residual(f.assign(size=2.), reader, 7, outside='frame')


# ---- declared, exported, mirrored --------------------------------------------------------------------
def test_declared_and_exported():
    assert {'residual', 'residual_arrays'} <= set(ct.__all__) and ct.residual is residual.residual
    assert ct.residual_arrays is residual.residual_arrays
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    body = re.search(r'typedef struct ctr_residual \{(.*?)\} ctr_residual;', header, re.S).group(1)
    fields = re.findall(r'(\w+)(?:\[\w+\])?;', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    assert fields == [name for name, _ in _abi.Residual._fields_]
    assert 'ctr_residual_device' in _lib.SIGNATURES and 'ctr_residual_plan' in _lib.SIGNATURES
    assert int(re.search(r'#define CTR_RESID_CHUNK (\d+)', header).group(1)) == _abi.RESID_CHUNK
    assert residual.Residual._fields == R.Residual._fields[:-2] + ('status',)
    lib = _lib.load()
    assert lib.ctr_residual_device(None, None, None) == _abi.ERR_INVALID
    d = residual.descriptor((16, 16), np.uint8, 1, 0, 7)
    assert lib.ctr_residual_device(None, ctypes.byref(d), None) == _abi.ERR_INVALID
    assert (lib.ctr_last_error(None) or b'').decode() == 'ctr_residual_device: null frame_offset or status'


# ---- the launch decision -----------------------------------------------------------------------------
PLANS = [
    ('no rows', (37, 53), 4, 0, True, False, 0),
    ('no frames', (37, 53), 0, 0, True, True, 0),
    ('one tile', (8, 32), 1, 3, True, True, 0),
    ('one pixel more than a tile', (9, 33), 1, 3, False, True, 0),
    ('no multiple of the tile', (37, 53), 4, 10, False, False, 0),
    ('3D, no multiple of the tile', (5, 19, 23), 4, 10, True, True, 0),
    ('one row more than a chunk', (24, 24), 1, _abi.RESID_CHUNK + 1, True, True, 0),
    ('lowered cap', (37, 53), 4, 40, False, True, 3),
    ('the cap of a handle', (512, 512), 256, 51200, False, True, 0),
    ('more features than the cap', (64, 64), 2, 4 * 65536 + 1, True, False, 0),
]


@pytest.mark.parametrize('what,shape,n_frames,n_features,want_frames,has_cluster,max_grid', PLANS, ids=[p[0] for p in PLANS])
def test_plan_at_its_edges(what, shape, n_frames, n_features, want_frames, has_cluster, max_grid):
    d = residual.descriptor(shape, np.float32, n_frames, n_features, 9 if len(shape) == 2 else (5, 9, 9), 'gauss',
                            want_frames=want_frames, has_cluster=has_cluster, max_grid=max_grid)
    plan = _lib.residual_plan(d)
    tile, chunk, n_tiles, grids, scratch = R.plan_np(shape, n_frames, n_features, want_frames, has_cluster, max_grid or 65536)
    assert plan.tile == tile and plan.chunk == chunk == 256 and plan.n_tiles == n_tiles
    assert plan.grids == grids and plan.scratch_bytes == scratch and 0 < plan.lds_bytes <= 64 * 1024
    if what == 'the cap of a handle':
        assert plan.n_tiles == 256 * 1024 and plan.grids[1] == 65536 and plan.grids[2] == 12800
    if what == 'lowered cap':
        assert plan.grids == (1, 3, 3, 3)
    if what == 'one tile':
        assert plan.n_tiles == 1 and plan.grids == (1, 1, 1, 1)
    if what == 'one pixel more than a tile':
        assert plan.n_tiles == 4


def test_plan_refuses_what_the_call_refuses():
    good = lambda: residual.descriptor((16, 16), np.uint8, 1, 0, 7, 'ring')
    for field, value in (('ndim', 4), ('fit_function', 4), ('n_profile', 0), ('outside', 3), ('want_frames', 2),
                         ('max_grid', -1), ('n_features', 2 ** 31 - 1), ('n_frames', -1), ('isotropic', 2)):
        d = good()
        setattr(d, field, value)
        with pytest.raises(ValueError, match='ctr_residual_plan'):
            _lib.residual_plan(d)
    d = good()
    d.radius[1] = 0
    with pytest.raises(ValueError, match='radius'):
        _lib.residual_plan(d)
    d = good()
    d.radius[0] = 1025
    with pytest.raises(NotImplementedError, match='radius'):
        _lib.residual_plan(d)
    d = residual.descriptor((16, 16), np.uint8, 1, 0, 7, 'inv_series_2')
    d.n_profile = 8
    with pytest.raises(ValueError, match='n_profile'):
        _lib.residual_plan(d)
