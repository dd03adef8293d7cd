"""clustertracking_amd.shape without a GPU: the NumPy restatement of its rule (tests/_shape.py) against
hand-computed clusters, the names and the number of coordinates of every geometry, argument errors
raised before the engine is touched, the three entry points and the plan declared, exported and laid
out as the header says, the launch decision of the dynamics restated from the source and equal to
ctr_shape_plan at its edges, and the condition on the inputs of the GPU histogram tests.

Tolerances: a hand-computed bond or radius of gyration that is a representable number is met exactly;
angles and irrational lengths within 4 ulp of the value (atol 1e-15 on O(1) numbers).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _cases
import _shape as S
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib, shape

GEOMETRIES = [(2, 2), (2, 3), (2, 4), (3, 2), (3, 3), (3, 4)]       # (ndim, cluster_size): the 2D tetramer included
PI = np.pi


def _one(points, mpp=1.):
    p = np.asarray(points, dtype=np.float64)
    return S.coords(p[None, None], p.shape[0], p.shape[1], mpp)[0, 0]


# ---- rule 1 against hand-computed clusters ----------------------------------------------------------
def test_triangle_3_4_5():
    q = _one([[0., 0.], [3., 0.], [0., 4.]])
    assert S.names(3) == ('bond_01', 'bond_02', 'bond_12', 'angle_0_12', 'angle_1_02', 'angle_2_01', 'rg')
    assert list(q[:3]) == [3., 4., 5.]
    assert np.abs(q[3:6] - [PI / 2, np.arctan2(4., 3.), np.arctan2(3., 4.)]).max() <= 1e-15
    assert abs(q[3:6].sum() - PI) <= 1e-15
    assert abs(q[6] - np.sqrt(50. / 9.)) <= 1e-15            # rg^2 = (a^2 + b^2 + c^2) / 9
    # the same triangle in 3D, in a tilted plane
    q3 = _one([[1., 1., 1.], [1., 4., 1.], [1., 1., 5.]])
    assert list(q3[:3]) == [3., 4., 5.] and np.abs(q3[3:] - q[3:]).max() <= 1e-15


def test_unit_square_2d():
    q = _one([[0., 0.], [0., 1.], [1., 1.], [1., 0.]])
    names = S.names(4)
    assert len(names) == 19 and names[:6] == ('bond_01', 'bond_02', 'bond_03', 'bond_12', 'bond_13', 'bond_23')
    assert names[6:9] == ('angle_0_12', 'angle_0_13', 'angle_0_23') and names[-4:] == ('angle_3_01', 'angle_3_02', 'angle_3_12', 'rg')
    r2 = np.sqrt(2.)
    assert list(q[:6]) == [1., r2, 1., 1., r2, 1.]
    # at every vertex the two sides enclose pi / 2, a side and the diagonal pi / 4, in the order of the names
    want = {0: [PI / 4, PI / 2, PI / 4], 1: [PI / 2, PI / 4, PI / 4], 2: [PI / 4, PI / 4, PI / 2], 3: [PI / 4, PI / 2, PI / 4]}
    for a in range(4):
        assert np.abs(q[6 + 3 * a:9 + 3 * a] - want[a]).max() <= 1e-15, a
    assert q[18] == np.sqrt(0.5)


def test_regular_tetrahedron():
    q = _one([[1., 1., 1.], [1., -1., -1.], [-1., 1., -1.], [-1., -1., 1.]])
    assert (q[:6] == np.sqrt(8.)).all()
    assert np.abs(q[6:18] - PI / 3).max() <= 1e-15
    assert q[18] == np.sqrt(3.)


def test_collinear_trimer_and_coincident_features():
    q = _one([[0., 0.], [0., 1.], [0., 2.]])
    assert list(q[:3]) == [1., 2., 1.] and list(q[3:6]) == [0., PI, 0.]
    q = _one([[0., 0., 0.], [0., 0., 1.], [0., 0., 2.]])
    assert list(q[3:6]) == [0., PI, 0.]
    for ndim in (2, 3):                                     # coincident: what IEEE atan2 gives, no error
        for n in (2, 3, 4):
            q = _one(np.full((n, ndim), 2.5))
            assert (q == 0.).all() and not np.signbit(q).any(), (ndim, n)
        q = _one([[1.] * ndim, [1.] * ndim, [-3.] * ndim])  # two of three coincide: u = 0 and u . v = -0
        assert q[0] == 0. and list(q[3:5]) == [0., 0.] and q[5] == 0.


def test_per_axis_mpp_and_missing_data():
    q = _one([[0., 0., 0.], [1., 1., 1.]], mpp=(2., 3., 6.))
    assert list(q) == [7., 3.5]
    q = _one([[0., 0.], [3., 2.]], mpp=(1., 2.))
    assert list(q) == [5., 2.5]
    pos = np.zeros((2, 3, 3, 2))
    pos[0, 1, 2, 1] = np.nan
    pos[1, 2, 0, 0] = np.inf
    q = S.coords(pos, 3, 2)
    assert np.isnan(q[0, 1]).all() and np.isnan(q[1, 2]).all() and np.isfinite(q).sum() == 4 * 7


@pytest.mark.parametrize('ndim,n', GEOMETRIES)
def test_names_and_counts(ndim, n):
    names = shape.shape_names(n)
    assert names == S.names(n) and len(names) == S.n_coords(n) == {2: 2, 3: 7, 4: 19}[n]
    assert len(set(names)) == len(names) and names[-1] == 'rg'
    nb = n * (n - 1) // 2
    assert all(x.startswith('bond_') for x in names[:nb]) and all(x.startswith('angle_') for x in names[nb:-1])
    assert len(names) - 1 - nb == {2: 0, 3: 3, 4: 12}[n]
    q = S.coords(S.clusters(np.random.RandomState(n), 2, 9, n, ndim), n, ndim, 0.5)
    assert q.shape == (2, 9, len(names))
    ok = np.isfinite(q[..., 0])
    assert (q[ok][:, nb:-1] >= 0.).all() and (q[ok][:, nb:-1] <= PI).all()
    if n == 3:                                              # the angles of a triangle add up to pi
        assert np.abs(q[ok][:, 3:6].sum(1) - PI).max() <= 1e-14


def test_restated_dynamics_and_histogram_by_hand():
    """one dimer breathing 1, 2, 4, NaN, 7: the rows of lag 1 are (1, 2) and (2, 4), of lag 2 (1, 4) and
    (4, 7); bond and rg = bond / 2"""
    pos = np.zeros((1, 5, 2, 2))
    pos[0, :, 1, 1] = [1., 2., 4., np.nan, 7.]
    q = S.coords(pos, 2, 2)
    assert list(q[0, :, 0][[0, 1, 2, 4]]) == [1., 2., 4., 7.] and np.isnan(q[0, 3]).all()
    d = S.dynamics(q, [1, 2, 4, 5], fps=10.)
    assert d['n'][0, 0].tolist() == [2, 2, 1, 0] and d['n_frames'].tolist() == [[4, 4]]
    assert d['mean_d'][0, 0, :3].tolist() == [1.5, 3., 6.] and d['mean_d2'][0, 0, :3].tolist() == [2.5, 9., 36.]
    assert d['mean_d4'][0, 0, :3].tolist() == [8.5, 81., 1296.] and np.isnan(d['mean_d'][0, :, 3]).all()
    assert d['flex'][0, 0, :3].tolist() == [12.5, 22.5, 45.] and d['flex'][0, 1, 0] == 12.5 / 4
    assert d['mean'][0, 0] == 3.5 and d['var'][0, 0] == 5.25 and (d['min'][0, 0], d['max'][0, 0]) == (1., 7.)
    assert (d['pooled_n'] == d['n'][0]).all() and d['pooled_mean_d2'][0, 1] == 9.
    h = S.histogram(q, 2, 4., 1., 3)
    # bonds 1, 2 fall in the upper bin of their edge, 4 and 7 are above; rg 0.5, 1, 2, 3.5
    assert h['count_bond'].tolist() == [[0, 1, 1, 0], [1, 1, 1, 1]] and h['above'].tolist() == [2, 0] and h['n'].tolist() == [4]
    assert h['count_angle'].shape == (0, 3) and h['density_bond'][1].tolist() == [0.25] * 4
    assert (h['count_bond'].sum(1) + h['above'] == h['n']).all()


# ---- arguments ---------------------------------------------------------------------------------------
def test_refusals_before_the_engine(monkeypatch):
    def no_engine(device=0):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    pos = np.zeros((2, 5, 3, 2))
    for call in (lambda *a, **k: shape.shape_arrays(*a, **k),
                 lambda *a, **k: shape.shape_dynamics_arrays(*a, lagtime=1, **k),
                 lambda *a, **k: shape.shape_histogram_arrays(*a, bond_max=2., bond_dr=0.1, angle_bins=10, **k)):
        with pytest.raises(ValueError, match='cluster_size'):
            call(pos, 5, 2)
        with pytest.raises(ValueError, match='cluster_size'):
            call(pos, 1, 2)
        with pytest.raises(ValueError, match='ndim'):
            call(pos, 3, 4)
        with pytest.raises(ValueError, match='pos must be'):
            call(pos, 2, 2)
        with pytest.raises(ValueError, match='pos must be'):
            call(pos[0], 3, 2)
        with pytest.raises(ValueError, match='mpp'):
            call(pos, 3, 2, mpp=np.inf)
        with pytest.raises(ValueError, match='mpp'):
            call(pos, 3, 2, mpp=(1., 1., 1.))
        with pytest.raises(ValueError, match='numbers'):
            call(pos.astype(str), 3, 2)
    with pytest.raises(ValueError, match='lagtime'):
        shape.shape_dynamics_arrays(pos, 3, 2, 0)
    with pytest.raises(ValueError, match='lagtime'):
        shape.shape_dynamics_arrays(pos, 3, 2, [1, 2.5])
    with pytest.raises(ValueError, match='fps'):
        shape.shape_dynamics_arrays(pos, 3, 2, 1, fps=0.)
    hist = shape.shape_histogram_arrays
    with pytest.raises(ValueError, match='bond_dr'):
        hist(pos, 3, 2, 2., 0., 10)
    with pytest.raises(ValueError, match='bond_max'):
        hist(pos, 3, 2, np.nan, 0.1, 10)
    with pytest.raises(ValueError, match='more than 4096'):
        hist(pos, 3, 2, 4097., 1., 10)
    with pytest.raises(ValueError, match='angle_bins'):
        hist(pos, 3, 2, 2., 0.1, 1025)
    with pytest.raises(ValueError, match='angle_bins'):
        hist(pos, 3, 2, 2., 0.1, 0)
    with pytest.raises(ValueError, match='cluster_size'):
        shape.shape_df(None, 7)
    with pytest.raises(ValueError, match='lagtime'):
        shape.flexibility(None, 2, -1)
    with pytest.raises(AssertionError, match='engine was touched'):      # a good call gets as far as the engine
        shape.shape_arrays(pos, 3, 2)
    with pytest.raises(AssertionError, match='engine was touched'):      # the 2D tetramer is accepted
        shape.shape_arrays(np.zeros((1, 2, 4, 2)), 4, 2)


def test_bins():
    B, be, A, ae, width = shape.bins(16., 2. ** -8, 1024)
    assert (B, A) == (4096, 1024) and be[-1] == 16. and ae[0] == 0. and ae[-1] == np.pi and width == np.pi / 1024
    assert (be == np.arange(4097) * 2. ** -8).all() and (ae == np.linspace(0., np.pi, 1025)).all()
    assert shape.bins(1., 0.3, 1)[0] == 4 and shape.bins(3., 3., 1)[0] == 1
    for case in S.HIST_CASES.values():
        be, ae = S.edges(case['bond_max'], case['bond_dr'], case['angle_bins'])
        got = shape.bins(case['bond_max'], case['bond_dr'], case['angle_bins'])
        assert (got[1] == be).all() and (got[3] == ae).all()


# ---- the interface -----------------------------------------------------------------------------------
CALLS = {'ctr_shape_device': _abi.Shape, 'ctr_shape_dynamics_device': _abi.ShapeDynamics,
         'ctr_shape_histogram_device': _abi.ShapeHistogram}


def test_declared_exported_and_mirrored():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    for clause in ('Rule 1', 'Rule 2', 'Rule 3', 'Bonds:', 'Angles:', 'Radius of gyration', 'Missing data:'):
        assert clause in header, clause
    for clause in ('1. The coordinates', '2. Dynamics', '3. Distributions', 'no CPU fallback'):
        assert clause in shape.__doc__, clause
    bare = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', bare))
    assert set(protos) == set(_lib.SIGNATURES)
    lib = _lib.load()
    for call, cls in CALLS.items():
        cname = call[:-len('_device')]
        params = [p.strip() for p in protos[call].split(',')]
        assert params[0] == 'ctr_handle* h' and params[1].startswith('const %s* ' % cname) and params[2] == 'void* hip_stream'
        assert _lib.SIGNATURES[call] == _lib._stage(cls) and call in _lib.EXPORTS and hasattr(lib, call)
        assert callable(getattr(_lib.Engine, call[len('ctr_'):]))
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), bare, flags=re.S).group(1)
        assert re.findall(r'\b(\w+)(?:\[\w+\])?\s*;', body) == [f[0] for f in cls._fields_], cname
    assert 'ctr_shape_plan' in protos and hasattr(lib, 'ctr_shape_plan') and callable(_lib.shape_plan)
    defines = dict(re.findall(r'#define\s+(CTR_SHAPE_\w+)\s+(\d+)', header))
    assert defines == {'CTR_SHAPE_MAX_COORDS': '19', 'CTR_SHAPE_TILE': '256', 'CTR_SHAPE_HALO_CAP': '768',
                       'CTR_SHAPE_MAX_BOND_BINS': '4096', 'CTR_SHAPE_MAX_ANGLE_BINS': '1024'}
    assert (_abi.SHAPE_MAX_COORDS, _abi.SHAPE_TILE, _abi.SHAPE_HALO_CAP) == (19, 256, 768)
    assert (_abi.SHAPE_MAX_BOND_BINS, _abi.SHAPE_MAX_ANGLE_BINS) == (4096, 1024)


def test_struct_layout_matches_the_compiler(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    want = []
    for call, cls in CALLS.items():
        cname = call[:-len('_device')]
        src += 'printf("%%zu\\n", sizeof(%s));\n' % cname
        want.append(ctypes.sizeof(cls))
        for f in cls._fields_:
            src += 'printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0])
            want.append(getattr(cls, f[0]).offset)
    src += 'return 0;}\n'
    (tmp_path / 'layout.c').write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == want


def test_public_names():
    names = {'shape_arrays', 'shape_dynamics_arrays', 'shape_histogram_arrays', 'shape_names', 'shape_df', 'flexibility'}
    assert names | {'shape'} <= set(ct.__all__) and ct.shape is shape
    for name in names:
        assert getattr(ct, name) is getattr(shape, name)
    assert shape.Shape._fields == ('coords', 'names')
    assert shape.ShapeDynamics._fields == (
        'lags', 'names', 'n', 'mean_d', 'mean_d2', 'mean_d4', 'flex', 'pooled_n', 'pooled_mean_d', 'pooled_mean_d2',
        'pooled_mean_d4', 'pooled_flex', 'n_frames', 'mean', 'var', 'min', 'max')
    assert shape.ShapeHistogram._fields == ('names_bond', 'names_angle', 'bond_edges', 'angle_edges', 'count_bond', 'above',
                                            'count_angle', 'n', 'density_bond', 'density_angle')


# ---- the launch decision -----------------------------------------------------------------------------
def test_launch_decision_restated_from_the_source():
    csrc = os.path.join(_cases.ROOT, 'clustertracking_amd', 'csrc')
    kern = open(os.path.join(csrc, 'shape_kernels.h')).read()
    host = open(os.path.join(csrc, 'tu_shape.hip')).read()
    for name in ('SHP_THREADS', 'SHP_NSUM', 'SHP_RED_ROW'):
        assert re.search(r'constexpr int %s = %d;' % (name, getattr(S, name)), kern), name
    assert 'SHP_TILE = CTR_SHAPE_TILE;' in kern and 'SHP_HALO_CAP = CTR_SHAPE_HALO_CAP;' in kern
    assert 'SHP_LDS_MAX = 64 * 1024;' in host and 'constexpr int SHP_HIST_CHUNK = 4096;' in kern
    assert [S.shp_halo_max(S.n_coords(n)) for n in (2, 3, 4)] == [768, 768, 158]
    for C in (2, 7, 19):
        assert S.shp_lds_bytes(S.shp_halo_max(C), C) <= S.SHP_LDS_MAX
    assert S.shp_lds_bytes(159, 19) > S.SHP_LDS_MAX                    # the tetramer's halo is what 64 KiB hold
    assert [S.shp_halo(F, 19) for F in (0, 1, 256, 257, 414, 415, 10 ** 6)] == [0, 0, 0, 1, 158, 158, 158]
    assert [S.shp_halo(F, 2) for F in (256, 1024, 1025)] == [0, 768, 768]
    # every later frame is staged while the video fits tile + halo; beyond that a long lag reads global memory
    assert not any(S.shp_reads_global(414, 19, k) for k in range(1, 414))
    assert [S.shp_reads_global(444, 19, k) for k in (1, 158, 159, 414, 443, 444)] == [False, False, True, True, True, False]
    assert [S.shp_reads_global(1054, 2, k) for k in (768, 769)] == [False, True]


@pytest.mark.parametrize('n', [2, 3, 4])
def test_plan_equals_the_restated_decision(n):
    C = S.n_coords(n)
    top = S.shp_halo_max(C)
    for F in (0, 1, 255, 256, 257, 256 + top - 1, 256 + top, 256 + top + 1, 10 ** 6):
        for T, L in ((1, 1), (3, 100)):
            tile, halo, lds, n_tiles, scratch = _lib.shape_plan(shape.dynamics_descriptor(n, 2, T, F, L))
            assert (tile, halo, lds) == (S.TILE, S.shp_halo(F, C), S.shp_lds_bytes(S.shp_halo(F, C), C)), (F, T, L)
            assert n_tiles == -(-F // S.TILE) and lds <= S.SHP_LDS_MAX
            coords_bytes = -(-8 * T * F * C // 256) * 256
            assert scratch == coords_bytes + 8 * T * (n_tiles + 1) * L * C * S.SHP_NSUM + 256     # partials, sums of the tracks
    assert _lib.shape_plan(shape.dynamics_descriptor(n, 3, 5, 300, 7))[:2] == (256, S.shp_halo(300, C))     # ndim plays no part
    with pytest.raises(ValueError, match='cluster_size'):
        _lib.shape_plan(shape.dynamics_descriptor(5, 2, 1, 10, 1))
    with pytest.raises(ValueError, match='ndim'):
        _lib.shape_plan(shape.dynamics_descriptor(n, 4, 1, 10, 1))
    with pytest.raises(ValueError, match='too many'):
        _lib.shape_plan(shape.dynamics_descriptor(n, 2, 2 ** 20, 2 ** 20, 1))
    with pytest.raises(ValueError, match='fps'):
        _lib.shape_plan(shape.dynamics_descriptor(n, 2, 1, 10, 1, fps=0.))


# ---- the condition on the inputs of the GPU histogram tests -------------------------------------------
@pytest.mark.parametrize('name', sorted(S.HIST_CASES))
def test_histogram_inputs_keep_their_angles_off_the_edges(name):
    """device angles are a few ulp from NumPy's (atol 1e-12 in tests/test_gpu_shape.py), so an angle
    within 1e-9 of an edge could be counted on either side: the seeds are drawn until none is, and
    here, on the CPU, that is checked once"""
    case = S.HIST_CASES[name]
    pos, q, seed = S.clusters_off_edges(case['seed'], case['T'], case['F'], case['cluster_size'], case['ndim'], case['mpp'],
                                        case['angle_bins'])
    assert seed == case['seed']                              # the recorded seed holds without a retry
    assert S.min_angle_edge_distance(q, case['cluster_size'], case['angle_bins']) > 1e-9
    h = S.histogram(q, case['cluster_size'], case['bond_max'], case['bond_dr'], case['angle_bins'], case['per_track'])
    assert (h['count_bond'].sum(-1) + h['above'] == h['n'][..., None]).all()
    assert (h['count_angle'].sum(-1) == h['n'][..., None]).all() and h['n'].sum() > 0
    assert h['above'].sum() > 0 or name == 'two_chunks'      # the reach cuts the bonds' tail
