"""clustertracking_amd.motion without a GPU: the NumPy restatement of its rule (tests/_motion.py)
reproduces what the reference gives (tests/golden/motion/motion_cases.npz, written by
tests/golden/make_golden_motion.py), the two entry points are declared, exported and laid out as
the header says, argument errors are raised before a device is needed, and the host plumbing of
orientation_df builds the arrays the reference's loop would.

Tolerances: com and bases are short float64 chains on O(1) values: atol 1e-12 (a few thousand
ulp).  A tensor is a mean of at most ~500 float64 products: within 1e-10 of its largest entry
(n eps is ~1e-13).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _cases
import _motion as M
import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib, motion

CASES = M.load_cases()
IDS = [c['name'] for c in CASES]


def test_fixture_set():
    """the five geometries, one case without sizes, the 3D dimer with its recorded angles"""
    geo = {(c['ndim'], c['cluster_size']) for c in CASES}
    assert geo == {(2, 2), (2, 3), (3, 3), (3, 4), (3, 2)}
    assert sum(c['sizes'] is None for c in CASES) == 1
    for c in CASES:
        F = len(c['com'])
        assert 35 <= F <= 45 and c['mpp'] != 1. and c['table'][:, 0].min() > 0
        assert list(c['lags']) == [1, 3, F - 1]
        assert np.isnan(c['com']).all(1).sum() == 3        # two frames without rows, one a feature short
        assert (c['angles'] is not None) == ((c['ndim'], c['cluster_size']) == (3, 2))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_restatement_reproduces_reference_orientation(case):
    com, bases = M.orientation(M.dense_from_table(case), case['cluster_size'], case['ndim'], case['mpp'],
                               case['sizes'], None if case['angles'] is None else case['angles'][None])
    M.assert_same(com[0], case['com'], 1e-12, 'com')
    M.assert_same(bases[0], case['bases'], 1e-12, 'bases')


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_restatement_reproduces_reference_tensor(case):
    tensor, counts = M.diffusion_tensor(case['com'][None], case['bases'][None], case['lags'], case['fps'], case['ndim'])
    M.assert_tensors(tensor[0], case['tensors'])
    assert counts[0, -1] == len(case['bases'])             # lag F - 1: one row per permutation
    # a lag beyond the video, and a track of NaN: a NaN tensor and count 0
    tensor, counts = M.diffusion_tensor(np.stack([case['com'], case['com'] * np.nan]), np.stack([case['bases']] * 2),
                                        [2, len(case['com'])], case['fps'], case['ndim'])
    assert counts[0, 0] > 0 and np.isfinite(tensor[0, 0]).all()
    assert (counts[:, 1] == 0).all() and counts[1, 0] == 0 and np.isnan(tensor[1]).all() and np.isnan(tensor[:, 1]).all()


def test_restatement_degenerate_geometry_is_nan():
    """coincident features, a collinear 3D trimer, a 3D dimer along [1, 0, 0]: NaN bases, finite com"""
    pos = np.array([[[[3., 4.], [3., 4.]], [[3., 4.], [5., 4.]]]])                       # [1, 2, 2, 2]
    com, bases = M.orientation(pos, 2, 2)
    assert np.isnan(bases[0, :, 0]).all() and np.isfinite(bases[0, :, 1]).all() and np.isfinite(com).all()
    pos = np.array([[[[0., 0., 0.], [0., 0., 1.], [0., 0., 2.]], [[0., 0., 0.], [0., 1., 1.], [0., 0., 2.]]]])
    com, bases = M.orientation(pos, 3, 3)
    assert np.isnan(bases[0, :, 0]).all() and np.isfinite(bases[0, :, 1]).all() and np.isfinite(com).all()
    pos = np.array([[[[0., 0., 0.], [0., 0., 2.]], [[0., 0., 0.], [0., 1., 2.]]]])       # z, y, x: along x
    com, bases = M.orientation(pos, 2, 3, angles=np.full((1, 2, 2), 0.3))
    assert np.isnan(bases[0, :, 0]).all() and np.isfinite(bases[0, :, 1]).all() and np.isfinite(com).all()


def test_permutation_tables():
    assert {k: [list(p) for p in v] for k, v in motion.PERMUTATIONS.items()} == M.PERMUTATIONS
    assert [len(motion.PERMUTATIONS[k]) for k in (2, 3, 4)] == [2, 6, 12]


# ---- the interface -----------------------------------------------------------------------------
def test_abi_and_exports():
    assert _abi.ABI_VERSION == 8
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define CTR_ABI_VERSION 8\b', header)
    declared = set(re.findall(r'\b(ctr_[a-z_]+)\s*\(', header))
    lib = _lib.load()
    assert lib.ctr_abi_version() == 8
    for name in ('ctr_orientation_device', 'ctr_diffusion_device'):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert 'motion' in cta.__all__ and cta.motion is motion
    for name in ('orientation_arrays', 'orientation_df', 'diffusion_tensor', 'friction_tensor'):
        assert callable(getattr(motion, name))
    assert not hasattr(motion, 'diffusion_tensor_ci')


def test_struct_layout_matches_header(tmp_path):
    """the ctypes mirrors of the two descriptors against the C compiler's view of the header"""
    structs = (('ctr_orientation', _abi.Orientation), ('ctr_diffusion', _abi.Diffusion))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    for cname, cls in structs:
        src += 'printf("%%zu\\n", sizeof(%s));\n' % cname
        for f in cls._fields_:
            src += 'printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f[0])
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    want = []
    for cname, cls in structs:
        want += [ctypes.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
    assert out == want


def test_launch_decision_restated_from_the_source():
    """the constants of tests/_motion.py are the source's, the staged tile fills 64 KiB and no more"""
    csrc = os.path.join(_cases.ROOT, 'clustertracking_amd', 'csrc')
    kern = open(os.path.join(csrc, 'motion_kernels.h')).read()
    host = open(os.path.join(csrc, 'tu_motion.hip')).read()
    for name in ('MOT_THREADS', 'MOT_TILE', 'MOT_ROW', 'MOT_NSUM', 'MOT_NPAD'):
        assert re.search(r'constexpr int %s = %d;' % (name, getattr(M, name)), kern), name
    assert 'MOT_LDS_MAX = 64 * 1024;' in host
    assert M.MOT_HALO_MAX == 418 and M.TILE == 256
    assert M.mot_lds_bytes(M.MOT_HALO_MAX) <= M.MOT_LDS_MAX < M.mot_lds_bytes(M.MOT_HALO_MAX + 1)
    assert [M.mot_halo(F) for F in (0, 1, 256, 257, 674, 675, 10 ** 6)] == [0, 0, 0, 1, 418, 418, 418]
    # every later frame of a video of up to TILE + MOT_HALO_MAX frames is staged; beyond that the
    # lags above the halo read global memory
    assert not any(M.mot_reads_global(674, lag) for lag in range(1, 674))
    assert not M.mot_reads_global(675, 418) and M.mot_reads_global(675, 419)
    assert M.mot_reads_global(704, 500) and not M.mot_reads_global(704, 704)


# ---- argument errors: raised before a device is needed -------------------------------------------
def test_argument_errors():
    pos2 = np.zeros((1, 5, 2, 2))
    with pytest.raises(NotImplementedError, match='single particle'):
        motion.orientation_arrays(np.zeros((1, 5, 1, 2)), 1, 2)
    with pytest.raises(NotImplementedError, match='single particle'):
        motion.orientation_arrays(np.zeros((1, 5, 1, 3)), 1, 3)
    with pytest.raises(NotImplementedError, match='2D tetramer'):
        motion.orientation_arrays(np.zeros((1, 5, 4, 2)), 4, 2)
    with pytest.raises(ValueError, match='angles'):
        motion.orientation_arrays(np.zeros((1, 5, 2, 3)), 2, 3)
    with pytest.raises(ValueError, match='angles'):
        motion.orientation_arrays(np.zeros((1, 5, 2, 3)), 2, 3, angles=np.zeros((1, 2, 4)))
    for bad in (np.zeros((5, 2, 2)), np.zeros((1, 5, 3, 2)), np.zeros((1, 5, 2, 3))):
        with pytest.raises(ValueError, match='pos must be'):
            motion.orientation_arrays(bad, 2, 2)
    with pytest.raises(ValueError, match='sizes'):
        motion.orientation_arrays(pos2, 2, 2, sizes=[1., 2., 3.])
    with pytest.raises(ValueError):
        motion.orientation_arrays(pos2, 5, 2)
    with pytest.raises(ValueError):
        motion.orientation_arrays(np.zeros((1, 5, 2, 4)), 2, 4)
    com, bases = np.zeros((5, 3)), np.zeros((2, 5, 3, 3))
    for lag in (0, -1, [1, 0], 1.5):
        with pytest.raises(ValueError, match='lagtime'):
            motion.diffusion_tensor(com, bases, lag)
    with pytest.raises(ValueError, match='ndim'):
        motion.diffusion_tensor(com, bases, 1, ndim=4)
    with pytest.raises(ValueError, match='fps'):
        motion.diffusion_tensor(com, bases, 1, fps=0.)
    for p, o in ((np.zeros((5, 2)), bases), (com, np.zeros((2, 4, 3, 3))), (com, np.zeros((2, 5, 3, 2))),
                 (com[None], bases), (com, bases[None]), (np.zeros((2, 5, 3)), bases[None])):
        with pytest.raises(ValueError):
            motion.diffusion_tensor(p, o, 1)


def test_orientation_df_argument_errors():
    f = M.table_frame(CASES[0])
    with pytest.raises(NotImplementedError):
        motion.orientation_df(f, cluster_size=1)
    with pytest.raises(NotImplementedError):
        motion.orientation_df(f, cluster_size=4)             # no z column: 2D
    f3 = M.table_frame([c for c in CASES if c['name'] == 'd3_dimer'][0])
    with pytest.raises(ValueError, match='angles'):
        motion.orientation_df(f3, cluster_size=2)
    with pytest.raises(ValueError, match='angles'):
        motion.orientation_df(f3, cluster_size=2, angles=np.zeros((2, 3)))


def _reject(call, desc, code, text):
    lib = _lib.load()
    rc = getattr(lib, call)(None, ctypes.byref(desc), None)
    msg = (lib.ctr_last_error(None) or b'').decode()
    assert rc == code and text in msg and msg.startswith(call), (rc, msg)


def test_descriptors_are_checked_before_the_handle():
    """with a NULL handle a bad descriptor is reported as such, a good one as "null handle\""""
    def ori(**kw):
        d = _abi.Orientation()
        d.ndim, d.cluster_size, d.n_tracks, d.n_frames, d.mpp = 3, 3, 2, 5, 0.5
        for k in range(4):
            d.weights[k] = 1.
        d.pos = d.com = d.bases = 8         # never dereferenced: the handle is NULL
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    call = 'ctr_orientation_device'
    _reject(call, ori(), _abi.ERR_INVALID, 'null handle')
    _reject(call, ori(ndim=4), _abi.ERR_INVALID, 'ndim')
    _reject(call, ori(cluster_size=1), _abi.ERR_UNSUPPORTED, 'single particle')
    _reject(call, ori(ndim=2, cluster_size=1), _abi.ERR_UNSUPPORTED, 'single particle')
    _reject(call, ori(ndim=2, cluster_size=4), _abi.ERR_UNSUPPORTED, '2D tetramer')
    _reject(call, ori(cluster_size=5), _abi.ERR_INVALID, 'cluster_size')
    _reject(call, ori(cluster_size=0), _abi.ERR_INVALID, 'cluster_size')
    _reject(call, ori(cluster_size=2), _abi.ERR_INVALID, 'angles')
    _reject(call, ori(cluster_size=2, angles=8), _abi.ERR_INVALID, 'null handle')
    _reject(call, ori(n_frames=-1), _abi.ERR_INVALID, 'negative')
    _reject(call, ori(mpp=float('nan')), _abi.ERR_INVALID, 'mpp')
    _reject(call, ori(bases=None), _abi.ERR_INVALID, 'null input or output')
    _reject(call, ori(n_tracks=2 ** 40, n_frames=2 ** 20), _abi.ERR_INVALID, 'too many')
    d = ori()
    d.weights[2] = float('inf')
    _reject(call, d, _abi.ERR_INVALID, 'weights')

    def dif(**kw):
        d = _abi.Diffusion()
        d.ndim, d.n_perm, d.n_tracks, d.n_frames, d.n_lags, d.fps = 3, 6, 2, 5, 3, 10.
        d.lags = d.positions = d.bases = d.tensor = d.n_samples = 8
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    call = 'ctr_diffusion_device'
    _reject(call, dif(), _abi.ERR_INVALID, 'null handle')
    _reject(call, dif(ndim=1), _abi.ERR_INVALID, 'ndim')
    _reject(call, dif(n_perm=0), _abi.ERR_INVALID, 'n_perm')
    _reject(call, dif(n_lags=-1), _abi.ERR_INVALID, 'negative')
    _reject(call, dif(fps=0.), _abi.ERR_INVALID, 'fps')
    _reject(call, dif(fps=float('nan')), _abi.ERR_INVALID, 'fps')
    _reject(call, dif(lags=None), _abi.ERR_INVALID, 'null lags or output')
    _reject(call, dif(bases=None), _abi.ERR_INVALID, 'null input')
    _reject(call, dif(n_tracks=2 ** 30, n_frames=2 ** 20), _abi.ERR_INVALID, 'too many')
    lib = _lib.load()
    assert lib.ctr_orientation_device(None, None, None) == _abi.ERR_INVALID
    assert lib.ctr_diffusion_device(None, None, None) == _abi.ERR_INVALID


# ---- the host plumbing of orientation_df, with the restatement in the engine's place -----------
@pytest.fixture
def restated_engine(monkeypatch):
    def arrays(pos, cluster_size, ndim, mpp=1., sizes=None, angles=None, device=0):
        motion._check_geometry(cluster_size, ndim)
        return M.orientation(pos, cluster_size, ndim, mpp, sizes, angles)
    monkeypatch.setattr(motion, 'orientation_arrays', arrays)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_orientation_df_builds_the_reference_arrays(case, restated_engine):
    com, bases = motion.orientation_df(M.table_frame(case), case['cluster_size'], case['mpp'], None, case['sizes'],
                                       case['angles'])
    M.assert_same(com, case['com'], 1e-12, 'com')          # the reference's shapes: (length, 3), (P, length, 3, 3)
    M.assert_same(bases, case['bases'], 1e-12, 'bases')


def test_orientation_df_groups_and_tracks(restated_engine):
    """of several qualifying (frame, cluster) groups of a frame the last in sorted order wins, a
    later group of another size does not; with a track column every track has its own axis entry,
    frames counted from the table's first frame"""
    case = [c for c in CASES if c['name'] == 'd2_trimer'][0]
    f = M.table_frame(case)
    first = int(f['frame'].min())
    other = f[f['frame'] == first + 3].copy()
    other['cluster'] = 9                              # sorts behind cluster 5: it wins
    other[['y', 'x']] += 20.
    short = f[(f['frame'] == first + 4) & (f['particle'] != 10)].copy()
    short['cluster'] = 9                              # two rows: does not count
    both = pd_concat([f, other, short])
    com, bases = motion.orientation_df(both, 3, case['mpp'], sizes=case['sizes'])
    want = case['com'].copy()
    want[3, :2] += 20. * case['mpp']
    M.assert_same(com, want, 1e-10, 'com')
    M.assert_same(bases, case['bases'], 1e-10, 'bases')
    # two tracks: the second starts five frames later and is shifted
    g = f.copy()
    g['frame'] += 5
    g[['y', 'x']] += 7.
    f['track'], g['track'] = 4, 2
    com, bases, ids = motion.orientation_df(pd_concat([f, g]), 3, case['mpp'], sizes=case['sizes'], track_column='track')
    F = len(case['com'])
    assert list(ids) == [2, 4] and com.shape == (2, F + 5, 3) and bases.shape == (2, 6, F + 5, 3, 3)
    M.assert_same(com[1, :F], case['com'], 1e-12)
    M.assert_same(bases[1, :, :F], case['bases'], 1e-12)
    assert np.isnan(com[1, F:]).all() and np.isnan(com[0, :5]).all() and np.isnan(bases[0, :, :5]).all()
    M.assert_same(com[0, 5:, :2], case['com'][:, :2] + 7. * case['mpp'], 1e-10)
    M.assert_same(bases[0, :, 5:], case['bases'], 1e-10)


def pd_concat(frames):
    import pandas as pd
    return pd.concat(frames, ignore_index=True)


def test_friction_tensor_is_the_inverse():
    rng = np.random.RandomState(3)
    a = rng.normal(size=(6, 6))
    d = a.dot(a.T) + 6 * np.eye(6)
    np.testing.assert_allclose(motion.friction_tensor(d).dot(d), np.eye(6), atol=1e-12)
    np.testing.assert_allclose(motion.friction_tensor(d[:3, :3].ravel()).dot(d[:3, :3]), np.eye(3), atol=1e-12)
