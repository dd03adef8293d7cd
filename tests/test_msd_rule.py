"""Mean squared displacement of linked particles, without a device: the yardstick
``tests/_msd.py`` against an independent brute force over all row pairs and on known answers, the
argument errors of the four functions, and the stage path of the two calls -- descriptor before
handle, the header's prototypes, structs and constants against ``_lib`` and ``_abi``, the ABI version
and the public names."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import _cases
import _drift
import _msd as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib
from clustertracking_amd import msd as ms


# ---- the restatement against the brute force: tables of at most 40 rows ----
def _gap_2d():
    """particle 0 misses frames 2 and 3, particle 1 has one row, particle 3 has no row at all"""
    return yard.table([[(0, (1., 2.)), (1, (9., 9.)), (2, (4., 4.))],
                       [(2, (4.5, 3.)), (0, (1.25, 2.5))],
                       [(2, (5.5, 3.25))],
                       [(2, (5.75, 2.))],
                       [(0, (3., 1.)), (2, (7., 2.5)), (4, (0., 0.))],
                       [(4, (0.5, 0.25)), (0, (3.5, 1.75))]])


def _repeated_and_unlinked_3d():
    """id 0 twice in frame 1 (the lowest row wins) and again twice in frame 3; unlinked rows that
    would pair with each other if a negative id were an id"""
    return yard.table([[(0, (0., 0., 0.)), (-1, (5., 5., 5.)), (1, (2., 2., 2.))],
                       [(0, (1., 0.5, 0.25)), (0, (30., 30., 30.)), (1, (2.5, 2., 1.)), (-1, (6., 5., 5.))],
                       [(1, (3., 3., 3.)), (0, (1.5, 1., 1.)), (-7, (7., 7., 7.))],
                       [(0, (2.25, 2., 1.5)), (1, (3.5, 3.25, 3.)), (0, (-40., 0., 0.)), (-7, (8., 7., 7.))]], ndim=3)


def _jittered(ndim):
    return yard.jittered_video(ndim, n_frames=6, n_particles=5, ndim=ndim)


BRUTE = {'gap_2d': (_gap_2d, 1.), 'gap_2d_long_lag': (_gap_2d, 0.5),
         'repeated_3d': (_repeated_and_unlinked_3d, (0.5, 1., 2.)),
         'jitter_2d': (lambda: _jittered(2), (0.16, 0.21)), 'jitter_3d': (lambda: _jittered(3), 0.3)}


@pytest.mark.parametrize('name', sorted(BRUTE))
def test_restatement_equals_the_brute_force(name):
    make, mpp = BRUTE[name]
    pos, off, par = make()
    assert len(pos) <= 40
    T = len(off) - 1
    L = T + 2                                   # L > T - 1
    P = int(par.max()) + 1
    per, pooled = yard.msd(pos, off, par, L, mpp), yard.emsd(pos, off, par, L, mpp)
    cells, pool = yard.brute_force(pos, off, par, L, mpp)
    assert per.msd.shape == (P, L) and per.mean_d.shape == (P, L, pos.shape[1]) and pooled.n.shape == (L,)
    seen = 0
    for p in range(P):
        for k in range(1, L + 1):
            got = (per.msd[p, k - 1], per.mean_d[p, k - 1], per.mean_d2[p, k - 1], per.n[p, k - 1])
            if (p, k) in cells:
                want = cells[(p, k)]
                assert got[3] == want[3] > 0 and got[0] == want[0]
                assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
                seen += 1
            else:
                assert got[3] == 0 and np.isnan(got[0]) and np.isnan(got[1]).all() and np.isnan(got[2]).all()
    assert seen == len(cells) > 0
    for k in range(1, L + 1):
        if k in pool:
            assert pooled.n[k - 1] == pool[k][3] and pooled.msd[k - 1] == pool[k][0]
            assert pooled.mean_d[k - 1].tobytes() == pool[k][1].tobytes() and pooled.mean_d2[k - 1].tobytes() == pool[k][2].tobytes()
        else:
            assert pooled.n[k - 1] == 0 and np.isnan(pooled.msd[k - 1])
    assert np.isnan(per.msd[:, T - 1:]).all() and (per.n[:, T - 1:] == 0).all()       # k beyond any span


def test_tables_hold_what_they_are_for():
    pos, off, par = _gap_2d()
    per = yard.msd(pos, off, par, 5)
    assert per.n[0].tolist() == [2, 0, 1, 2, 1]            # the gap: frames 0, 1, 4, 5
    assert per.n[1].tolist() == [0] * 5 and per.n[3].tolist() == [0] * 5      # one row; no row
    assert per.n[2].tolist() == [4, 3, 2, 1, 0]
    pos, off, par = _repeated_and_unlinked_3d()
    per = yard.msd(pos, off, par, 3, (0.5, 1., 2.))
    assert per.n[0].tolist() == [3, 2, 1]                  # the rows at 30 and -40 do not exist
    np.testing.assert_array_equal(per.mean_d[0, 2], [2.25 * 0.5, 2., 3.])
    np.testing.assert_array_equal(per.mean_d2[0, 2], [(2.25 * 0.5) ** 2, 4., 9.])
    assert per.msd[0, 2] == (2.25 * 0.5) ** 2 + 4. + 9.
    assert yard.emsd(pos, off, par, 3).n.tolist() == [6, 4, 2]


# ---- known answers ----
@pytest.mark.parametrize('ndim', [2, 3])
def test_uniform_motion_gives_v2_k2(ndim):
    v = np.array([3., -2., 5.])[:ndim]
    x0 = np.array([[10., 20., 30.], [-4., 7., 0.5]])[:, :ndim]
    frames = [[(p, tuple(x0[p] + v * t)) for p in range(2) if (p, t) != (1, 3)] for t in range(7)]
    pos, off, par = yard.table(frames, ndim)
    per, pooled = yard.msd(pos, off, par, 8), yard.emsd(pos, off, par, 8)
    k = np.arange(1, 9.)
    want = np.where(k <= 6, (v ** 2).sum() * k ** 2, np.nan)
    np.testing.assert_array_equal(per.msd, np.stack([want, want]))
    np.testing.assert_array_equal(pooled.msd, want)
    np.testing.assert_array_equal(per.mean_d[0, :6], k[:6, None] * v)
    assert per.n[0].tolist() == [6, 5, 4, 3, 2, 1, 0, 0] and per.n[1].tolist() == [4, 3, 2, 3, 2, 1, 0, 0]


def test_msd_is_zero_after_the_restated_drift_is_subtracted():
    """particles that only move with a common drift of exact steps: the restated drift takes all of it"""
    rng = np.random.RandomState(3)
    start = rng.randint(0, 400, (4, 2)) / 4.
    steps = np.cumsum(rng.randint(-8, 9, (6, 2)) / 4., axis=0)
    pos, off, par = yard.table([[(p, tuple(start[p] + steps[t])) for p in rng.permutation(4)] for t in range(6)])
    assert (yard.msd(pos, off, par, 5).msd > 0).any()
    drift = _drift.compute_drift(pos, off, par).drift
    fixed = _drift.subtract_drift(pos, off, drift)
    per = yard.msd(fixed, off, par, 5)
    assert (per.msd == 0.).all() and (per.mean_d == 0.).all() and (per.n > 0).all()
    assert (yard.emsd(fixed, off, par, 5).msd == 0.).all()


@pytest.mark.parametrize('name', ['gap_2d', 'jitter_3d'])
def test_ensemble_is_the_weighted_mean_of_the_particles(name):
    make, mpp = BRUTE[name]
    pos, off, par = make()
    per, pooled = yard.msd(pos, off, par, 5, mpp), yard.emsd(pos, off, par, 5, mpp)
    n = per.n.sum(0)
    assert (n == pooled.n).all() and (n > 0).all()
    P = len(per.n)
    for name, X in (('mean_d', per.max_d.max()), ('mean_d2', per.max_d.max() ** 2)):
        weighted = np.nansum(getattr(per, name) * per.n[..., None], axis=0) / n[:, None]
        # terms of size <= X, u = 2^-53: a particle's mean is off by 2 X u (fsum, division) and its
        # product with n_p by one rounding more, 3 n_p X u; the P - 1 additions of partial sums <= n X
        # add (P - 1) n X u; divided by n and rounded: (P + 3) X u; the pooled mean itself 2 X u
        assert np.abs(weighted - getattr(pooled, name)).max() <= (P + 5) * X * yard.U
    np.testing.assert_allclose(pooled.msd, pooled.mean_d2.sum(-1), rtol=4 * yard.U, atol=0)


def test_bounds_are_small_and_positive():
    pos, off, par = _jittered(2)
    want = yard.msd(pos, off, par, 5)
    assert (yard.bound(want)[want.n > 0] > 0).all() and yard.bound(want).max() < 1e-14
    assert yard.bound_msd(want).max() < 1e-13


# ---- argument errors, before any device work ----
def test_value_errors_before_the_engine(monkeypatch):
    def no_engine(device=0):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    pos, off, par = yard.table([[(0, (0., 0.)), (1, (5., 5.))], [(0, (1., 1.)), (1, (6., 6.))]])
    for fn in (ct.msd_arrays, ct.emsd_arrays):
        for L in (0, -1, 1.5, True, 2 ** 31):
            with pytest.raises(ValueError, match='max_lagtime'):
                fn(pos, off, par, max_lagtime=L)
        with pytest.raises(ValueError, match='pos must be'):
            fn(pos[:, :1], off, par)
        with pytest.raises(ValueError, match='pos must be'):
            fn(pos.reshape(-1), off, par)
        with pytest.raises(ValueError, match='particle'):
            fn(pos, off, par[:3])
        with pytest.raises(ValueError, match='integers'):
            fn(pos, off, par.astype(float))
        with pytest.raises(ValueError, match='frame_offset'):
            fn(pos, off[:0], par)
        for mpp in ((1., 2., 3.), (1.,), np.nan, [[1., 1.]], (1., np.inf)):
            with pytest.raises(ValueError, match='mpp'):
                fn(pos, off, par, mpp=mpp)
        for fps in (0, -2., np.nan, 'fast', True):
            with pytest.raises(ValueError, match='fps'):
                fn(pos, off, par, fps=fps)
        for P in (-1, 1.5, 2 ** 31 - 1):
            with pytest.raises(ValueError, match='particles'):
                fn(pos, off, par, n_particles=P)
    for particles in ([1, 0], [0, 0], [-1, 0], [0, 2], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match='particles'):
            ct.msd_arrays(pos, off, par, particles=particles)
    with pytest.raises(ValueError, match='particles'):
        ct.msd_arrays(pos, off, par, particles=[0, 5], n_particles=5)
    f = pd.DataFrame({'frame': [0, 0, 1, 1], 'y': pos[:, 0], 'x': pos[:, 1], 'particle': par})
    for fn in (ct.imsd, ct.emsd):
        with pytest.raises(ValueError, match="'particle'"):
            fn(f.drop(columns='particle'), 1., 1.)
        with pytest.raises(ValueError, match="'frame'"):
            fn(f.drop(columns='frame'), 1., 1.)
        with pytest.raises(ValueError, match='empty'):
            fn(f.iloc[:0], 1., 1.)
        with pytest.raises(ValueError, match='pos_columns'):
            fn(f, 1., 1., pos_columns=['y', 'q'])
        with pytest.raises(ValueError, match='max_lagtime'):
            fn(f, 1., 1., max_lagtime=0)
        with pytest.raises(ValueError, match='mpp'):
            fn(f, (1., 2., 3.), 1.)
        with pytest.raises(ValueError, match='fps'):
            fn(f, 1., 0.)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    pos, off, par = yard.table([[(0, (0., 0.))], [(0, (1., 1.))]])
    with pytest.raises(_lib.EngineError):
        ct.msd_arrays(pos, off, par)
    with pytest.raises(_lib.EngineError):
        ct.emsd_arrays(pos, off, par)
    f = pd.DataFrame({'frame': [0, 1], 'y': [0., 1.], 'x': [0., 1.], 'particle': [0, 0]})
    with pytest.raises(_lib.EngineError):
        ct.imsd(f, 1., 1.)
    with pytest.raises(_lib.EngineError):
        ct.emsd(f, 1., 1.)


# ---- the stage path ----
def _msd():
    d = _abi.Msd()
    d.ndim, d.max_lagtime = 2, 3
    d.mpp[0] = d.mpp[1] = 1.
    d.status = d.frame_offset = 64        # never dereferenced: there is no handle
    return d


def _emsd():
    d = _abi.Emsd()
    d.ndim, d.max_lagtime = 3, 1
    d.mpp[0] = d.mpp[1] = d.mpp[2] = 0.5
    d.status = d.frame_offset = d.msd = d.mean_d = d.mean_d2 = d.n = 64
    return d


STAGES = [('ctr_msd_device', _msd), ('ctr_emsd_device', _emsd)]


@pytest.mark.parametrize('call,descriptor', STAGES, ids=[s[0] for s in STAGES])
def test_descriptor_then_handle(call, descriptor):
    lib = _lib.load()
    fn = getattr(lib, call)
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    assert fn(None, None, None) == _abi.ERR_INVALID
    assert msg() == call + ': null descriptor'
    assert fn(None, ctypes.byref(descriptor()), None) == _abi.ERR_INVALID
    assert msg() == call + ': null handle'


BAD = [('ndim', 4, 'ndim'), ('ndim', 1, 'ndim'), ('max_lagtime', 0, 'max_lagtime'), ('max_lagtime', 2 ** 31 - 2, 'too many'),
       ('n_frames', -1, 'negative'), ('n_features', -1, 'negative'), ('n_particles', -1, 'negative'),
       ('n_frames', 2 ** 31 - 2, 'too many'), ('n_features', 2 ** 31, 'too many'), ('n_particles', 2 ** 31 - 1, 'too many'),
       ('status', None, 'null status'), ('frame_offset', None, 'null status'), ('n_features', 1, 'without particle')]


@pytest.mark.parametrize('call,descriptor,field,value,word',
                         [(c, d) + bad for c, d in STAGES for bad in BAD] + [
                             ('ctr_msd_device', _msd, 'n_select', -1, 'negative'),
                             ('ctr_msd_device', _msd, 'n_select', 2 ** 31 - 1, 'too many'),
                             ('ctr_msd_device', _msd, 'n_select', 1, 'null output'),
                             ('ctr_emsd_device', _emsd, 'msd', None, 'null output'),
                             ('ctr_emsd_device', _emsd, 'n', None, 'null output')])
def test_descriptor_is_refused_under_the_entry_point_name(call, descriptor, field, value, word):
    lib = _lib.load()
    d = descriptor()
    setattr(d, field, value)
    assert getattr(lib, call)(None, ctypes.byref(d), None) == _abi.ERR_INVALID
    msg = (lib.ctr_last_error(None) or b'').decode()
    assert msg.startswith(call + ': ') and word in msg


@pytest.mark.parametrize('call,descriptor', STAGES, ids=[s[0] for s in STAGES])
def test_mpp_must_be_finite(call, descriptor):
    lib = _lib.load()
    for axis, value in ((0, float('nan')), (1, float('inf'))):
        d = descriptor()
        d.mpp[axis] = value
        assert getattr(lib, call)(None, ctypes.byref(d), None) == _abi.ERR_INVALID
        assert (lib.ctr_last_error(None) or b'').decode() == call + ': mpp must be finite'


STRUCTS = {'ctr_msd': _abi.Msd, 'ctr_emsd': _abi.Emsd}


def test_prototypes_signatures_constants_and_abi():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    assert _lib.load().ctr_abi_version() == 8
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', header))
    assert set(protos) == set(_lib.SIGNATURES)
    for desc, cls in STRUCTS.items():
        name = desc + '_device'
        params = [p.strip() for p in protos[name].split(',')]
        assert params == ['ctr_handle* h', 'const %s* d' % desc, 'void* hip_stream']
        assert _lib.SIGNATURES[name] == _lib._stage(cls) and name in _lib.EXPORTS
        assert hasattr(_lib.load(), name) and callable(getattr(_lib.Engine, name[len('ctr_'):]))
        # the struct of _abi is the header's: the same fields in the same order
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (desc, desc), header, flags=re.S).group(1)
        assert re.findall(r'\b(\w+)(?:\[\w+\])?\s*;', body) == [f[0] for f in cls._fields_]
    defines = dict(re.findall(r'#define\s+(CTR_MSD_\w+)\s+(\d+)', header))
    assert defines == {'CTR_MSD_OK': '0', 'CTR_MSD_BAD_TABLE': '1', 'CTR_MSD_TILE': str(_abi.MSD_TILE),
                       'CTR_MSD_CHUNK': str(_abi.MSD_CHUNK)}
    assert (_abi.MSD_OK, _abi.MSD_BAD_TABLE) == (0, 1) and _abi.MSD_TILE >= 256 and _abi.MSD_CHUNK >= 1


def test_struct_layout_matches_the_compiler(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    expect = []
    for name, cls in STRUCTS.items():
        src += 'printf("%%zu\\n", sizeof(%s));\n' % name
        expect.append(ctypes.sizeof(cls))
        for f, _ in cls._fields_:
            src += 'printf("%%zu\\n", offsetof(%s, %s));\n' % (name, f)
            expect.append(getattr(cls, f).offset)
    src += 'return 0;}\n'
    (tmp_path / 'layout.c').write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == expect


def test_public_names():
    names = {'msd_arrays', 'emsd_arrays', 'imsd', 'emsd'}
    assert names | {'msd'} <= set(ct.__all__) and ct.msd is ms
    for name in names:
        assert getattr(ct, name) is getattr(ms, name)
    assert ms.MSD._fields == ('lagt', 'msd', 'mean_d', 'mean_d2', 'n', 'status') == ms.EMSD._fields
    for fn in (ms.msd_arrays, ms.emsd_arrays, ms.imsd, ms.emsd):
        assert 'trackpy' in fn.__doc__
    assert 'not pinned' in ms.__doc__
