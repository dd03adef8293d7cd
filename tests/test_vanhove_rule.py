"""Van Hove displacement distributions of linked particles, without a device: the
yardstick ``tests/_vanhove.py`` against an independent brute force over all row pairs and on a known
answer, the argument errors of the two functions, and the stage path of the call -- descriptor before
handle, every refused scalar, the header's prototype, struct and constants against ``_lib`` and
``_abi``, the ABI version and the public names."""
import ctypes
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import _cases
import _msd
import _vanhove as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib

vh = importlib.import_module('clustertracking_amd.vanhove')      # ct.vanhove is the function
CALL = 'ctr_vanhove_device'


# ---- the restatement against the brute force ----
def _gap_2d():
    """particle 0 misses frames 2 and 3, particle 1 has one row, particle 3 has no row at all"""
    return _msd.table([[(0, (1., 2.)), (1, (9., 9.)), (2, (4., 4.))],
                       [(2, (4.5, 3.)), (0, (1.25, 2.5))],
                       [(2, (5.5, 3.25))],
                       [(2, (5.75, 2.))],
                       [(0, (3., 1.)), (2, (7., 2.5)), (4, (0., 0.))],
                       [(4, (0.5, 0.25)), (0, (3.5, 1.75))]])


def _repeated_and_unlinked_3d():
    """id 0 twice in frame 1 (the lowest row wins) and twice in frame 3; unlinked rows"""
    return _msd.table([[(0, (0., 0., 0.)), (-1, (5., 5., 5.)), (1, (2., 2., 2.))],
                       [(0, (1., 0.5, 0.25)), (0, (30., 30., 30.)), (1, (2.5, 2., 1.)), (-1, (6., 5., 5.))],
                       [(1, (3., 3., 3.)), (0, (1.5, 1., 1.)), (-7, (7., 7., 7.))],
                       [(0, (2.25, 2., 1.5)), (1, (3.5, 3.25, 3.)), (0, (-40., 0., 0.)), (-7, (8., 7., 7.))]], ndim=3)


# name: (table, mpp, lags, bin_width, max_disp): the reach is short enough that both tails are met
BRUTE = {'gap_2d': (_gap_2d, 1., [1, 2, 4, 7], 0.3, 1.2), 'repeated_3d': (_repeated_and_unlinked_3d, (0.5, 1., 2.), [1, 3, 5], 0.25, 1.)}


@pytest.mark.parametrize('name', sorted(BRUTE))
def test_restatement_equals_the_brute_force(name):
    make, mpp, lags, width, reach = BRUTE[name]
    pos, off, par = make()
    assert len(pos) <= 40
    ndim = pos.shape[1]
    got = yard.vanhove(pos, off, par, lags, width, reach, mpp)
    want = yard.brute_force(pos, off, par, lags, width, reach, mpp)
    half = len(got.r_edges) - 1
    assert got.count.shape == (len(lags), ndim, 2 * half) and got.count_r.shape == (len(lags), half) and half == 4
    assert got.edges[half] == 0. and (got.edges == -got.edges[::-1]).all()
    for q, k in enumerate(lags):
        count, below, above, count_r, above_r, n, s1, s2, s4 = want[k]
        assert got.n[q] == n and (got.count[q] == count).all() and (got.below[q] == below).all() and (got.above[q] == above).all()
        assert (got.count_r[q] == count_r).all() and got.above_r[q] == above_r
        assert (got.count[q].sum(-1) + got.below[q] + got.above[q] == n).all() and got.count_r[q].sum() + got.above_r[q] == n
        if n == 0:
            for name_ in yard.FLOATS:
                assert np.isnan(getattr(got, name_)[q]).all()
            continue
        for a in range(ndim):
            assert got.mean_d[q, a] == math.fsum(s1[a]) / n and got.mean_d2[q, a] == math.fsum(s2[a]) / n
            assert got.mean_d4[q, a] == math.fsum(s4[a]) / n
        assert (got.density[q] == count / (n * width)).all() and (got.density_r[q] == count_r / (n * width)).all()
    assert got.n[-1] == 0 and got.n[0] > 0                       # a lag beyond every span
    assert got.below.sum() > 0 and got.above.sum() > 0 and got.above_r.sum() > 0 and got.count.sum() > 0


@pytest.mark.parametrize('ndim', [2, 3])
def test_uniform_motion_is_a_delta(ndim):
    """x0 + v t: every pair of lag k is in the bin of k v, and m4 = m2^2 gives alpha2 = 1/3 - 1, the -2/3 of
    a delta distribution as clause 9 rounds it"""
    v = np.array([1.5, -0.75, 0.25])[:ndim]
    x0 = np.array([[10., 20., 30.], [-4., 7., 0.5]])[:, :ndim]
    frames = [[(p, tuple(x0[p] + v * t)) for p in range(2) if (p, t) != (1, 3)] for t in range(7)]
    pos, off, par = _msd.table(frames, ndim)
    lags = [1, 2, 4]
    got = yard.vanhove(pos, off, par, lags, 0.5, 8.)
    half = 16
    assert got.n.tolist() == [10, 8, 6]
    for q, k in enumerate(lags):
        for a in range(ndim):
            b = int(np.floor(k * v[a] / 0.5)) + half
            assert got.count[q, a, b] == got.n[q] and got.count[q, a].sum() == got.n[q]
            assert got.mean_d[q, a] == k * v[a] and got.mean_d2[q, a] == (k * v[a]) ** 2 and got.mean_d4[q, a] == (k * v[a]) ** 4
            # clause 9 rounds every operation: m4 / (3 m2^2) is rn(1/3) and alpha2 is rn(1/3) - 1 exactly,
            # the double above rn(-2/3) (the exact difference lies halfway between the two)
            assert got.alpha2[q, a] == 1. / 3. - 1. == np.nextafter(-2. / 3., -1.)
        r = k * np.sqrt((v ** 2).sum())
        assert got.count_r[q, int(r / 0.5)] == got.n[q] and got.above_r[q] == 0
    assert not got.below.any() and not got.above.any()


def test_edges_and_nan_in_the_restatement():
    """a displacement on an edge belongs to the bin above it, -0.0 to bin H, a NaN nowhere"""
    width, reach = 0.1, 0.3
    half, edges, r_edges, edge2 = yard.bins(width, reach)
    assert half == 3 and edges[3] == 0. and edges[4] == 0.1 and edges[5] == 0.2 and edges[6] == 0.1 * 3 != 0.3
    ds = [edges[0], edges[4], edges[6], np.nextafter(edges[4], -1.), -0., np.nan, np.nextafter(edges[0], -1.)]
    frames = [[(p, (0., 0.)) for p in range(len(ds))], [(p, (d, 0.)) for p, d in enumerate(ds)]]
    pos, off, par = _msd.table(frames)
    got = yard.vanhove(pos, off, par, [1], width, reach)
    assert got.n[0] == len(ds) and got.count[0, 0].tolist() == [1, 0, 0, 2, 1, 0] and got.below[0, 0] == 1 and got.above[0, 0] == 1
    assert got.count[0, 0].sum() + got.below[0, 0] + got.above[0, 0] == got.n[0] - 1       # the NaN
    assert got.count_r[0].sum() + got.above_r[0] == got.n[0] - 1 and np.isnan(got.mean_d[0, 0]) and got.mean_d[0, 1] == 0.


# ---- argument errors, before any device work ----
def test_value_errors_before_the_engine(monkeypatch):
    def no_engine(device=0):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    pos, off, par = _msd.table([[(0, (0., 0.)), (1, (5., 5.))], [(0, (1., 1.)), (1, (6., 6.))]])
    fn = ct.vanhove_arrays
    for lag in (0, -1, 1.5, True, 2 ** 31 - 2, [], [2, 1], [1, 1], [1, 0], [[1, 2]], list(range(1, 66)), None, 'a'):
        with pytest.raises(ValueError, match='lagtime'):
            fn(pos, off, par, lag, 0.1, 1.)
    for width in (0, -0.1, np.nan, np.inf, True, 'w'):
        with pytest.raises(ValueError, match='bin_width'):
            fn(pos, off, par, 1, width, 1.)
    for reach in (0, -1., np.nan, np.inf, None):
        with pytest.raises(ValueError, match='max_disp'):
            fn(pos, off, par, 1, 0.1, reach)
    with pytest.raises(ValueError, match='more than 1024'):
        fn(pos, off, par, 1, 0.001, 1.0251)
    with pytest.raises(ValueError, match='pos must be'):
        fn(pos[:, :1], off, par, 1, 0.1, 1.)
    with pytest.raises(ValueError, match='pos must be'):
        fn(pos.reshape(-1), off, par, 1, 0.1, 1.)
    with pytest.raises(ValueError, match='particle'):
        fn(pos, off, par[:3], 1, 0.1, 1.)
    with pytest.raises(ValueError, match='integers'):
        fn(pos, off, par.astype(float), 1, 0.1, 1.)
    with pytest.raises(ValueError, match='frame_offset'):
        fn(pos, off[:0], par, 1, 0.1, 1.)
    for mpp in ((1., 2., 3.), (1.,), np.nan, [[1., 1.]], (1., np.inf)):
        with pytest.raises(ValueError, match='mpp'):
            fn(pos, off, par, 1, 0.1, 1., mpp=mpp)
    for P in (-1, 1.5, 2 ** 31 - 1):
        with pytest.raises(ValueError, match='particles'):
            fn(pos, off, par, 1, 0.1, 1., n_particles=P)
    f = pd.DataFrame({'frame': [0, 0, 1, 1], 'y': pos[:, 0], 'x': pos[:, 1], 'particle': par})
    with pytest.raises(ValueError, match="'particle'"):
        ct.vanhove(f.drop(columns='particle'), 1, 1., 0.1, 1.)
    with pytest.raises(ValueError, match="'frame'"):
        ct.vanhove(f.drop(columns='frame'), 1, 1., 0.1, 1.)
    with pytest.raises(ValueError, match='empty'):
        ct.vanhove(f.iloc[:0], 1, 1., 0.1, 1.)
    with pytest.raises(ValueError, match='pos_columns'):
        ct.vanhove(f, 1, 1., 0.1, 1., pos_columns=['y', 'q'])
    for lag in (0, [1, 2], [1]):
        with pytest.raises(ValueError, match='lagtime'):
            ct.vanhove(f, lag, 1., 0.1, 1.)
    with pytest.raises(ValueError, match='mpp'):
        ct.vanhove(f, 1, (1., 2., 3.), 0.1, 1.)
    with pytest.raises(ValueError, match='bin_width'):
        ct.vanhove(f, 1, 1., 0., 1.)
    with pytest.raises(ValueError, match='max_disp'):
        ct.vanhove(f, 1, 1., 0.1, -1.)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    pos, off, par = _msd.table([[(0, (0., 0.))], [(0, (1., 1.))]])
    with pytest.raises(_lib.EngineError):
        ct.vanhove_arrays(pos, off, par, 1, 0.1, 1.)
    f = pd.DataFrame({'frame': [0, 1], 'y': [0., 1.], 'x': [0., 1.], 'particle': [0, 0]})
    with pytest.raises(_lib.EngineError):
        ct.vanhove(f, 1, 1., 0.1, 1.)
    with pytest.raises(_lib.EngineError):
        ct.vanhove(f, 1, 1., 0.1, 1., radial=True)


# ---- the stage path ----
POINTERS = [f for f, t in _abi.Vanhove._fields_ if t is ctypes.c_void_p]


def _descriptor():
    d = _abi.Vanhove()
    d.ndim, d.n_lags, d.half_bins, d.bin_width = 2, 2, 8, 0.1
    d.lag[0], d.lag[1] = 1, 3
    d.mpp[0] = d.mpp[1] = 1.
    for f in POINTERS:
        if f not in ('pos', 'particle', 'order'):
            setattr(d, f, 64)                 # never dereferenced: there is no handle
    return d


def _refused(d):
    lib = _lib.load()
    assert getattr(lib, CALL)(None, ctypes.byref(d), None) == _abi.ERR_INVALID
    msg = (lib.ctr_last_error(None) or b'').decode()
    assert msg.startswith(CALL + ': ')
    return msg[len(CALL) + 2:]


def test_descriptor_then_handle():
    lib = _lib.load()
    fn = getattr(lib, CALL)
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    assert fn(None, None, None) == _abi.ERR_INVALID
    assert msg() == CALL + ': null descriptor'
    assert fn(None, ctypes.byref(_descriptor()), None) == _abi.ERR_INVALID
    assert msg() == CALL + ': null handle'
    d = _descriptor()                          # the largest descriptor the launch takes
    d.n_lags, d.half_bins, d.ndim = 64, 1024, 3
    d.mpp[2] = 2.
    for q in range(64):
        d.lag[q] = q + 1
    d.lag[63] = 2 ** 31 - 3
    assert fn(None, ctypes.byref(d), None) == _abi.ERR_INVALID and msg() == CALL + ': null handle'


BAD = [('ndim', 1, 'ndim'), ('ndim', 4, 'ndim'), ('n_lags', 0, 'n_lags'), ('n_lags', 65, 'n_lags'),
       ('half_bins', 0, 'half_bins'), ('half_bins', 1025, 'half_bins'),
       ('bin_width', 0., 'bin_width'), ('bin_width', float('nan'), 'bin_width'), ('bin_width', float('inf'), 'bin_width'),
       ('bin_width', -0.1, 'bin_width'),
       ('n_frames', -1, 'negative'), ('n_features', -1, 'negative'), ('n_particles', -1, 'negative'),
       ('n_frames', 2 ** 31 - 2, 'too many'), ('n_features', 2 ** 31, 'too many'), ('n_particles', 2 ** 31 - 1, 'too many'),
       ('status', None, 'null status'), ('frame_offset', None, 'null status'), ('n_features', 1, 'without particle'),
       ('edges', None, 'null edges'), ('edge2', None, 'null edges')] + \
      [(f, None, 'null output') for f in POINTERS if f not in ('pos', 'frame_offset', 'particle', 'order', 'edges', 'edge2', 'status')]


@pytest.mark.parametrize('field,value,word', BAD, ids=['%s=%r' % b[:2] for b in BAD])
def test_descriptor_is_refused_under_the_entry_point_name(field, value, word):
    d = _descriptor()
    setattr(d, field, value)
    assert word in _refused(d)


@pytest.mark.parametrize('lags', [(0, 3), (3, 1), (2, 2), (1, 2 ** 31 - 2), (-1, 1)], ids=str)
def test_lags_are_checked_by_the_launch(lags):
    d = _descriptor()
    d.lag[0], d.lag[1] = lags
    assert 'lags must be ascending' in _refused(d)
    d.n_lags = 1                               # only the first K are looked at
    if 1 <= lags[0] <= 2 ** 31 - 3:
        assert _refused(d) == 'null handle'


def test_mpp_must_be_finite():
    for axis, value in ((0, float('nan')), (1, float('inf'))):
        d = _descriptor()
        d.mpp[axis] = value
        assert _refused(d) == 'mpp must be finite'
    d = _descriptor()
    d.mpp[2] = float('nan')                    # beyond ndim: not looked at
    assert _refused(d) == 'null handle'


def test_prototype_signature_constants_and_abi():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    assert _lib.load().ctr_abi_version() == 8
    for clause in ('below[k, a]', 'above_r[k]', 'alpha2[k, a] = mean_d4 / (3 * (mean_d2 * mean_d2)) - 1', 'Against trackpy'):
        assert clause in header, clause
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', header))
    assert set(protos) == set(_lib.SIGNATURES)
    assert [p.strip() for p in protos[CALL].split(',')] == ['ctr_handle* h', 'const ctr_vanhove* d', 'void* hip_stream']
    assert _lib.SIGNATURES[CALL] == _lib._stage(_abi.Vanhove) and CALL in _lib.EXPORTS
    assert hasattr(_lib.load(), CALL) and callable(_lib.Engine.vanhove_device)
    body = re.search(r'typedef struct ctr_vanhove \{(.*?)\} ctr_vanhove;', header, flags=re.S).group(1)
    assert re.findall(r'\b(\w+)(?:\[\w+\])?\s*;', body) == [f[0] for f in _abi.Vanhove._fields_]
    defines = dict(re.findall(r'#define\s+(CTR_VANHOVE_\w+)\s+(\d+)', header))
    assert defines == {'CTR_VANHOVE_OK': '0', 'CTR_VANHOVE_BAD_TABLE': '1', 'CTR_VANHOVE_MAX_LAGS': '64',
                       'CTR_VANHOVE_MAX_HALF_BINS': '1024'}
    assert (_abi.VANHOVE_OK, _abi.VANHOVE_BAD_TABLE, _abi.VANHOVE_MAX_LAGS, _abi.VANHOVE_MAX_HALF_BINS) == (0, 1, 64, 1024)
    assert (_abi.VANHOVE_OK, _abi.VANHOVE_BAD_TABLE) == (_abi.MSD_OK, _abi.MSD_BAD_TABLE)     # the check kernel is the MSD's


def test_struct_layout_matches_the_compiler(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_vanhove));\n'
    expect = [ctypes.sizeof(_abi.Vanhove)]
    for f, _ in _abi.Vanhove._fields_:
        src += 'printf("%%zu\\n", offsetof(ctr_vanhove, %s));\n' % f
        expect.append(getattr(_abi.Vanhove, f).offset)
    src += 'return 0;}\n'
    (tmp_path / 'layout.c').write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == expect


def test_public_names():
    assert {'vanhove_arrays', 'vanhove'} <= set(ct.__all__)
    assert ct.vanhove is vh.vanhove and ct.vanhove_arrays is vh.vanhove_arrays
    assert vh.VanHove._fields == ('lags', 'edges', 'r_edges', 'count', 'below', 'above', 'density', 'count_r', 'above_r',
                                  'density_r', 'n', 'mean_d', 'mean_d2', 'mean_d4', 'alpha2', 'status')
    for fn in (vh.vanhove_arrays, vh.vanhove):
        assert 'trackpy' in fn.__doc__
    for words in ('not pinned', 'tails are counted', 'ensemble only', 'Several lags'.lower(), 'a width and a reach'):
        assert words in vh.__doc__, words
    # the module is built on _tables alone: no private name of another stage module
    source = open(vh.__file__).read()
    assert not re.search(r'from \.(msd|drift|static|motion)\b|import (msd|drift|static)\b', source)
