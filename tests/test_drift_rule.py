"""Drift of a linked video, without a device: the yardstick ``tests/_drift.py`` on
known answers worked by hand, the argument errors of the six functions, and the stage path of the
three calls -- descriptor before handle, the header's prototypes and structs against ``_lib`` and
``_abi``, the ABI version and the public names."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest

import _cases
import _drift as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib
from clustertracking_amd import drift as dr


# ---- the yardstick on hand-worked tables ----
def test_uniform_drift():
    pos, off, par = yard.table([[(0, (1., 2.)), (1, (5., 6.))],
                                [(1, (6., 6.5)), (0, (2., 2.5))],
                                [(0, (3., 3.)), (1, (7., 7.))]])
    res = yard.compute_drift(pos, off, par)
    np.testing.assert_array_equal(res.n_pairs, [0, 2, 2])
    np.testing.assert_array_equal(res.drift, [[0., 0.], [1., 0.5], [2., 1.]])
    np.testing.assert_array_equal(yard.subtract_drift(pos, off, res.drift),
                                  [[1., 2.], [5., 6.], [5., 6.], [1., 2.], [1., 2.], [5., 6.]])


def test_a_particle_that_skips_a_frame():
    """particle 1 is absent in frame 1: it forms no pair in frame 1 and none in frame 2"""
    pos, off, par = yard.table([[(0, (0., 0.)), (1, (10., 10.))],
                                [(0, (1., 2.))],
                                [(0, (3., 3.)), (1, (50., 50.))]])
    res = yard.compute_drift(pos, off, par)
    np.testing.assert_array_equal(res.n_pairs, [0, 1, 1])
    np.testing.assert_array_equal(res.drift, [[0., 0.], [1., 2.], [3., 3.]])
    assert res.pairs == [(1, 2, 0), (2, 3, 2)]


def test_an_unlinked_row():
    """rows with a negative id pair with nothing, not even with each other"""
    pos, off, par = yard.table([[(-1, (0., 0.)), (0, (4., 4.))],
                                [(0, (4., 6.)), (-1, (100., 100.))]])
    res = yard.compute_drift(pos, off, par)
    np.testing.assert_array_equal(res.n_pairs, [0, 1])
    np.testing.assert_array_equal(res.drift, [[0., 0.], [0., 2.]])


def test_a_frame_without_pairs_carries_the_drift():
    pos, off, par = yard.table([[(0, (0., 0.))], [(0, (1., 0.))], [(1, (7., 7.))], [(1, (10., 7.))]])
    res = yard.compute_drift(pos, off, par)
    np.testing.assert_array_equal(res.n_pairs, [0, 1, 0, 1])
    np.testing.assert_array_equal(res.drift[:, 0], [0., 1., 1., 4.])
    # a window of two frames: frame 2 takes dx[1], frame 3 dx[3] alone (frame 2 has no pair)
    np.testing.assert_array_equal(yard.compute_drift(pos, off, par, 2).drift[:, 0], [0., 1., 2., 5.])
    # an empty frame in the middle
    pos, off, par = yard.table([[(0, (0., 0.))], [(0, (1., 0.))], [], [(0, (5., 0.))], [(0, (7., 0.))]])
    res = yard.compute_drift(pos, off, par)
    np.testing.assert_array_equal(res.n_pairs, [0, 1, 0, 0, 1])
    np.testing.assert_array_equal(res.drift[:, 0], [0., 1., 1., 1., 3.])


@pytest.mark.parametrize('smoothing,want', [(0, [0., 1., 3., 6., 10.]), (1, [0., 1., 3., 6., 10.]),
                                            (3, [0., 1., 2.5, 4.5, 7.5]), (7, [0., 1., 2.5, 4.5, 7.])])
def test_smoothing(smoothing, want):
    """dx = 1, 2, 3, 4: the mean over the last s frames from frame 1 on, then the running sum"""
    x = np.cumsum([0., 1., 2., 3., 4.])
    pos, off, par = yard.table([[(0, (0., v))] for v in x])
    res = yard.compute_drift(pos, off, par, smoothing)
    np.testing.assert_array_equal(res.dx[:, 1], [0., 1., 2., 3., 4.])
    np.testing.assert_array_equal(res.drift[:, 1], want)
    np.testing.assert_array_equal(res.drift[:, 0], 0.)


def test_the_lowest_row_of_a_repeated_id():
    """two rows of frame 0 carry id 0: the lower one is the partner; both rows of frame 1 count"""
    pos, off, par = yard.table([[(1, (9., 9.)), (0, (0., 0.)), (0, (10., 10.))],
                                [(0, (1., 1.)), (0, (3., 5.))]])
    res = yard.compute_drift(pos, off, par)
    assert res.pairs == [(1, 3, 1), (1, 4, 1)]
    np.testing.assert_array_equal(res.n_pairs, [0, 2])
    np.testing.assert_array_equal(res.drift[1], [2., 3.])


def test_stubs():
    res = yard.filter_stubs([0, 1, -1, 0, 2, 0, 1], 2)
    np.testing.assert_array_equal(res.count, [3, 2, 1])
    np.testing.assert_array_equal(res.particle, [0, 1, -1, 0, -1, 0, 1])
    np.testing.assert_array_equal(yard.filter_stubs([0, 1, 0], 3, n_particles=4).count, [2, 1, 0, 0])
    np.testing.assert_array_equal(yard.filter_stubs([0, 1, 0], 3).particle, [-1, -1, -1])


def test_generators_have_what_the_device_tests_need():
    pos, off, par = yard.drifting_video(0)
    res = yard.compute_drift(pos, off, par)
    np.testing.assert_array_equal(res.n_pairs, [0, 5, 5, 4, 4, 5])
    assert (par < 0).sum() == 1 and np.diff(off).tolist() == [5, 5, 6, 4, 5, 5]
    np.testing.assert_allclose(res.drift[-1], 5 * np.array([0.7, -0.4]), atol=0.2)
    assert (yard.bound(res, pos) < 1e-12).all() and (yard.bound(res, pos)[1:] > 0).all()
    pos, off, par = yard.relabelled_video(1)
    np.testing.assert_array_equal(yard.compute_drift(pos, off, par).n_pairs, [0, 4, 4, 0, 4])


# ---- argument errors, before any device work ----
def test_value_errors_before_the_engine(monkeypatch):
    def no_engine(device=0):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    pos, off, par = yard.table([[(0, (0., 0.)), (1, (5., 5.))], [(0, (1., 1.)), (1, (6., 6.))]])
    drift = np.zeros((2, 2))
    for s in (-1, 1.5, True, 2 ** 31):
        with pytest.raises(ValueError, match='smoothing'):
            ct.compute_drift_arrays(pos, off, par, smoothing=s)
    with pytest.raises(ValueError, match='pos must be'):
        ct.compute_drift_arrays(pos[:, :1], off, par)
    with pytest.raises(ValueError, match='pos must be'):
        ct.compute_drift_arrays(pos.reshape(-1), off, par)
    with pytest.raises(ValueError, match='numbers'):
        ct.compute_drift_arrays(pos.astype(str), off, par)
    with pytest.raises(ValueError, match='particle'):
        ct.compute_drift_arrays(pos, off, par[:3])
    with pytest.raises(ValueError, match='integers'):
        ct.compute_drift_arrays(pos, off, par.astype(float))
    with pytest.raises(ValueError, match='integers'):
        ct.compute_drift_arrays(pos, off.astype(float), par)
    with pytest.raises(ValueError, match='frame_offset'):
        ct.compute_drift_arrays(pos, off[:0], par)
    with pytest.raises(ValueError, match='frame_offset'):
        ct.compute_drift_arrays(pos, off.reshape(1, -1), par)
    for P in (-1, 1.5, 2 ** 31 - 1):
        with pytest.raises(ValueError, match='particles'):
            ct.compute_drift_arrays(pos, off, par, n_particles=P)
        with pytest.raises(ValueError, match='particles'):
            ct.filter_stubs_arrays(par, 2, n_particles=P)
    with pytest.raises(ValueError, match='pos must be'):
        ct.subtract_drift_arrays(pos[:, :1], off, drift)
    with pytest.raises(ValueError, match='drift must be'):
        ct.subtract_drift_arrays(pos, off, drift[:1])
    with pytest.raises(ValueError, match='drift must be'):
        ct.subtract_drift_arrays(pos, off, np.zeros((2, 3)))
    with pytest.raises(ValueError, match='frame_offset'):
        ct.subtract_drift_arrays(pos, off[:0], drift[:0])
    for th in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match='threshold'):
            ct.filter_stubs_arrays(par, threshold=th)
    with pytest.raises(ValueError, match='particle'):
        ct.filter_stubs_arrays(par.reshape(2, 2))
    with pytest.raises(ValueError, match='integers'):
        ct.filter_stubs_arrays(par.astype(float))
    f = pd.DataFrame({'frame': [0, 0, 1, 1], 'y': pos[:, 0], 'x': pos[:, 1], 'particle': par})
    for fn in (ct.compute_drift, ct.subtract_drift, ct.filter_stubs):
        with pytest.raises(ValueError, match="'particle'"):
            fn(f.drop(columns='particle'))
        with pytest.raises(ValueError, match="'frame'"):
            fn(f.drop(columns='frame'))
        with pytest.raises(ValueError, match='empty'):
            fn(f.iloc[:0])
        with pytest.raises(ValueError, match='integers'):
            fn(f.assign(particle=[0.5, 1., 0.5, 1.]))
    for fn in (ct.compute_drift, ct.subtract_drift):
        with pytest.raises(ValueError, match='pos_columns'):
            fn(f, pos_columns=['y', 'q'])
        with pytest.raises(ValueError, match='pos_columns'):
            fn(f, pos_columns=['y'])
        with pytest.raises(ValueError, match='smoothing'):
            fn(f, smoothing=-1)
    with pytest.raises(ValueError, match='threshold'):
        ct.filter_stubs(f, threshold=0)
    with pytest.raises(ValueError, match='cover'):
        ct.subtract_drift(f, drift=pd.DataFrame({'y': [0.], 'x': [0.]}, index=[0]))
    with pytest.raises(ValueError, match='columns'):
        ct.subtract_drift(f, drift=pd.DataFrame({'y': [0., 0.]}, index=[0, 1]))


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    pos, off, par = yard.table([[(0, (0., 0.))], [(0, (1., 1.))]])
    with pytest.raises(_lib.EngineError):
        ct.compute_drift_arrays(pos, off, par)
    with pytest.raises(_lib.EngineError):
        ct.subtract_drift_arrays(pos, off, np.zeros((2, 2)))
    with pytest.raises(_lib.EngineError):
        ct.filter_stubs_arrays(par, 2)


# ---- the stage path ----
def _drift():
    d = _abi.Drift()
    d.ndim = 2
    d.status = d.frame_offset = 64        # never dereferenced: there is no handle
    return d


def _subtract():
    d = _abi.DriftSubtract()
    d.ndim = 3
    d.status = d.frame_offset = 64
    return d


def _stubs():
    d = _abi.FilterStubs()
    d.threshold = 1
    d.status = 64
    return d


STAGES = [('ctr_drift_device', _drift), ('ctr_drift_subtract_device', _subtract), ('ctr_filter_stubs_device', _stubs)]


@pytest.mark.parametrize('call,descriptor', STAGES, ids=[s[0] for s in STAGES])
def test_descriptor_then_handle(call, descriptor):
    lib = _lib.load()
    fn = getattr(lib, call)
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    assert fn(None, None, None) == _abi.ERR_INVALID
    assert msg() == call + ': null descriptor'
    assert fn(None, ctypes.byref(descriptor()), None) == _abi.ERR_INVALID
    assert msg() == call + ': null handle'


@pytest.mark.parametrize('call,descriptor,field,value,word', [
    ('ctr_drift_device', _drift, 'ndim', 4, 'ndim'), ('ctr_drift_device', _drift, 'smoothing', -1, 'smoothing'),
    ('ctr_drift_device', _drift, 'n_frames', -1, 'negative'), ('ctr_drift_device', _drift, 'n_particles', 2 ** 31 - 1, 'too many'),
    ('ctr_drift_device', _drift, 'status', None, 'null status'), ('ctr_drift_device', _drift, 'n_features', 1, 'without particle'),
    ('ctr_drift_device', _drift, 'n_frames', 1, 'null output'),
    ('ctr_drift_subtract_device', _subtract, 'ndim', 1, 'ndim'), ('ctr_drift_subtract_device', _subtract, 'n_features', 1, 'without pos'),
    ('ctr_drift_subtract_device', _subtract, 'n_frames', 1, 'without drift'),
    ('ctr_filter_stubs_device', _stubs, 'threshold', 0, 'threshold'), ('ctr_filter_stubs_device', _stubs, 'n_features', 1, 'without particle'),
    ('ctr_filter_stubs_device', _stubs, 'n_particles', 1, 'without count')])
def test_descriptor_is_refused_under_the_entry_point_name(call, descriptor, field, value, word):
    lib = _lib.load()
    d = descriptor()
    setattr(d, field, value)
    assert getattr(lib, call)(None, ctypes.byref(d), None) == _abi.ERR_INVALID
    msg = (lib.ctr_last_error(None) or b'').decode()
    assert msg.startswith(call + ': ') and word in msg


def test_prototypes_signatures_and_abi():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    assert _lib.load().ctr_abi_version() == 8
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', header))
    structs = {'ctr_drift': _abi.Drift, 'ctr_drift_subtract': _abi.DriftSubtract, 'ctr_filter_stubs': _abi.FilterStubs}
    for desc, cls in structs.items():
        name = desc + '_device'
        params = [p.strip() for p in protos[name].split(',')]
        assert params == ['ctr_handle* h', 'const %s* d' % desc, 'void* hip_stream']
        assert _lib.SIGNATURES[name] == _lib._stage(cls) and name in _lib.EXPORTS
        assert callable(getattr(_lib.Engine, name[len('ctr_'):]))
        # the struct of _abi is the header's: the same fields in the same order
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (desc, desc), header, flags=re.S).group(1)
        assert re.findall(r'\b(\w+)\s*;', body) == [f[0] for f in cls._fields_]
    assert (_abi.DRIFT_OK, _abi.DRIFT_BAD_TABLE) == (0, 1)
    assert re.search(r'#define\s+CTR_DRIFT_BAD_TABLE\s+1\b', header)


def test_struct_layout_matches_the_compiler(tmp_path):
    import subprocess
    structs = {'ctr_drift': _abi.Drift, 'ctr_drift_subtract': _abi.DriftSubtract, 'ctr_filter_stubs': _abi.FilterStubs}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    expect = []
    for name, cls in structs.items():
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
    names = {'compute_drift', 'subtract_drift', 'filter_stubs', 'compute_drift_arrays', 'subtract_drift_arrays',
             'filter_stubs_arrays'}
    assert names | {'drift'} <= set(ct.__all__) and ct.drift is dr
    for name in names:
        assert getattr(ct, name) is getattr(dr, name)
    assert dr.Drift._fields == ('drift', 'n_pairs', 'status') and dr.Stubs._fields == ('particle', 'count')
    for fn in (dr.compute_drift_arrays, dr.subtract_drift_arrays, dr.filter_stubs_arrays, dr.compute_drift,
               dr.subtract_drift, dr.filter_stubs):
        assert 'trackpy' in fn.__doc__
