"""Cluster tracks, without a device: the yardstick ``tests/_cluster_tracks.py`` on
hand-written known answers, and the stage path of the two calls -- descriptor before handle, the
header's prototypes against ``_lib.SIGNATURES``, the ABI version, the round bound, the argument
errors and the public names."""
import ctypes
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

import _cases
import _cluster_tracks as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib, _tables

ctmod = sys.modules['clustertracking_amd.cluster_tracks']     # ct.cluster_tracks is the function


@pytest.mark.parametrize('name', sorted(yard.KNOWN))
def test_yardstick_known_answers(name):
    (off, par, clu, pos), cs, mf, (track_of, n_members, present) = yard.known(name)
    res = yard.cluster_tracks(off, par, clu, cs, mf)
    np.testing.assert_array_equal(res.track_of_particle, track_of)
    np.testing.assert_array_equal(res.n_members, n_members)
    assert res.n_tracks == len(n_members)
    out, pres = yard.track_positions(pos, off, par, res.track_of_particle, res.n_tracks, cs)
    np.testing.assert_array_equal(pres, present)
    np.testing.assert_array_equal(np.isnan(out).all(axis=(2, 3)), present != cs)
    assert not np.isnan(out[present == cs]).any()


def test_yardstick_order_inside_a_cell():
    """ascending (particle, row), whatever the order of the rows and their cluster values"""
    off, par, clu, pos = yard.table([[(1, 0, (10., 11.)), (0, 0, (20., 21.))],
                                     [(1, 3, (30., 31.)), (0, 4, (40., 41.))]])
    res = yard.cluster_tracks(off, par, clu, 2)
    out, present = yard.track_positions(pos, off, par, res.track_of_particle, res.n_tracks, 2)
    np.testing.assert_array_equal(out, [[[[20., 21.], [10., 11.]], [[40., 41.], [30., 31.]]]])
    np.testing.assert_array_equal(present, [[2, 2]])


@pytest.mark.parametrize('cs,mf,seed', [(2, 1, 0), (2, 3, 1), (3, 1, 2), (4, 2, 3)])
def test_vectorised_form_equals_the_loops(cs, mf, seed):
    """the host baseline of tools/cluster_tracks_time.py computes the same rule"""
    off, par, clu, pos = yard.random_video(seed, n_frames=12, n_clusters=9, cluster_size=cs, ndim=3, extra=2)
    res = yard.cluster_tracks(off, par, clu, cs, mf)
    out, present = yard.track_positions(pos, off, par, res.track_of_particle, res.n_tracks, cs)
    track_of, n_tracks, out_v, present_v = yard.tracks_vectorised(off, par, clu, pos, cs, mf)
    assert res.n_tracks == n_tracks and n_tracks > 0
    np.testing.assert_array_equal(track_of, res.track_of_particle)
    np.testing.assert_array_equal(present_v, present)
    np.testing.assert_array_equal(out_v, out)


def test_random_video_has_every_kind_of_cell():
    off, par, clu, pos = yard.random_video(5)
    res = yard.cluster_tracks(off, par, clu, 2)
    _, present = yard.track_positions(pos, off, par, res.track_of_particle, res.n_tracks, 2)
    assert (present == 2).any() and (present > 2).any() and ((present > 0) & (present < 2)).any()
    assert (res.n_members > 2).any() and (par < 0).any() and (clu < 0).any()


# ---- the stage path ----
def _pairs():
    return ctmod.descriptor(_abi.TRACKS_PAIRS, 2, 1, 0, 0, 0)


def _components():
    return ctmod.descriptor(_abi.TRACKS_COMPONENTS, 3, 2, 0, 0, 0)


def _positions():
    d = _abi.TrackPositions()
    d.ndim, d.cluster_size = 2, 2
    d.status = d.frame_offset = 64        # never dereferenced: there is no handle
    return d


def _with_pointers(d):
    d.status = d.frame_offset = d.n_tracks = 64      # never dereferenced: there is no handle
    return d


STAGES = [('ctr_cluster_tracks_device', lambda: _with_pointers(_pairs())),
          ('ctr_cluster_tracks_device', lambda: _with_pointers(_components())),
          ('ctr_track_positions_device', _positions)]


@pytest.mark.parametrize('call,descriptor', STAGES, ids=['pairs', 'components', 'positions'])
def test_descriptor_then_handle(call, descriptor):
    lib = _lib.load()
    fn = getattr(lib, call)
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    assert fn(None, None, None) == _abi.ERR_INVALID
    assert msg().startswith(call + ': ') and msg() != call + ': null handle'
    assert fn(None, ctypes.byref(descriptor()), None) == _abi.ERR_INVALID
    assert msg() == call + ': null handle'


@pytest.mark.parametrize('field,value,word', [('cluster_size', 1, 'cluster_size'), ('cluster_size', 5, 'cluster_size'),
                                              ('min_frames', 0, 'min_frames'), ('phase', 2, 'phase'),
                                              ('check_every', -1, 'check_every'), ('n_particles', -1, 'negative'),
                                              ('n_particles', 2 ** 31 - 1, 'too many')])
def test_descriptor_is_refused_under_the_entry_point_name(field, value, word):
    lib = _lib.load()
    d = _with_pointers(_components())
    setattr(d, field, value)
    assert lib.ctr_cluster_tracks_device(None, ctypes.byref(d), None) == _abi.ERR_INVALID
    msg = (lib.ctr_last_error(None) or b'').decode()
    assert msg.startswith('ctr_cluster_tracks_device: ') and word in msg
    p = _positions()
    p.ndim = 4
    assert lib.ctr_track_positions_device(None, ctypes.byref(p), None) == _abi.ERR_INVALID
    assert (lib.ctr_last_error(None) or b'').decode() == 'ctr_track_positions_device: ndim must be 2 or 3'
    p = _positions()
    p.n_particles, p.n_tracks = 3, 2
    assert lib.ctr_track_positions_device(None, ctypes.byref(p), None) == _abi.ERR_INVALID


def test_prototypes_signatures_and_abi():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    assert _lib.load().ctr_abi_version() == 8
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', header))
    assert set(protos) == set(_lib.SIGNATURES)
    for name, desc in (('ctr_cluster_tracks_device', 'ctr_cluster_tracks'), ('ctr_track_positions_device', 'ctr_track_positions')):
        params = [p.strip() for p in protos[name].split(',')]
        assert len(params) == 3 == len(_lib.SIGNATURES[name][1])
        assert params[0] == 'ctr_handle* h' and params[1].startswith('const %s*' % desc) and params[2] == 'void* hip_stream'
        assert _lib.SIGNATURES[name] == _lib._stage(getattr(_abi, {'ctr_cluster_tracks': 'ClusterTracks',
                                                                   'ctr_track_positions': 'TrackPositions'}[desc]))
    assert len(protos['ctr_cluster_tracks_plan'].split(',')) == 4 == len(_lib.SIGNATURES['ctr_cluster_tracks_plan'][1])
    assert {'ctr_cluster_tracks_device', 'ctr_cluster_tracks_plan', 'ctr_track_positions_device'} <= set(_lib.EXPORTS)
    for name in ('cluster_tracks_device', 'track_positions_device'):
        assert callable(getattr(_lib.Engine, name))
    # the structs of _abi are the header's: the same fields in the same order
    for struct, cls in (('ctr_cluster_tracks', _abi.ClusterTracks), ('ctr_track_positions', _abi.TrackPositions)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), header, flags=re.S).group(1)
        fields = re.findall(r'\b(\w+)\s*;', body)
        assert fields == [f[0] for f in cls._fields_]
    assert (_abi.TRACKS_PAIRS, _abi.TRACKS_COMPONENTS) == (0, 1)
    assert (_abi.TRACKS_OK, _abi.TRACKS_BAD_TABLE, _abi.TRACKS_ROUNDS) == (0, 1, 2)
    assert re.search(r'#define\s+CTR_TRACKS_NO_KEY\s+0x7fffffffffffffffLL', header) and _abi.TRACKS_NO_KEY == 2 ** 63 - 1


@pytest.mark.parametrize('P,log2', [(0, 0), (1, 0), (2, 1), (63, 6), (64, 6), (65, 7), (4097, 13), (2 ** 31 - 2, 31)])
def test_round_bound_is_logarithmic(P, log2):
    """R = 2 ceil(log2 P) + 2 rounds of one hook and J = ceil(log2 P) + 1 jumps (no device needed)"""
    assert ctmod.round_bound(P) == (2 * log2 + 2, log2 + 1)
    scratch = _lib.cluster_tracks_plan(ctmod.descriptor(_abi.TRACKS_COMPONENTS, 2, 1, 0, 0, P))[0]
    assert 16 * P <= scratch <= 16 * P + 4 * (P // 256 + 2) + 4 * (2 * log2 + 2) * (log2 + 2) + 6 * 256
    with pytest.raises(ValueError, match='too many'):
        ctmod.round_bound(2 ** 31 - 1)


def test_value_errors_before_the_engine(monkeypatch):
    def no_engine(device=0):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    off, par, clu, pos = yard.table([[(0, 0), (1, 0)]])
    for cs in (1, 5, 2.5, True):
        with pytest.raises(ValueError, match='cluster_size'):
            ct.cluster_tracks_arrays(off, par, clu, cs)
        with pytest.raises(ValueError, match='cluster_size'):
            ct.track_positions_arrays(pos, off, par, np.zeros(2, np.int32), 1, cs)
    for mf in (0, -1, 1.5):
        with pytest.raises(ValueError, match='min_frames'):
            ct.cluster_tracks_arrays(off, par, clu, 2, min_frames=mf)
    with pytest.raises(ValueError, match='cluster'):
        ct.cluster_tracks_arrays(off, par, clu[:1], 2)
    with pytest.raises(ValueError, match='particle'):
        ct.cluster_tracks_arrays(off, par.reshape(1, 2), clu, 2)
    with pytest.raises(ValueError, match='integers'):
        ct.cluster_tracks_arrays(off, par.astype(float), clu, 2)
    with pytest.raises(ValueError, match='frame_offset'):
        ct.cluster_tracks_arrays(off[:0], par, clu, 2)
    with pytest.raises(ValueError, match='check_every'):
        ct.cluster_tracks_arrays(off, par, clu, 2, check_every=-1)
    with pytest.raises(ValueError, match='pos must be'):
        ct.track_positions_arrays(pos[:, :1], off, par, np.zeros(2, np.int32), 1, 2)
    with pytest.raises(ValueError, match='particle'):
        ct.track_positions_arrays(pos, off, par[:1], np.zeros(2, np.int32), 1, 2)
    with pytest.raises(ValueError, match='n_tracks'):
        ct.track_positions_arrays(pos, off, par, np.zeros(2, np.int32), 2, 2)
    # the rules of the shared front-end (_tables), as drift and msd have them
    for P in (True, -1, 1.5):
        with pytest.raises(ValueError, match='n_particles must be an integer >= 0'):
            ct.cluster_tracks_arrays(off, par, clu, 2, n_particles=P)
    with pytest.raises(ValueError, match=r'more than 2\^31 - 2 particles'):
        ct.cluster_tracks_arrays(off, par, clu, 2, n_particles=2 ** 31 - 1)
    for bad in (pos > 0, pos.astype(str)):
        with pytest.raises(ValueError, match='pos must hold numbers, not '):
            ct.track_positions_arrays(bad, off, par, np.zeros(2, np.int32), 1, 2)
    import torch
    assert _tables.count_particles(torch.tensor([0, 2 ** 31 - 3]), 2) == 2 ** 31 - 2
    with pytest.raises(ValueError, match=r'more than 2\^31 - 2 particles'):       # an id read from a tensor
        _tables.count_particles(torch.tensor([0, 2 ** 31 - 2]), 2)
    f = pd.DataFrame({'frame': [0, 0], 'y': [1., 2.], 'x': [3., 4.], 'cluster': [0, 0], 'particle': [0, 1]})
    for fn in (ct.cluster_tracks, ct.track_positions):
        with pytest.raises(ValueError, match="'particle'"):
            fn(f.drop(columns='particle'), 2)
        with pytest.raises(ValueError, match="'cluster'"):
            fn(f.drop(columns='cluster'), 2)
        with pytest.raises(ValueError, match='cluster_size'):
            fn(f, 7)
        with pytest.raises(ValueError, match='min_frames'):
            fn(f, 2, min_frames=0)
        with pytest.raises(ValueError, match='pos_columns'):
            fn(f, 2, pos_columns=['y', 'q'])
        with pytest.raises(ValueError, match='empty'):
            fn(f.iloc[:0], 2)
        with pytest.raises(ValueError, match='integers'):
            fn(f.assign(particle=[0.5, 1.]), 2)


def test_public_names():
    names = {'cluster_tracks', 'cluster_tracks_arrays', 'track_positions', 'track_positions_arrays'}
    assert names <= set(ct.__all__)
    for name in names:
        assert getattr(ct, name) is getattr(ctmod, name)
    assert ctmod.ClusterTracks._fields == ('track_of_particle', 'n_tracks', 'n_members', 'status')
    assert ctmod.TrackPositions._fields == ('pos', 'present')
