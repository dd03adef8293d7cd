"""Nearest neighbours and proximity, without a device: the yardstick
``tests/_neighbors.py`` against ``scipy.spatial.cKDTree.query`` and on hand cases, the argument errors
of the three calls, and the stage path of the call -- descriptor before handle, the header's prototype,
struct and constants against ``_lib`` and ``_abi``, the ABI version and the public names."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import _cases
import _neighbors as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib
from clustertracking_amd import static as st


# ---- the restatement on known answers ----
@pytest.mark.parametrize('ndim', [2, 3])
@pytest.mark.parametrize('rows', [5, 300, 700])
def test_restatement_agrees_with_ckdtree(ndim, rows):
    """tie-free random tables, one frame, k = 4: the indices are equal, the distances agree within
    4 x 2^-52 relative (cKDTree may add the squares in another order)"""
    from scipy.spatial import cKDTree
    pos, off = yard.uniform_frames(100 * ndim + rows, (rows,), (80., 60., 40.)[:ndim], ndim)
    res = yard.neighbors(pos, off, k=4)
    dist, index = cKDTree(pos).query(pos, k=5)
    assert (index[:, 0] == np.arange(rows)).all()                       # the row itself, which the rule excludes
    assert (res.index == index[:, 1:]).all() and (res.count == rows - 1).all()
    rel = np.abs(res.dist - dist[:, 1:]) / dist[:, 1:]
    print('largest relative difference to cKDTree', rel.max())
    assert (rel <= 4 * 2. ** -52).all()
    yard.assert_equal_bits(res.dist, np.sqrt(res.dist2))


def test_lattice_ties_and_the_count_within_max_dist():
    """5 x 5 unit lattice, max_dist 1.5: ties go to the smaller row; the diagonal rows are counted"""
    pos, off = yard.lattice(5, 5)
    res = yard.neighbors(pos, off, k=4, max_dist=1.5)
    assert res.index[12].tolist() == [7, 11, 13, 17] and res.dist2[12].tolist() == [1., 1., 1., 1.] and res.count[12] == 8
    assert res.index[0].tolist() == [1, 5, 6, -1] and res.count[0] == 3
    assert res.dist2[0, :3].tolist() == [1., 1., 2.] and np.isnan(res.dist2[0, 3]) and np.isnan(res.dist[0, 3])


def test_a_row_at_exactly_max_dist_is_not_counted():
    pos, off = yard.table([[[0., 0.], [3., 4.], [6., 8.]]])
    at = yard.neighbors(pos, off, k=2, max_dist=5.)
    assert at.count.tolist() == [0, 0, 0] and (at.index == -1).all() and np.isnan(at.dist).all()
    over = yard.neighbors(pos, off, k=2, max_dist=np.nextafter(5., 6.))
    assert over.count.tolist() == [1, 2, 1] and over.index.tolist() == [[1, -1], [0, 2], [1, -1]]
    assert over.dist2[1].tolist() == [25., 25.] and over.dist[0, 0] == 5.


def test_hand_cases():
    """two frames; a NaN row, coincident rows, groups, lag 1, rows outside the frames, particles"""
    pos = np.array([[0., 0.], [0., 1.], [np.nan, 0.], [0., 1.], [5., 5.],        # frame 0: rows 0 .. 4
                    [0., 0.5], [9., 9.]])                                         # frame 1: rows 5, 6
    off = np.array([0, 5, 7])
    res = yard.neighbors(pos, off, k=2)
    assert res.index.tolist() == [[1, 3], [3, 0], [-1, -1], [1, 0], [1, 3], [6, -1], [5, -1]]
    assert res.dist2[1].tolist() == [0., 1.] and res.count.tolist() == [3, 3, 0, 3, 3, 1, 1]
    assert np.isnan(res.dist2[2]).all() and np.isnan(res.dist2[5, 1])
    group = np.array([0, 0, 0, 1, -1, 0, 0])
    same = yard.neighbors(pos, off, k=2, group=group, pairs='same')
    other = yard.neighbors(pos, off, k=2, group=group, pairs='other')
    assert same.index.tolist() == [[1, -1], [0, -1], [-1, -1], [-1, -1], [-1, -1], [6, -1], [5, -1]]
    assert other.index[4].tolist() == [1, 3] and other.index[3].tolist() == [1, 0]      # group -1 is nobody's group
    assert (same.count + other.count == res.count).all()
    ahead = yard.neighbors(pos, off, k=1, lag=1)
    assert ahead.index[:, 0].tolist() == [5, 5, -1, 5, 6, -1, -1] and ahead.dist2[0, 0] == 0.25 and ahead.dist2[4, 0] == 32.
    assert ahead.count.tolist() == [2, 2, 0, 2, 2, 0, 0]
    assert (yard.neighbors(pos, off, k=1, lag=2).index == -1).all()
    part = yard.neighbors(pos, [1, 5], k=1)                      # rows 0, 5 and 6 are outside every frame
    assert part.index[:, 0].tolist() == [-1, 3, -1, 1, 1, -1, -1] and part.count.tolist() == [0, 2, 0, 2, 2, 0, 0]
    scaled = yard.neighbors(pos, off, k=1, mpp=(2., 0.5))
    assert scaled.dist2[0, 0] == 0.25 and scaled.dist2[4, 0] == 104.
    particle = np.array([0, 1, 2, 9, -1, 0, 4])
    per = yard.neighbors(pos, off, k=1, particle=particle, n_particles=6)
    assert per.particle_min2[:2].tolist() == [1., 0.] and np.isnan(per.particle_min2[2:4]).all()      # 2: a NaN row; 3: absent
    assert per.particle_min2[4] == 153.25 and np.isnan(per.particle_min2[5])      # ids 9 and -1 contribute nowhere
    yard.assert_equal_bits(per.particle_min, np.sqrt(per.particle_min2))
    alone = yard.neighbors(pos[:1], [0, 1], k=1, particle=[0])
    assert np.isnan(alone.particle_min).all() and alone.particle_min.shape == (1,)


def test_the_yardstick_of_a_refused_table():
    r = yard.refused(3, 2, 4)
    assert np.isnan(r.dist).all() and np.isnan(r.dist2).all() and (r.index == -1).all() and not r.count.any()
    assert np.isnan(r.particle_min).all() and r.particle_min.shape == (4,)


@pytest.mark.parametrize('ndim', [2, 3])
def test_the_yardsticks_agree_on_the_shared_rule(ndim):
    """the table and the identity of test_gpu_neighbors.py::test_count_matches_pair_correlation, on the two
    restatements: the pairs that g(r) bins in a frame are the candidates that the neighbours count in it"""
    import _pair_correlation as pcf
    pos, off, group = yard.shared_rule(ndim)
    assert np.diff(off).tolist() == [0, 1, 2, 255, 256, 257, 513] and np.isnan(pos).any(1).sum() == 1 and (group < 0).any()
    mpp = (0.5, 1., 2.)[:ndim]
    totals = {}
    for pairs in ('all', 'same', 'other'):
        g = pcf.pair_correlation(pos, off, yard.SHARED_CUTOFF, yard.SHARED_DR, mpp=mpp, edge='none', group=group, pairs=pairs)
        assert g.count.shape == (7, 16) and g.r_edges[16] == yard.SHARED_CUTOFF
        n = yard.neighbors(pos, off, k=1, mpp=mpp, max_dist=g.r_edges[16], group=group, pairs=pairs)
        totals[pairs] = g.count.sum(1)
        assert (totals[pairs] == yard.counts_per_frame(n.count, off)).all(), (ndim, pairs)
    assert (totals['all'] == totals['same'] + totals['other']).all()
    assert totals['all'][:2].tolist() == [0, 0] and (totals['same'][3:] > 0).all() and (totals['other'][3:] > 0).all()


# ---- argument errors: raised before the engine is looked up ----
POS2, POS3, OFF = np.zeros((4, 2)), np.zeros((4, 3)), np.array([0, 2, 4])
GROUP = np.zeros(4, dtype=np.int64)
BAD_CALLS = {
    'k_zero': (dict(k=0), 'k'), 'k_17': (dict(k=_abi.NBR_MAX_K + 1), 'k'), 'k_float': (dict(k=2.), 'k'), 'k_bool': (dict(k=True), 'k'),
    'k_negative': (dict(k=-1), 'k'),
    'lag_negative': (dict(lag=-1), 'lag'), 'lag_float': (dict(lag=1.5), 'lag'), 'lag_bool': (dict(lag=False), 'lag'),
    'lag_text': (dict(lag='1'), 'lag'),
    'max_dist_zero': (dict(max_dist=0.), 'max_dist'), 'max_dist_negative': (dict(max_dist=-2.), 'max_dist'),
    'max_dist_nan': (dict(max_dist=float('nan')), 'max_dist'), 'max_dist_inf': (dict(max_dist=float('inf')), 'max_dist'),
    'max_dist_text': (dict(max_dist='3'), 'max_dist'), 'max_dist_squares_to_zero': (dict(max_dist=1e-200), 'max_dist'),
    'mpp_zero': (dict(mpp=0.), 'mpp'), 'mpp_negative': (dict(mpp=(1., -1.)), 'mpp'), 'mpp_nan': (dict(mpp=float('nan')), 'mpp'),
    'mpp_three_for_2d': (dict(mpp=(1., 1., 1.)), 'mpp'), 'mpp_two_for_3d': (dict(pos=POS3, mpp=(1., 1.)), 'mpp'),
    'pairs_unknown': (dict(pairs='cross', group=GROUP), 'pairs'),
    'same_without_group': (dict(pairs='same'), 'group'), 'other_without_group': (dict(pairs='other'), 'group'),
    'group_length': (dict(group=np.zeros(3, dtype=np.int64)), 'group'), 'group_dtype': (dict(group=np.zeros(4)), 'group'),
    'group_2d': (dict(group=np.zeros((4, 1), dtype=np.int64)), 'group'),
    'particle_length': (dict(particle=np.zeros(5, dtype=np.int64)), 'particle'), 'particle_dtype': (dict(particle=np.zeros(4)), 'particle'),
    'n_particles_alone': (dict(n_particles=3), 'particle'), 'n_particles_negative': (dict(particle=GROUP, n_particles=-1), 'n_particles'),
    'pos_1d': (dict(pos=np.zeros(4)), 'pos'), 'pos_4d': (dict(pos=np.zeros((4, 4))), 'pos'), 'pos_text': (dict(pos=np.array([['a', 'b']])), 'pos'),
    'offsets_float': (dict(frame_offset=np.array([0., 4.])), 'frame_offset'), 'offsets_empty': (dict(frame_offset=np.zeros(0, dtype=np.int64)), 'frame_offset'),
}


@pytest.mark.parametrize('name', sorted(BAD_CALLS))
def test_argument_errors_of_the_arrays_form(name):
    extra, word = BAD_CALLS[name]
    kw = dict(pos=POS2, frame_offset=OFF)
    kw.update(extra)
    with pytest.raises(ValueError, match=word):
        ct.neighbors_arrays(**kw)


def test_argument_errors_of_the_table_forms():
    f = pd.DataFrame({'frame': [0, 0, 1, 1], 'y': [0., 1., 2., 3.], 'x': [0., 1., 2., 3.], 'cluster': [0, 0, 1, 1], 'size': [1., 1., 1., 1.]})
    for kw, word in ((dict(k=0), 'k'), (dict(lag=-1), 'lag'), (dict(max_dist=0.), 'max_dist'), (dict(pairs='same'), 'group_column'),
                     (dict(pairs='x'), 'pairs'), (dict(group_column='label'), 'label'), (dict(group_column='size'), 'integers'),
                     (dict(pos_columns=['y']), 'pos_columns'), (dict(pos_columns=['y', 'q']), 'pos_columns'), (dict(t_column='t'), "'t'"),
                     (dict(mpp=0.), 'mpp')):
        with pytest.raises(ValueError, match=word):
            ct.neighbors(f, **kw)
    with pytest.raises(ValueError, match='empty'):
        ct.neighbors(f.iloc[:0])
    with pytest.raises(ValueError, match='particle'):
        ct.proximity(f)                                   # not linked
    linked = f.assign(particle=[0, 1, 0, 1])
    for kw, word in ((dict(mpp=-1.), 'mpp'), (dict(pos_columns=['x']), 'pos_columns'), (dict(t_column='t'), "'t'")):
        with pytest.raises(ValueError, match=word):
            ct.proximity(linked, **kw)
    with pytest.raises(ValueError, match='integers'):
        ct.proximity(f.assign(particle=[0., 1., 0., 1.]))


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        return
    with pytest.raises(_lib.EngineError):
        ct.neighbors_arrays(POS2, OFF)
    f = pd.DataFrame({'frame': [0, 1], 'y': [0., 1.], 'x': [0., 1.]})       # no particle column
    with pytest.raises(_lib.EngineError):
        ct.neighbors(f)
    with pytest.raises(_lib.EngineError):
        ct.proximity(f.assign(particle=[0, 0]))


# ---- the stage path ----
def _descriptor():
    d = _abi.Neighbors()
    d.ndim, d.pairs, d.k, d.lag, d.limit2 = 2, _abi.PCF_PAIRS_ALL, 1, 0, float('inf')
    d.mpp[0] = d.mpp[1] = d.mpp[2] = 1.
    d.status = d.frame_offset = 64        # never dereferenced: there is no handle
    return d


CALL = 'ctr_neighbors_device'


def _refused(d):
    lib = _lib.load()
    assert getattr(lib, CALL)(None, ctypes.byref(d), None) == _abi.ERR_INVALID
    return (lib.ctr_last_error(None) or b'').decode()


def test_descriptor_then_handle():
    lib = _lib.load()
    assert getattr(lib, CALL)(None, None, None) == _abi.ERR_INVALID
    assert (lib.ctr_last_error(None) or b'').decode() == CALL + ': null descriptor'
    assert _refused(_descriptor()) == CALL + ': null handle'
    d = _descriptor()
    d.k, d.limit2, d.ndim = _abi.NBR_MAX_K, 1e-300, 3                       # the edges that pass
    assert _refused(d) == CALL + ': null handle'


BAD = [('ndim', 1, 'ndim'), ('ndim', 4, 'ndim'), ('k', 0, 'k must'), ('k', _abi.NBR_MAX_K + 1, 'CTR_NBR_MAX_K'), ('lag', -1, 'lag'),
       ('pairs', 3, 'pairs'), ('pairs', -1, 'pairs'),
       ('n_frames', -1, 'negative'), ('n_features', -1, 'negative'), ('n_particles', -1, 'negative'),
       ('n_frames', 2 ** 31 - 2, 'too many'), ('n_features', 2 ** 31, 'too many'), ('n_particles', 2 ** 31 - 1, 'too many'),
       ('limit2', float('nan'), 'limit2'), ('limit2', 0., 'limit2'), ('limit2', -1., 'limit2'),
       ('status', None, 'null status'), ('frame_offset', None, 'null status'), ('n_features', 1, 'without pos')]


@pytest.mark.parametrize('field,value,word', BAD)
def test_descriptor_is_refused_under_the_entry_point_name(field, value, word):
    d = _descriptor()
    setattr(d, field, value)
    msg = _refused(d)
    assert msg.startswith(CALL + ': ') and word in msg, msg


def test_mpp_group_outputs_and_particles_are_refused():
    for axis, value in ((0, float('nan')), (1, float('inf')), (1, 0.), (0, -1.)):
        d = _descriptor()
        d.mpp[axis] = value
        assert _refused(d) == CALL + ': mpp must be finite and positive'
    d = _descriptor()
    d.mpp[2] = float('nan')                                # ndim 2: the third is not looked at
    assert _refused(d) == CALL + ': null handle'
    d = _descriptor()
    d.n_features, d.pos, d.pairs = 1, 64, _abi.PCF_PAIRS_SAME
    assert 'without group' in _refused(d)
    outputs = ('dist', 'dist2', 'index', 'count')
    for missing in outputs:
        d = _descriptor()
        d.n_features, d.pos = 1, 64
        for name in outputs:
            setattr(d, name, None if name == missing else 64)
        assert _refused(d) == CALL + ': null output'
    for missing in ('particle_min', 'particle_min2'):
        d = _descriptor()
        d.n_particles, d.particle, d.particle_min, d.particle_min2 = 2, 64, 64, 64
        setattr(d, missing, None)
        assert _refused(d) == CALL + ': a particle column without particle_min'
    d = _descriptor()
    d.n_features, d.pos, d.dist, d.dist2, d.index, d.count = 1, 64, 64, 64, 64, 64
    d.n_particles, d.particle_min, d.particle_min2 = 2, 64, 64
    assert _refused(d) == CALL + ': n_particles without particle'
    d.particle = 64
    assert _refused(d) == CALL + ': null handle'


def test_prototype_signature_constants_and_abi():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    assert _lib.load().ctr_abi_version() == 8
    for clause in ('Scaling.', 'A row exists', 'Candidates.', 'Distance.', 'count[i]', 'Neighbours.', 'Rows with no result',
                   'Per particle', 'A refused table.'):
        assert clause in header and clause in st.__doc__, clause
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', header))
    assert set(protos) == set(_lib.SIGNATURES)
    params = [p.strip() for p in protos[CALL].split(',')]
    assert params == ['ctr_handle* h', 'const ctr_neighbors* d', 'void* hip_stream']
    assert _lib.SIGNATURES[CALL] == _lib._stage(_abi.Neighbors) and CALL in _lib.EXPORTS
    assert hasattr(_lib.load(), CALL) and callable(_lib.Engine.neighbors_device)
    body = re.search(r'typedef struct ctr_neighbors \{(.*?)\} ctr_neighbors;', header, flags=re.S).group(1)
    assert re.findall(r'\b(\w+)(?:\[\w+\])?\s*;', body) == [f[0] for f in _abi.Neighbors._fields_]
    defines = dict(re.findall(r'#define\s+(CTR_NBR_\w+)\s+(\d+)', header))
    assert defines == {'CTR_NBR_OK': '0', 'CTR_NBR_BAD_TABLE': '1', 'CTR_NBR_MAX_K': '16'}
    assert (_abi.NBR_OK, _abi.NBR_BAD_TABLE, _abi.NBR_MAX_K) == (0, 1, 16)
    assert len(re.findall(r'#define\s+CTR_\w+_PAIRS_ALL\b', header)) == 1          # the pairs codes of g(r), no second set


def test_struct_layout_matches_the_compiler(tmp_path):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_neighbors));\n'
    expect = [ctypes.sizeof(_abi.Neighbors)]
    for f, _ in _abi.Neighbors._fields_:
        src += 'printf("%%zu\\n", offsetof(ctr_neighbors, %s));\n' % f
        expect.append(getattr(_abi.Neighbors, f).offset)
    src += 'return 0;}\n'
    (tmp_path / 'layout.c').write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == expect


def test_public_names():
    names = {'neighbors_arrays', 'neighbors', 'proximity'}
    assert names | {'static'} <= set(ct.__all__) and ct.static is st
    for name in names:
        assert getattr(ct, name) is getattr(st, name)
    assert st.Neighbors._fields == ('dist', 'dist2', 'index', 'count', 'particle_min', 'particle_min2', 'status')
    assert 'cKDTree' in st.neighbors.__doc__ and 'static.proximity' in st.proximity.__doc__ and 'trackpy' in st.neighbors_arrays.__doc__
    for fn in (st.neighbors, st.proximity):
        assert 'trackpy' in fn.__doc__ and 'not pinned' in fn.__doc__ and 'not a dependency' in fn.__doc__
