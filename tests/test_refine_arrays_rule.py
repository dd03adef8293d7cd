"""``ct.refine_arrays`` and the prepare stage without a device: the yardstick
``tests/_refine_arrays.py`` against the shipped host path ``prepare_batch``, the refusals of
``refine_arrays`` before the engine, and the stage path of ``ctr_refine_prepare_device`` /
``ctr_refine_prepare_plan`` -- descriptor before handle, the header's prototypes against
``_lib.SIGNATURES``, the struct's layout."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _cases
import _refine_arrays as yard
import clustertracking_amd as ct
from clustertracking_amd import _abi, _lib


@pytest.mark.parametrize('name', yard.PREPARE + yard.REFINE)
def test_yardstick_is_the_shipped_host_path(name):
    """after relabelling (the reference's ids depend on set order, the yardstick's are the smallest
    row), the yardstick's tables are prepare_batch's"""
    case = yard.cases()[name]
    want = yard.yardstick(case)
    ff, _, _ = yard.model(case)
    assert yard.infeasible(ff, want) is None
    prep = ct.prepare_batch(yard.table(case), ct.ArrayReader(case.frames), cluster_labels='reference',
                            **yard.refine_kwargs(case))
    b = prep.batch
    # relabel: a cluster is named by its smallest row, and the clusters of a frame follow in that order
    order_rows = np.asarray(prep.order, dtype=np.int64)
    canon = np.array([order_rows[b.feat_offset[c]:b.feat_offset[c + 1]].min() for c in range(b.n_clusters)],
                     dtype=np.int64)
    label = np.empty(len(case.pos), dtype=np.int64)
    for c in range(b.n_clusters):
        label[order_rows[b.feat_offset[c]:b.feat_offset[c + 1]]] = canon[c]
    np.testing.assert_array_equal(label, want.label)
    np.testing.assert_array_equal(prep.f['cluster_size'].values, want.cluster_size)
    theirs = np.lexsort((canon, b.frame_index))
    np.testing.assert_array_equal(np.r_[0, np.cumsum(np.diff(b.feat_offset)[theirs])], want.feat_offset)
    np.testing.assert_array_equal(b.frame_index[theirs], want.frame_index)
    rows = np.concatenate([np.arange(b.feat_offset[c], b.feat_offset[c + 1]) for c in theirs] +
                          [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    np.testing.assert_array_equal(prep.order[rows], want.order)
    for theirs_t, ours in ((b.params, want.params), (b.low, want.low), (b.high, want.high)):
        assert ours.dtype == np.float64 and ours.shape == (len(case.pos), ff.n_params)
        np.testing.assert_array_equal(theirs_t[rows], ours)


@pytest.mark.parametrize('name', sorted(yard.INFEASIBLE))
def test_yardstick_refuses_the_box_that_prepare_batch_refuses(name):
    case = yard.cases()[name]
    ff, _, _ = yard.model(case)
    assert yard.infeasible(ff, yard.yardstick(case)) == yard.INFEASIBLE[name]
    with pytest.raises(ValueError, match=r"SLSQP Error: the lower bound exceeds the upper bound \(parameter '%s'\)"
                       % yard.INFEASIBLE[name]):
        ct.prepare_batch(yard.table(case), ct.ArrayReader(case.frames), **yard.refine_kwargs(case))


def test_yardstick_known_answers():
    """hand-checked: the tie, the chain, the straddling cluster, the bounds of one value"""
    c = yard.cases()
    np.testing.assert_array_equal(yard.yardstick(c['exact_tie']).label, [0, 0, 2, 3, 4])
    np.testing.assert_array_equal(yard.yardstick(c['pythagoras']).label, [0, 0, 2, 2, 4])
    y = yard.yardstick(c['chain'])
    assert (y.cluster_size[3:] == 40).all() and (y.label[3:] == 3).all() and (y.cluster_size[:3] == 1).all()
    y = yard.yardstick(c['straddle'])
    np.testing.assert_array_equal(np.flatnonzero(y.cluster_size == 4), [10, 255, 256, 299])
    np.testing.assert_array_equal(y.label[[10, 255, 256, 299]], 10)
    np.testing.assert_array_equal(y.order[10:14], [10, 255, 256, 299])
    y = yard.yardstick(c['tile_edges'])
    np.testing.assert_array_equal(np.bincount(y.frame_index, minlength=5) > 0, [True, False, True, True, True])
    y = yard.yardstick(c['bounds_all'])        # signal 90: max(90 - 30, 90 * 0.5, 1), min(90 + 40, 90 * 1.6, 500)
    assert (y.low[:, 1] == 60.).all() and (y.high[:, 1] == 130.).all()
    y = yard.yardstick(c['bounds_none'])       # signal, the positions without their default, thickness
    assert np.isneginf(y.low[:, [1, 2, 3, 5]]).all() and np.isposinf(y.high[:, 1:]).all() and (y.low[:, [0, 4]] == 0).all()
    y = yard.yardstick(c['nan_start'])
    rows = np.flatnonzero(np.isnan(y.params[:, 1]))
    assert len(rows) == 2 and (y.low[rows, 1] == 0.).all() and np.isposinf(y.high[rows, 1]).all()
    rows = np.flatnonzero(np.isnan(y.params[:, 4]))
    assert len(rows) == 1 and (y.low[rows, 4] == 0.5).all() and (y.high[rows, 4] == 10.).all()


def test_refusals_before_the_engine(monkeypatch):
    def no_engine(device=0):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    case = yard.cases()['gauss_2d']
    frames, pos, off = case.frames, case.pos, case.off
    call = lambda *a, **k: ct.refine_arrays(*a, **dict(dict(signal=90., size=2.), **k))
    with pytest.raises(NotImplementedError, match='global'):
        call(frames, pos, off, 9, param_mode=dict(size='global'))
    with pytest.raises(NotImplementedError, match='dict'):
        call(frames, pos, off, 9, fit_function=dict(name='mine', params=[], fun=None))
    with pytest.raises(NotImplementedError, match='one constraint'):
        call(frames, pos, off, 9, constraints=ct.constraints.dimer(5.) + ct.constraints.trimer(5.))
    for bad in (0, -1):
        with pytest.raises(ValueError, match='max_iter'):
            call(frames, pos, off, 9, max_iter=bad)
    for bad in (frames[0], frames[0, 0], frames[None, None]):
        with pytest.raises(ValueError, match='frames'):
            call(bad, pos, off, 9)
    for bad in (pos[:, :1], pos.reshape(-1), np.c_[pos, pos[:, :1]]):
        with pytest.raises(ValueError, match='pos must be'):
            call(frames, bad, off, 9)
    for bad in (off[::-1].copy(), np.r_[0, 13, 12], off - 1, np.r_[0, 12, 23], off[:-1], off.astype(float)):
        with pytest.raises(ValueError, match='frame_offset'):
            call(frames, pos, bad, 9)
    huge = np.lib.stride_tricks.as_strided(np.zeros(1), shape=(2 ** 31, 2), strides=(0, 0))
    with pytest.raises(ValueError, match='rows'):
        call(frames, huge, off, 9)
    with pytest.raises(ValueError, match='signal'):
        ct.refine_arrays(frames, pos, off, 9, size=2.)


def test_public_names():
    from clustertracking_amd import refine
    assert 'refine_arrays' in ct.__all__ and ct.refine_arrays is refine.refine_arrays
    assert refine.RefineResult._fields == ('params', 'columns', 'cost', 'cluster', 'cluster_size', 'params_std',
                                           'status', 'n_rounds', 'n_iter', 'feat_offset')


def _descriptor(n=1000, n_frames=3, ndim=2, modes=(3, 1, 1, 1, 0)):
    d = _abi.RefinePrepare()
    d.mode, d.ndim, d.n_params, d.n_frames, d.n_features = _abi.PREPARE_BATCH, ndim, len(modes), n_frames, n
    for a in range(ndim):
        d.separation[a] = 5.
    for k, m in enumerate(modes):
        d.modes[k] = m
    return d


def test_plan_reports_the_scratch():
    """scaled positions, three words per row, one per frame; blocks aligned to 256 bytes"""
    for n, t, ndim in ((1000, 3, 2), (1000, 3, 3), (0, 0, 2), (257, 5, 2), (2 ** 31 - 2, 7, 3)):
        scratch = _lib.refine_prepare_plan(_descriptor(n, t, ndim))
        need = (8 * ndim + 12) * n + 4 * (t + 1)
        assert need <= scratch <= need + 5 * 256
    d = _descriptor()
    d.mode = _abi.PREPARE_SCATTER
    assert _lib.refine_prepare_plan(d) == 0


def test_descriptor_then_handle():
    """a malformed descriptor is reported, under the entry point's name, before the handle is looked
    at; a valid one reaches "null handle" """
    lib = _lib.load()
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    call = 'ctr_refine_prepare_device'
    assert lib.ctr_refine_prepare_device(None, None, None) == _abi.ERR_INVALID
    assert msg() == call + ': null descriptor'
    keep = []

    def filled(d):
        for name, ctype in _abi.RefinePrepare._fields_:
            if ctype is ctypes.c_void_p:
                keep.append(ctypes.create_string_buffer(8))
                setattr(d, name, ctypes.addressof(keep[-1]))     # never dereferenced: there is no handle
        return d
    for change, why in ((dict(mode=2), 'mode'), (dict(ndim=4), 'ndim'), (dict(n_params=0), 'n_params'),
                        (dict(n_params=13), 'n_params'), (dict(n_features=-1), 'negative'),
                        (dict(n_features=2 ** 31 - 1), 'too many'), (dict(n_frames=-1), 'negative')):
        d = filled(_descriptor())
        for k, v in change.items():
            setattr(d, k, v)
        assert lib.ctr_refine_prepare_device(None, ctypes.byref(d), None) == _abi.ERR_INVALID
        assert msg().startswith(call + ': ') and why in msg() and 'null handle' not in msg(), msg()
        with pytest.raises(ValueError, match=why):
            _lib.refine_prepare_plan(d)
    d = filled(_descriptor())
    d.separation[1] = 0.
    assert lib.ctr_refine_prepare_device(None, ctypes.byref(d), None) == _abi.ERR_INVALID and 'separation' in msg()
    d = filled(_descriptor(modes=(3, 1, 2, 1, 0)))
    assert lib.ctr_refine_prepare_device(None, ctypes.byref(d), None) == _abi.ERR_INVALID and 'modes' in msg()
    d = filled(_descriptor())
    d.status = None
    assert lib.ctr_refine_prepare_device(None, ctypes.byref(d), None) == _abi.ERR_INVALID and 'status' in msg()
    assert _lib.refine_prepare_plan(d) > 0           # the plan looks at no pointer
    for mode in (_abi.PREPARE_BATCH, _abi.PREPARE_SCATTER):
        d = filled(_descriptor())
        d.mode = mode
        assert lib.ctr_refine_prepare_device(None, ctypes.byref(d), None) == _abi.ERR_INVALID
        assert msg() == call + ': null handle'


def test_prototypes_signatures_and_layout(tmp_path):
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    bare = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    protos = dict(re.findall(r'\b(ctr_[a-z_]+)\s*\(([^()]*)\)\s*;', bare))
    params = [p.strip() for p in protos['ctr_refine_prepare_device'].split(',')]
    assert params == ['ctr_handle* h', 'const ctr_refine_prepare* r', 'void* hip_stream']
    assert _lib.SIGNATURES['ctr_refine_prepare_device'] == _lib._stage(_abi.RefinePrepare)
    assert len(protos['ctr_refine_prepare_plan'].split(',')) == 2 == len(_lib.SIGNATURES['ctr_refine_prepare_plan'][1])
    assert {'ctr_refine_prepare_device', 'ctr_refine_prepare_plan'} <= set(_lib.EXPORTS)
    assert callable(_lib.Engine.refine_prepare_device)
    for name in ('BATCH', 'SCATTER', 'OK', 'BAD_TABLE', 'INFEASIBLE'):
        value = int(re.search(r'#define\s+CTR_PREPARE_%s\s+(\d+)' % name, header).group(1))
        assert getattr(_abi, 'PREPARE_' + name) == value
    # the struct of _abi is the header's: compiled, the same size and offsets
    fields = [f[0] for f in _abi.RefinePrepare._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void) {\n'
    src += 'printf("%zu\\n", sizeof(ctr_refine_prepare));\n'
    for f in fields:
        src += 'printf("%%zu\\n", offsetof(ctr_refine_prepare, %s));\n' % f
    src += 'return 0;\n}\n'
    (tmp_path / 'layout.c').write_text(src)
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', exe])
    out = [int(v) for v in subprocess.check_output([exe]).split()]
    assert out == [ctypes.sizeof(_abi.RefinePrepare)] + [getattr(_abi.RefinePrepare, f).offset for f in fields]
