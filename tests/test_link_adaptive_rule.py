"""The adaptive search range of the linker without a GPU (clustertracking_amd/link.py's module text,
DESIGN.md 7b): the host restatement against the plain call, against the independent restatement of
tests/_link_adaptive.py and against exhaustive enumeration; the validation; the C-ABI of
``ctr_link_adaptive_device``."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest
from numpy.testing import assert_equal

import _cases
import _link_adaptive as ref
from _link_adaptive import blob40, blob100, lattice, memory_case
from clustertracking_amd import _abi, _lib
from clustertracking_amd import link as lk

Z = np.load(os.path.join(_cases.GOLDEN, 'link', 'link_edge_cases.npz'))
NAMES = sorted(k[:-4] for k in Z.files if k.endswith('_ids'))


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def assert_equals_restatement(levels, sr, memory, stop, step, got=None):
    ids, rounds = got if got is not None else lk.link_levels(levels, sr, memory, adaptive_stop=stop, adaptive_step=step,
                                                             diag=True)
    want_ids, want_rounds = ref.link_levels(levels, sr, memory, stop, step)
    for t in range(len(levels)):
        assert_equal(ids[t], want_ids[t], err_msg='ids of level %d' % t)
        assert_equal(rounds[t], want_rounds[t], err_msg='rounds of level %d' % t)
        assert ids[t].dtype == np.int64 and rounds[t].dtype == np.int32
    return ids, rounds


def _levels(name):
    offs = np.r_[0, np.cumsum(Z[name + '_counts'])]
    return [Z[name + '_pos'][a:b] for a, b in zip(offs[:-1], offs[1:])]


@pytest.mark.parametrize('name', NAMES)
def test_same_ids_as_the_plain_call_on_the_edge_fixtures(name):
    levels, sr, memory = _levels(name), tuple(Z[name + '_sr']), int(Z[name + '_memory'])
    plain = lk.link_levels(levels, sr, memory)
    ids, rounds = lk.link_levels(levels, sr, memory, adaptive_stop=tuple(0.1 * s for s in sr), diag=True)
    assert_equal(np.concatenate(ids), np.concatenate(plain))
    assert_equal(np.concatenate(ids), Z[name + '_ids'])
    assert not np.concatenate(rounds).any()
    assert_equal(np.concatenate(lk.link_levels(levels, sr, memory, adaptive_stop=tuple(0.1 * s for s in sr))),
                 Z[name + '_ids'])


def test_blob_of_40_is_resolved():
    levels, perm = blob40()
    with pytest.raises(lk.SubnetOversizeException):
        lk.link_levels(levels, 5.)
    ids, rounds = assert_equals_restatement(levels, 5., 0, .25, .9)
    assert sorted(ids[1]) == list(range(40))                  # all 40 linked
    print('on the true partner: %d, rounds: %s' % ((ids[1] == perm).sum(), np.bincount(rounds[1])))
    assert (ids[1] == perm).sum() == 38 and rounds[1].max() + 1 == 9
    assert not rounds[0].any()
    with pytest.raises(lk.SubnetOversizeException) as info:
        lk.link_levels(levels, 5., adaptive_stop=3., adaptive_step=.95)
    assert 'level 1' in str(info.value) and '40' in str(info.value)
    with pytest.raises(ref.GaveUp):
        ref.link_levels(levels, 5., 0, 3., .95)


def test_blob_of_100_has_too_many_destinations_and_is_resolved():
    levels = blob100()
    with pytest.raises(lk.SubnetOversizeException):
        lk.link_levels(levels, 5.)
    edges = ref.candidates(levels[1], levels[0], [5., 5.])
    assert max(len({j for _, j in part}) for part in ref.components(edges)) > 64
    ids, rounds = assert_equals_restatement(levels, 5., 0, .25, .9)
    assert rounds[1].max() > 0 and (ids[1] < 100).sum() > 90


def test_lattice_is_exact():
    """rho = 1, 0.5, 0.25 are exact: the neighbours at 0.5 survive the first cut (36 x 36 still), the
    second leaves every point its own copy"""
    levels = lattice()
    ids, rounds = assert_equals_restatement(levels, 2., 0, .4, .5)
    assert_equal(ids[1], np.arange(36))
    assert_equal(rounds[1], np.full(36, 2))
    assert_equal(rounds[0], np.zeros(36))


def test_memory_takes_the_sources_that_a_cut_set_free():
    levels, lost = memory_case()
    ids, rounds = assert_equals_restatement(levels, 5., 2, .25, .9)
    assert rounds[2].max() > 0
    # ids of level 1 that level 2 did not continue, continued by level 3 or 4
    back = [p for p in lost(ids) if p in ids[3] or p in ids[4]]
    print('lost at level 2: %r, back at level 3 or 4: %r' % (lost(ids), back))
    assert len(lost(ids)) == 3 and len(back) >= 1


def test_solver_is_optimal_on_small_subnetworks():
    """the host's assignment against every set of links tried, at several rho"""
    rng = np.random.default_rng(7)
    tried = 0
    for trial in range(60):
        ns, nd = rng.integers(2, 7), rng.integers(2, 7)
        rho = float(rng.choice([1., .9, .5, .3]))
        src = rng.uniform(0, rho, (ns, 2))
        dst = rng.uniform(0, rho, (nd, 2))
        b = rho * (1. + 1e-7)
        edges = {(i, j): ref.scaled_d2(dst[j], src[i], [1., 1.]) for i in range(ns) for j in range(nd)}
        edges = {e: d2 for e, d2 in edges.items() if d2 <= b * b}
        parts = [p for p in ref.components(edges) if len(p) > 1]
        for part in parts:
            s_ids = sorted({i for i, _ in part})
            d_ids = sorted({j for _, j in part})
            cs = np.array([e[0] for e in part])
            cd = np.array([e[1] for e in part])
            d2 = np.array([part[e] for e in part])
            link, _ = _solve_at(ns, nd, cs, cd, d2, rho)
            total = sum(2. * (rho * rho) - part[(link[j], j)] for j in d_ids if link[j] >= 0)
            assert all((link[j], j) in part for j in d_ids if link[j] >= 0)
            best, _ = ref.best_by_enumeration(s_ids, d_ids, part, rho)
            assert abs(total - best) <= 1e-12 * max(best, 1.), (trial, total, best)
            tried += 1
    assert tried >= 40


def _solve_at(n_src, n_dst, cand_src, cand_dst, cand_d2, rho, pad=31):
    """link._assign_adaptive solving one sub-network (edges within rho) at rho.  rho = 1: round 0.
    Else at round 1 of a step of rho: one more destination lists 31 more sources and a source of
    the sub-network, all at a d2 just above the cut, so round 0 sees one oversize sub-network and
    the cut to rho takes exactly the added edges."""
    if rho == 1.:
        return lk._assign_adaptive(n_src, n_dst, cand_src, cand_dst, cand_d2, .01, .5, 1)
    b = rho * (1. + 1e-7)
    above = b * b * (1. + 1e-9)
    cs = np.r_[cand_src, n_src + np.arange(pad), cand_src[0]]
    cd = np.r_[cand_dst, np.full(pad, n_dst), n_dst]
    d2 = np.r_[cand_d2, np.full(pad, above), above]
    link, rounds = lk._assign_adaptive(n_src + pad, n_dst + 1, cs, cd, d2, .01, rho, 1)
    assert (rounds[np.unique(cand_dst)] == 1).all() and link[n_dst] == -1 and rounds[n_dst] == 1
    return link[:n_dst], rounds[:n_dst]


def test_validation():
    levels = lattice()
    for stop in (2., 2.5, 0., -1., float('nan')):                 # at or above the range, zero or below
        with pytest.raises(ValueError):
            lk.link_levels(levels, 2., adaptive_stop=stop)
    for step in (0., 1., -.5, 1.5, float('nan')):
        with pytest.raises(ValueError):
            lk.link_levels(levels, 2., adaptive_stop=.5, adaptive_step=step)
    with pytest.raises(ValueError):                               # 0.99^k reaches 0.5 only at k = 69
        lk.link_levels(levels, 2., adaptive_stop=1., adaptive_step=.99)
    assert lk._adaptive_plan((2., 2.), 1., .99 ** (69 / 64.))[2] == 64
    # a step without a stop is ignored
    assert_equal(np.concatenate(lk.link_levels(levels[:1], 2., adaptive_step=7.)), np.arange(36))
    # per axis: the largest ratio decides
    assert lk._adaptive_plan((4., 2.), (1., 1.), .5) == (.5, .5, 1)
    assert lk._adaptive_plan((4., 2.), (3., 1.), .5) == (.75, .5, 1)
    assert lk._adaptive_plan((4., 2.), 1., .9)[0] == .5
    with pytest.raises(ValueError):
        lk.link_levels(levels, (4., 2.), adaptive_stop=(1., 2.))
    with pytest.raises(ValueError):
        lk.link_levels(levels, (4., 2.), adaptive_stop=(1., 1., 1.))
    with pytest.raises(ValueError):
        lk.link_levels([], 2., adaptive_stop=3.)
    stop_rel, step, k = lk._adaptive_plan((5., 5.), .25, .9)
    assert (stop_rel, step, k) == (.05, .9, 29) and len(ref.plan([5., 5.], [.25, .25], .9)[1]) == 30
    f = pd.DataFrame({'y': [1., 1.5, 2.], 'x': [1., 1.2, 1.4], 'frame': [0, 1, 2]})
    with pytest.raises(ValueError):
        lk.link(f, 3, adaptive_stop=3)
    got = lk.link(f, 3, adaptive_stop=1, diag=True)
    assert list(got.columns)[-2:] == ['particle', 'adaptive_round']
    assert_equal(got['particle'].values, [0, 0, 0])
    assert got['adaptive_round'].dtype == np.int32 and not got['adaptive_round'].any()
    assert 'adaptive_round' in lk.link(f, 3, diag=True) and 'adaptive_round' not in lk.link(f, 3, adaptive_stop=1)
    ids, rounds = lk.link_levels([np.array([[0., 0.], [10., 10.]])] * 2, 2., diag=True)
    assert_equal(np.concatenate(ids), [0, 1, 0, 1])
    assert_equal(np.concatenate(rounds), np.zeros(4))
    assert rounds[1].dtype == np.int32


def test_header_declares_and_library_exports():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'\bint\s+ctr_link_adaptive_device\s*\(\s*ctr_handle\s*\*\s*\w*\s*,\s*const\s+ctr_link_adaptive\s*\*', header)
    assert 'typedef struct ctr_link_adaptive' in header
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    assert 'ctr_link_adaptive_device' in _lib.EXPORTS
    assert _lib.SIGNATURES['ctr_link_adaptive_device'] == _lib._stage(_abi.LinkAdaptive)
    lib = _lib.load()
    assert hasattr(lib, 'ctr_link_adaptive_device') and lib.ctr_abi_version() == 8
    assert callable(_lib.Engine.link_adaptive_device)


def test_struct_layout_matches_header(tmp_path):
    fields = [f[0] for f in _abi.LinkAdaptive._fields_]
    assert fields[:len(_abi.Link._fields_)] == [f[0] for f in _abi.Link._fields_]
    assert fields[len(_abi.Link._fields_):] == ['stop_rel', 'step', 'max_rounds', 'adaptive_round']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu %zu\\n", sizeof(ctr_link_adaptive), sizeof(ctr_link));\n'
    for f in fields:
        src += 'printf("%%zu\\n", offsetof(ctr_link_adaptive, %s));\n' % f
    src += 'printf("%d\\n", CTR_LINK_MAX_ROUNDS);\nreturn 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == ctypes.sizeof(_abi.LinkAdaptive) and out[1] == ctypes.sizeof(_abi.Link)
    assert out[2:2 + len(fields)] == [getattr(_abi.LinkAdaptive, f).offset for f in fields]
    assert [getattr(_abi.LinkAdaptive, f[0]).offset for f in _abi.Link._fields_] == \
        [getattr(_abi.Link, f[0]).offset for f in _abi.Link._fields_]
    assert out[-1] == _abi.LINK_MAX_ROUNDS == 64


def _descriptor(n=0):
    d = _abi.LinkAdaptive()
    d.ndim, d.memory, d.n_levels, d.n_features = 2, 0, 3, n
    d.search_range[0] = d.search_range[1] = 5.
    d.stop_rel, d.step, d.max_rounds = .05, .9, 29
    # never dereferenced: the descriptor is refused, or the handle is
    d.pos = d.frame_offset = d.particle = d.n_tracks = d.status = d.adaptive_round = 8
    return d


def test_validation_needs_no_device():
    lib = _lib.load()

    def call(d):
        rc = lib.ctr_link_adaptive_device(None, ctypes.byref(d), None)
        return rc, (lib.ctr_last_error(None) or b'').decode()

    for n in (0, 7):
        rc, msg = call(_descriptor(n))
        assert rc == _abi.ERR_INVALID and msg == 'ctr_link_adaptive_device: null handle'
    d = _descriptor(7)
    d.adaptive_round = None                  # the diagnostic is optional
    assert call(d)[1] == 'ctr_link_adaptive_device: null handle'
    rc = lib.ctr_link_adaptive_device(None, None, None)
    assert rc == _abi.ERR_INVALID and b'null descriptor' in lib.ctr_last_error(None)
    for field, bad, word in [('stop_rel', (0., 1., -.1, 1.5, float('nan')), 'stop_rel'),
                             ('step', (0., 1., -.1, 1.5, float('nan')), 'step'),
                             ('max_rounds', (0, -1, 65), 'max_rounds')]:
        for value in bad:
            d = _descriptor()
            setattr(d, field, value)
            rc, msg = call(d)
            assert rc == _abi.ERR_INVALID and word in msg and 'null handle' not in msg, (field, value, msg)
    for value in (1, 64):
        d = _descriptor()
        d.max_rounds = value
        assert 'null handle' in call(d)[1]
    # ctr_link's own checks
    d = _descriptor()
    d.ndim = 4
    assert 'ndim' in call(d)[1]
    d = _descriptor()
    d.search_range[1] = 0.
    assert 'search_range' in call(d)[1]
    d = _descriptor()
    d.memory = -1
    assert 'memory' in call(d)[1]
    d = _descriptor(5)
    d.status = None
    assert 'null output' in call(d)[1]


@pytest.mark.skipif(_gpu_present(), reason="a GPU is present: tests/test_gpu_link_adaptive.py runs the device path")
def test_no_cpu_fallback():
    levels = lattice()
    with pytest.raises(_lib.EngineError):
        lk.link_levels(levels, 2., engine='device', adaptive_stop=.4, adaptive_step=.5)
    with pytest.raises(_lib.EngineError):
        lk.link_arrays(np.concatenate(levels), [0, 36, 72], 2., adaptive_stop=.4, adaptive_step=.5, diag=True)
    with pytest.raises(ValueError):          # refused before the engine is looked for
        lk.link_levels(levels, 2., engine='device', adaptive_stop=2.)
    with pytest.raises(ValueError):
        lk.link_arrays(np.concatenate(levels), [0, 36, 72], 2., adaptive_stop=.4, adaptive_step=1.)
