"""The rule of ``ctr_find_link_device`` as tests/_find_link.py restates it, without a device: the
constructed edge cases do what they were constructed for, the loop without anything lost is
``link_levels``, and the descriptor's mirror matches the header."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _cases
import _find_link as F
import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib
from clustertracking_amd import link as lk

EDGE = F.edge_cases()
FIXTURES = F.fixtures()


@pytest.mark.parametrize('index', range(len(FIXTURES)), ids=[c[0] for c in FIXTURES])
def test_restatement_equals_the_reference(index):
    name, frames, kw, want = FIXTURES[index]
    kw = {k: v for k, v in kw.items() if k != 'percentile'}
    got = F.find_link(frames, percentile=64, **kw)
    F.assert_equals_fixture(got, want, frames.ndim - 1, F.is_isotropic(kw), frames.dtype.kind in 'ui')


def test_fixtures_cover_what_they_are_for():
    names = [c[0] for c in FIXTURES]
    assert len(names) >= 7 and all(c[3]['relocated'].sum() >= 3 for c in FIXTURES)
    assert {c[1].dtype.name for c in FIXTURES} >= {'uint8', 'uint16', 'float64'}
    assert {c[2]['memory'] for c in FIXTURES} >= {0, 1, 2} and any(c[1].ndim == 4 for c in FIXTURES)
    assert any(c[2]['scale_factor'] == 1. for c in FIXTURES) and any(c[2]['scale_factor'] != 1. for c in FIXTURES)
    assert all(6 <= len(c[1]) <= 10 for c in FIXTURES)


def run(name, **extra):
    frames, kw = EDGE[name]
    log = []
    res = F.find_link(frames, log=log, **dict(kw, **extra))
    return res, log


def test_lost_pair_within_two_search_ranges_is_one_query():
    res, log = run('lost_pair_1_5')
    assert [(q['level'], len(q['sources']), q['shortage'], q['n_found']) for q in log] == [(1, 2, 2, 2)]
    assert res['relocated'].tolist() == [False, False, True, True]
    assert res['particle'].tolist() == [0, 1, 0, 1] and res['n_tracks'] == 2 and not res['coupled'].any()
    assert res['pos'][2:].tolist() == [[1., 30.], [1., 36.]]


def test_lost_pair_beyond_two_search_ranges_is_two_queries():
    res, log = run('lost_pair_2_5')
    assert [(q['level'], len(q['sources']), q['shortage'], q['n_found']) for q in log] == [(1, 1, 1, 1)] * 2
    assert res['particle'].tolist() == [0, 1, 0, 1] and res['relocated'].sum() == 2 and not res['coupled'].any()


def test_short_subnet_meets_surplus_no_query():
    res, log = run('short_meets_surplus')
    assert log == []
    # the lost one stays lost although its candidate is there; the spare destination starts a track
    assert np.diff(res['frame_offset']).tolist() == [2, 2] and not res['relocated'].any()
    assert res['particle'].tolist() == [0, 1, 1, 2]
    frames, kw = EDGE['short_meets_surplus']
    assert frames[1, 1, 28] > 0


def test_eleventh_source_is_not_united():
    res, log = run('eleventh_source')
    assert np.diff(res['frame_offset']).tolist() == [11, 10]
    sr = 4.
    first = res['pos'][:11]
    lost = np.array([11., 32.])
    assert (np.sqrt(((first - lost) ** 2).sum(1)) <= 2 * sr).all()          # all eleven within 2
    assert [(len(q['sources']), q['shortage']) for q in log] == [(10, 1)]
    assert not any((q['sources'] == [11., 25.]).all(1).any() for q in log)  # the farthest is not in it


def test_coupled_level_is_flagged():
    res, log = run('coupled')
    assert len(log) == 2 and res['coupled'].tolist() == [False, True] and res['relocated'].sum() == 2


def test_spare_candidate_is_dropped():
    res, log = run('spare_candidate')
    assert [(len(q['sources']), q['shortage'], q['n_found']) for q in log] == [(1, 1, 2)]
    assert res['pos'].tolist() == [[3., 30.], [1., 28.]] and res['particle'].tolist() == [0, 0]


def test_empty_first_frame():
    res, log = run('empty_first_frame')
    assert np.diff(res['frame_offset']).tolist() == [0, 1, 1]
    assert res['particle'].tolist() == [0, 0] and res['relocated'].tolist() == [False, True]


def test_frame_whose_rows_are_all_relocated():
    res, log = run('all_relocated')
    assert np.diff(res['frame_offset']).tolist() == [2, 2] and res['relocated'].tolist() == [False, False, True, True]
    assert sorted(res['particle'][2:].tolist()) == [0, 1]
    assert res['pos'][2:].tolist() == [[1., 30.], [20., 1.]]       # C order of position


def test_all_zero_frame_has_no_threshold():
    res, log = run('zero_frame')
    assert [(q['level'], q['n_found']) for q in log] == [(1, 0)]
    assert np.diff(res['frame_offset']).tolist() == [1, 0, 1] and res['particle'].tolist() == [0, 0]   # remembered
    res0, _ = run('zero_frame', memory=0)
    assert res0['particle'].tolist() == [0, 1]


def test_refusals():
    with pytest.raises(F.Refused) as e:
        run('lost_pair_2_5', max_queries=1)
    assert (e.value.what, e.value.level) == ('queries', 1)
    with pytest.raises(F.Refused) as e:
        run('lost_pair_1_5', max_relocated=1)
    assert (e.value.what, e.value.level) == ('rows', 1)
    frames, kw = F.oversize_case()
    with pytest.raises(lk.SubnetOversizeException):
        F.find_link(frames, **kw)
    for case, what in ((F.relocate_capacity_case, 'relocate'), (F.destinations_case, 'destinations')):
        frames, kw = case()
        with pytest.raises(F.Refused) as e:
            F.find_link(frames, **kw)
        assert (e.value.what, e.value.level) == (what, 1)


@pytest.mark.parametrize('index', range(6))
def test_nothing_lost_is_link_levels(index):
    """every feature bright in every frame: the loop is the linker's"""
    name, frames, kw = F.bright_cases()[index % len(F.bright_cases())]
    log = []
    res = F.find_link(frames, log=log, **kw)
    assert not res['relocated'].any()
    off = res['frame_offset']
    levels = [res['pos'][a:b] for a, b in zip(off[:-1], off[1:])]
    ids = lk.link_levels(levels, kw['search_range'], kw['memory'])
    assert not log and np.diff(off).tolist() == [12] * 6 and np.array_equal(np.concatenate(ids), res['particle'])


def test_random_cases_relocate():
    """what the device tests rely on: the seeded videos do relocate, in queries of one and of
    several sources, on coupled levels and not"""
    n_reloc = n_multi = n_spare = n_coupled = 0
    for name, frames, kw in F.random_cases():
        log = []
        res = F.find_link(frames, log=log, **kw)
        n_reloc += int(res['relocated'].sum())
        n_multi += sum(len(q['sources']) > 1 and q['n_found'] > 0 for q in log)
        n_spare += sum(q['n_found'] > q['shortage'] for q in log)
        n_coupled += int(res['coupled'].sum())
    assert n_reloc >= 60 and n_multi >= 5 and n_coupled >= 3, (n_reloc, n_multi, n_spare, n_coupled)


def test_header_declares_and_library_exports():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'\bint\s+ctr_find_link_device\s*\(\s*ctr_handle\s*\*', header)
    assert 'typedef struct ctr_find_link' in header
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    assert 'ctr_find_link_device' in _lib.EXPORTS and hasattr(_lib.load(), 'ctr_find_link_device')
    assert {'find_link', 'find_link_arrays'} <= set(cta.__all__)


def test_find_link_struct_layout_matches_header(tmp_path):
    """ctypes mirror of ctr_find_link vs the C compiler's view of include/ctrefine.h"""
    fields = [f[0] for f in _abi.FindLink._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_find_link));\n'
    for f in fields:
        src += 'printf("%%zu\\n", offsetof(ctr_find_link, %s));\n' % f
    src += 'printf("%d %d %d %d %d %d\\n", CTR_FIND_LINK_OK, CTR_FIND_LINK_OVERSIZE, CTR_FIND_LINK_CAPACITY, '
    src += 'CTR_FIND_LINK_RELOCATE, CTR_FIND_LINK_QUERIES, CTR_FIND_LINK_ROWS);\nreturn 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    n = len(fields)
    assert out[0] == ctypes.sizeof(_abi.FindLink)
    assert out[1:1 + n] == [getattr(_abi.FindLink, f).offset for f in fields]
    assert out[1 + n:] == [_abi.FIND_LINK_OK, _abi.FIND_LINK_OVERSIZE, _abi.FIND_LINK_CAPACITY,
                           _abi.FIND_LINK_RELOCATE, _abi.FIND_LINK_QUERIES, _abi.FIND_LINK_ROWS]


def test_validation_needs_no_device():
    """a bad descriptor is refused before the handle is looked at"""
    lib = _lib.load()
    d = _abi.FindLink()
    d.ndim, d.frame_dtype, d.n_frames, d.n_located = 2, _abi.DTYPE_CODES[np.dtype('uint8')], 2, 0
    for a in range(2):
        d.shape[a], d.radius[a], d.separation[a], d.search_range[a] = 32, 2, 5., 4.
    d.isotropic, d.max_queries, d.max_relocated, d.scale_factor, d.capacity = 1, 4, 4, 1., 4
    for f in ('frames', 'threshold', 'frame_offset', 'pos_out', 'frame_offset_out', 'particle', 'mass_out',
              'signal_out', 'size_out', 'relocated', 'n_tracks', 'coupled', 'status'):
        setattr(d, f, 8)      # never dereferenced: the descriptor is refused, or the handle is

    def call(**change):
        e = _abi.FindLink.from_buffer_copy(d)
        for k, v in change.items():
            setattr(e, k, v)
        rc = lib.ctr_find_link_device(None, ctypes.byref(e), None)
        return rc, (lib.ctr_last_error(None) or b'').decode()
    assert call(ndim=4)[0] == _abi.ERR_INVALID
    assert 'max_queries' in call(max_queries=0)[1]
    assert 'max_relocated' in call(max_relocated=2000)[1]
    assert 'capacity' in call(capacity=3)[1]
    assert 'scale_factor' in call(scale_factor=0.)[1]
    assert 'null output' in call(coupled=0)[1]
    rc, msg = call()
    assert rc == _abi.ERR_INVALID and 'null handle' in msg
