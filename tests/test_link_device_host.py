"""The device linker without a GPU: the C-ABI of ``ctr_link_device`` is declared,
exported, mirrored and validated; the engine switch of ``link`` / ``link_levels``; and the host
linker against the reference's ids on the edge fixtures
(tests/golden/make_golden_link_edges.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest
from numpy.testing import assert_equal

import _cases
import clustertracking_amd as cta
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


def _levels(name):
    offs = np.r_[0, np.cumsum(Z[name + '_counts'])]
    return [Z[name + '_pos'][a:b] for a, b in zip(offs[:-1], offs[1:])]


@pytest.mark.parametrize('name', NAMES)
def test_host_linker_equals_reference_on_edge_fixtures(name):
    ids = lk.link_levels(_levels(name), tuple(Z[name + '_sr']), int(Z[name + '_memory']))
    assert [len(i) for i in ids] == list(Z[name + '_counts'])
    assert_equal(np.concatenate(ids), Z[name + '_ids'])


def test_edge_fixtures_cover_the_edges():
    counts = {n: Z[n + '_counts'] for n in NAMES}
    mem = {n: int(Z[n + '_memory']) for n in NAMES}

    def longest_gap(c):
        best = run = 0
        for a in range(1, len(c)):
            run = run + 1 if c[a] == 0 else 0
            best = max(best, run)
        return best
    assert any(longest_gap(counts[n]) == 1 and mem[n] == 0 for n in NAMES)
    assert any(longest_gap(counts[n]) == 1 and mem[n] == 2 for n in NAMES)
    assert any(longest_gap(counts[n]) == 2 and mem[n] == 2 for n in NAMES)
    assert any(longest_gap(counts[n]) == 3 and mem[n] == 2 for n in NAMES)
    assert any(counts[n][0] == 0 for n in NAMES)
    assert any(len(counts[n]) == 1 for n in NAMES)
    assert any((counts[n] <= 1).all() and len(counts[n]) > 1 for n in NAMES)
    assert any((Z[n + '_pos'] % 1 == 0).all() and len(Z[n + '_pos']) > 100 for n in NAMES)
    assert any(Z[n + '_pos'].shape[1] == 3 for n in NAMES)


def test_header_declares_and_library_exports():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'\bint\s+ctr_link_device\s*\(\s*ctr_handle\s*\*', header)
    assert 'typedef struct ctr_link' in header
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    assert 'ctr_link_device' in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, 'ctr_link_device') and lib.ctr_abi_version() == 8
    assert 'link_arrays' in cta.__all__ and cta.link_arrays is lk.link_arrays


def test_link_struct_layout_matches_header(tmp_path):
    """ctypes mirror of ctr_link vs the C compiler's view of include/ctrefine.h"""
    fields = [f[0] for f in _abi.Link._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_link));\n'
    for f in fields:
        src += 'printf("%%zu\\n", offsetof(ctr_link, %s));\n' % f
    src += 'printf("%d %d %d %d %d\\n", CTR_LINK_OK, CTR_LINK_OVERSIZE, CTR_LINK_CAPACITY, '
    src += 'CTR_LINK_MAX_SOURCES, CTR_LINK_MAX_DESTINATIONS);\n'
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    n = len(fields)
    assert out[0] == ctypes.sizeof(_abi.Link)
    assert out[1:1 + n] == [getattr(_abi.Link, f).offset for f in fields]
    assert out[1 + n:] == [_abi.LINK_OK, _abi.LINK_OVERSIZE, _abi.LINK_CAPACITY,
                           _abi.LINK_MAX_SOURCES, _abi.LINK_MAX_DESTINATIONS]
    assert _abi.LINK_MAX_SOURCES == lk.MAX_SUB_NET_SIZE


def _descriptor(n=0):
    d = _abi.Link()
    d.ndim, d.memory, d.n_levels, d.n_features = 2, 0, 3, n
    d.search_range[0] = d.search_range[1] = 5.
    # never dereferenced: the descriptor is refused, or the handle is
    d.pos = d.frame_offset = d.particle = d.n_tracks = d.status = 8
    return d


def test_validation_needs_no_device():
    """A bad descriptor is refused before the handle is looked at; the text is the NULL handle's
    last error.  A good descriptor then fails on the NULL handle itself."""
    lib = _lib.load()

    def call(d):
        rc = lib.ctr_link_device(None, ctypes.byref(d), None)
        return rc, (lib.ctr_last_error(None) or b'').decode()

    for n in (0, 7):
        rc, msg = call(_descriptor(n))
        assert rc == _abi.ERR_INVALID and 'null handle' in msg
    rc = lib.ctr_link_device(None, None, None)
    assert rc == _abi.ERR_INVALID and b'null descriptor' in lib.ctr_last_error(None)
    for ndim in (1, 4):
        d = _descriptor()
        d.ndim = ndim
        rc, msg = call(d)
        assert rc == _abi.ERR_INVALID and 'ndim' in msg
    for bad in (0., -1., float('nan'), float('inf')):
        d = _descriptor()
        d.search_range[1] = bad
        rc, msg = call(d)
        assert rc == _abi.ERR_INVALID and 'search_range' in msg, bad
    d = _descriptor()
    d.ndim = 3                      # the third axis' range is 0
    assert call(d)[0] == _abi.ERR_INVALID
    d = _descriptor()
    d.memory = -1
    rc, msg = call(d)
    assert rc == _abi.ERR_INVALID and 'memory' in msg
    for field in ('n_levels', 'n_features'):
        d = _descriptor()
        setattr(d, field, -1)
        rc, msg = call(d)
        assert rc == _abi.ERR_INVALID and 'negative' in msg
    for field in ('particle', 'n_tracks', 'status'):
        d = _descriptor(5)
        setattr(d, field, None)
        rc, msg = call(d)
        assert rc == _abi.ERR_INVALID and 'null output' in msg, field
    for field in ('pos', 'frame_offset'):
        d = _descriptor(5)
        setattr(d, field, None)
        assert call(d)[0] == _abi.ERR_INVALID, field
    d = _descriptor(5)
    d.n_levels = 0
    assert call(d)[0] == _abi.ERR_INVALID


def _frame():
    f = pd.DataFrame({'y': [1., 1.5, 2.], 'x': [1., 1.2, 1.4], 'frame': [0, 1, 2]})
    return f


def test_unknown_engine_is_a_value_error():
    with pytest.raises(ValueError):
        lk.link(_frame(), 3, engine='bogus')
    with pytest.raises(ValueError):
        lk.link_levels([np.zeros((1, 2))], 3, engine='gpu')
    with pytest.raises(ValueError):
        lk.link_levels([], 3, engine=None)
    # the default is the host path and needs no device
    assert_equal(lk.link(_frame(), 3)['particle'].values, [0, 0, 0])
    assert_equal(lk.link(_frame(), 3, engine='host')['particle'].values, [0, 0, 0])


@pytest.mark.skipif(_gpu_present(), reason="a GPU is present: tests/test_gpu_link.py runs the device path")
def test_no_cpu_fallback():
    with pytest.raises(_lib.EngineError):
        lk.link(_frame(), 3, engine='device')
    with pytest.raises(_lib.EngineError):
        lk.link_levels([np.zeros((1, 2)), np.zeros((1, 2))], 3, engine='device')
    with pytest.raises(_lib.EngineError):
        cta.link_arrays(np.zeros((2, 2)), [0, 1, 2], 3)
    with pytest.raises(_lib.EngineError):
        cta.link_arrays(np.zeros((0, 2)), [0], 3)
