"""Feature location on the host side (no GPU): the helpers equal the reference's, the test's own
composition reproduces every fixture of the reference's grey_dilation, the ctr_locate mirror
matches the header, and the device path refuses to run without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _cases
import _locate
from clustertracking_amd import _abi, _lib, find


def _reference():
    import refshim
    if not refshim.available():
        pytest.skip("reference not present")
    return refshim.load()


def test_helpers_equal_reference():
    ref = _reference()
    rng = np.random.RandomState(0)
    for trial in range(60):
        ndim = 2 + trial % 2
        n = rng.randint(0, 60)
        pos = rng.randint(0, 40, (n, ndim)).astype(np.int64)
        sep = tuple(rng.choice([3, 5, 6.5, 9], ndim)) if trial % 3 else rng.choice([4, 7])
        inten = rng.randint(0, 4, n).astype(np.uint8)       # many equal values: the tie rules
        ours = find.where_close(pos, sep, inten)
        theirs = ref.find.where_close(pos, sep, inten)
        np.testing.assert_array_equal(np.asarray(ours), np.asarray(theirs))
        out, exp = find.drop_close(pos, sep, inten), ref.find.drop_close(pos, sep, inten)
        assert out.dtype == exp.dtype and out.shape == exp.shape
        np.testing.assert_array_equal(out, exp)
    for dt in (np.uint8, np.int16, np.float32, np.float64):
        for trial in range(10):
            im = (rng.standard_normal((17, 19)) * 40).astype(dt)
            im[rng.rand(17, 19) < 0.3] = 0
            pct = rng.uniform(0, 100)
            a, b = find.percentile_threshold(im, pct), ref.find.percentile_threshold(im, pct)
            assert np.asarray(a).dtype == np.asarray(b).dtype
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert np.isnan(find.percentile_threshold(np.zeros((4, 4)), 50))
    assert find.where_close(np.zeros((0, 2)), 3) == []
    assert find.where_close(np.array([[0, 0], [0, 1]]), (0, 3), [1, 2]) == []


@pytest.mark.parametrize('case', _locate.fixtures(), ids=lambda c: c[0])
def test_composition_reproduces_fixture(case):
    name, frame, kw, expect, thr = case
    got = _locate.compose(frame, **kw)
    assert got.dtype == expect.dtype and got.shape == expect.shape
    np.testing.assert_array_equal(got, expect)
    t = np.float64(find.percentile_threshold(frame, kw['percentile']))
    assert t.tobytes() == np.float64(thr).tobytes() or (np.isnan(t) and np.isnan(thr))


def test_fixture_coverage():
    cases = _locate.fixtures()
    dtypes = {(c[1].dtype.name, c[1].ndim) for c in cases}
    for dt in ('uint8', 'uint16', 'int16', 'int32', 'float32', 'float64'):
        assert (dt, 2) in dtypes and (dt, 3) in dtypes
    assert any(len(c[3]) == 0 and c[3].dtype == np.float64 for c in cases)
    assert os.path.getsize(_locate.GOLDEN) < 1 << 20


def test_locate_struct_layout_matches_header(tmp_path):
    fields = [f[0] for f in _abi.Locate._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_locate));\n'
    for f in fields:
        src += 'printf("%%zu\\n", offsetof(ctr_locate, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == ctypes.sizeof(_abi.Locate)
    assert out[1:] == [getattr(_abi.Locate, f).offset for f in fields]


def test_locate_exported():
    assert 'ctr_locate_maxima_device' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'ctr_locate_maxima_device')


def test_device_path_needs_a_gpu():
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is visible: the device path runs (tests/test_gpu_locate.py)")
    except ImportError:
        pass
    with pytest.raises(_lib.EngineError):
        find.grey_dilation(np.zeros((8, 8), np.uint8), 3)
    with pytest.raises(_lib.EngineError):
        find.locate_maxima(np.zeros((2, 8, 8), np.uint8), 3)
