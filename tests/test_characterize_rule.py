"""The characterisation rule without a GPU: the NumPy yardstick of
tests/_characterize.py equals the reference's recorded results on every fixture, and the C-ABI of
``ctr_characterize_device`` is declared, exported, mirrored and validated."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _cases
import _characterize
import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.parametrize('case', _characterize.fixtures(), ids=lambda c: c[0])
def test_yardstick_equals_fixture(case):
    name, image, coords, kw, expect = case
    got = _characterize.compose(coords, image, **kw)
    assert list(got) == list(expect)
    np.testing.assert_array_equal(got['mass'], expect['mass'])
    np.testing.assert_array_equal(got['signal'], expect['signal'])
    for key in _characterize.size_keys(image.ndim, kw['isotropic']):
        assert got[key].dtype == np.float64 and got[key].shape == expect[key].shape
        np.testing.assert_array_equal(np.isnan(got[key]), np.isnan(expect[key]))
        if image.dtype.kind in 'ui':
            np.testing.assert_array_equal(got[key], expect[key])
        else:
            np.testing.assert_allclose(got[key], expect[key], rtol=1e-12, atol=0)


def test_fixtures_cover_the_rule():
    """what the fixtures are there for is in them"""
    fx = _characterize.fixtures()
    assert {np.dtype(d) for d in ('uint8', 'uint16', 'int16', 'int32', 'float32', 'float64')} == {c[1].dtype for c in fx}
    assert {(c[1].ndim, c[3]['isotropic']) for c in fx} == {(2, True), (2, False), (3, True), (3, False)}
    assert any(np.isnan(v).any() for c in fx for k, v in c[4].items() if k.startswith('size'))
    assert any(c[3]['scale_factor'] != 1 for c in fx)
    assert any(0 in c[3]['radius'] for c in fx) and any(c[3]['radius'] == (1, 1) for c in fx)
    assert any((c[4]['signal'] == 0).all() and (c[4]['mass'] < 0).all() for c in fx)   # negative floats
    assert any((np.asarray(c[1].shape) < 2 * np.asarray(c[3]['radius']) + 1).all() for c in fx)
    assert any((c[2] % 1 == 0.5).any() for c in fx)


def test_header_declares_and_library_exports():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'\bint\s+ctr_characterize_device\s*\(\s*ctr_handle\s*\*', header)
    assert 'typedef struct ctr_characterize' in header
    assert 'ctr_characterize_device' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'ctr_characterize_device')


def test_characterize_struct_layout_matches_header(tmp_path):
    """ctypes mirror of ctr_characterize vs the C compiler's view of include/ctrefine.h"""
    fields = [f[0] for f in _abi.Characterize._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_characterize));\n'
    for f in fields:
        src += 'printf("%%zu\\n", offsetof(ctr_characterize, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == ctypes.sizeof(_abi.Characterize)
    assert out[1:] == [getattr(_abi.Characterize, f).offset for f in fields]


def _descriptor():
    d = _abi.Characterize()
    d.ndim, d.frame_dtype, d.n_frames = 2, _abi.DTYPE_CODES[np.dtype(np.uint8)], 1
    d.shape[0] = d.shape[1] = 16
    d.radius[0] = d.radius[1] = 3
    d.isotropic, d.scale_factor = 1, 1.
    d.n_features = 0
    d.pos = 8          # never read: the descriptor is refused, or there is no feature
    return d


def test_validation_needs_no_device():
    """A bad descriptor is refused before the handle is looked at; the text is the NULL handle's
    last error.  A good descriptor then fails on the NULL handle itself."""
    lib = _lib.load()

    def call(d):
        rc = lib.ctr_characterize_device(None, ctypes.byref(d), None)
        return rc, (lib.ctr_last_error(None) or b'').decode()

    rc, msg = call(_descriptor())
    assert rc == _abi.ERR_INVALID and 'null handle' in msg
    d = _descriptor()
    d.radius[1] = -1
    rc, msg = call(d)
    assert rc == _abi.ERR_INVALID and 'radius' in msg
    d = _descriptor()
    d.pos_i32 = 8
    rc, msg = call(d)
    assert rc == _abi.ERR_INVALID and 'exactly one' in msg
    d = _descriptor()
    d.pos = None
    rc, msg = call(d)
    assert rc == _abi.ERR_INVALID and 'exactly one' in msg
    d = _descriptor()
    d.frame_dtype = 6
    rc, msg = call(d)
    assert rc == _abi.ERR_UNSUPPORTED and 'dtype' in msg
    d = _descriptor()
    d.ndim = 4
    assert call(d)[0] == _abi.ERR_INVALID
    d = _descriptor()
    d.shape[0] = 0
    assert call(d)[0] == _abi.ERR_INVALID
    d = _descriptor()
    d.scale_factor = 0.
    assert call(d)[0] == _abi.ERR_INVALID
    d = _descriptor()
    d.n_features = 3        # features, but no frames / offsets / outputs
    assert call(d)[0] == _abi.ERR_INVALID


def test_margins_that_cover_the_frame_raise():
    frames = np.ones((2, 12, 40), np.uint8)
    with pytest.raises(ValueError):
        cta.locate(frames, 13)                       # margin 6: 12 <= 2 * 6
    with pytest.raises(ValueError):
        cta.locate(frames, 5, diameter=(13, 5))
    with pytest.raises(ValueError):
        cta.locate(frames, 5, margin=(2, 20))
    with pytest.raises(ValueError):
        cta.locate(np.ones((2, 4, 30, 30), np.uint8), (9, 5, 5))    # z: 4 <= 2 * 4


def test_no_cpu_fallback():
    """without a GPU every entry point raises EngineError (with one they run:
    tests/test_gpu_characterize.py)"""
    frame = np.ones((20, 20), np.uint8)
    if _gpu_present():
        assert cta.characterize(np.array([[10., 10.]]), frame, (3, 3))['mass'][0] == 29
        return
    with pytest.raises(_lib.EngineError):
        cta.characterize(np.array([[10., 10.]]), frame, (3, 3))
    with pytest.raises(_lib.EngineError):
        cta.characterize_arrays(frame[None], np.array([[10., 10.]]), [0, 1], (3, 3))
    with pytest.raises(_lib.EngineError):
        cta.locate(frame[None], 5)
