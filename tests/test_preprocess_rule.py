"""The preprocessing rule on the CPU: the yardstick tests/_preprocess.py equals
every fixture the reference's own ``lowpass`` / ``preprocess`` wrote, the integer box rule the
device implements (exact window sum, one division, truncation) equals SciPy's in-type
``uniform_filter1d``, the argument checks raise before any GPU call, and
``ctr_preprocess_device`` is declared, exported, mirrored and validated."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.ndimage import uniform_filter1d

import _cases
import _preprocess
import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib

preprocessing = cta.preprocessing      # (AttributeError before the feature)

FIXTURES = _preprocess.fixtures()


def test_fixture_list_covers_the_cases():
    names = [f[0] for f in FIXTURES]
    assert len(names) == len(set(names)) >= 60
    for dt in ('uint8', 'uint16', 'int16', 'int32', 'float32', 'float64'):
        for stem in ('2d_', '2d_axes_', '3d_', '3d_axes_', 'none_2d_', 'sigma0_'):
            assert stem + dt in names
    for n in ('sigma4_u8', 'wide_box_u8', 'wide_box_i16_3d', 'box1_u16', 'threshold_-15_u8', 'slope_uint8',
              'negative_int16', 'row_u8', 'column_u16', 'all_zero_uint8', 'cfg2_crop', 'cfg3_crop'):
        assert n in names
    assert os.path.getsize(_preprocess.GOLDEN) < 1000000


@pytest.mark.parametrize('case', FIXTURES, ids=lambda c: c[0])
def test_yardstick_equals_fixture(case):
    name, raw, kw, expect = case
    with np.errstate(divide='ignore', invalid='ignore'):
        image, scale = _preprocess.preprocess(raw, **kw)
    assert image.dtype == expect['image'].dtype and image.shape == raw.shape
    np.testing.assert_array_equal(np.float64(scale), expect['scale_factor'])
    if np.isfinite(expect['scale_factor']):       # (a dark frame is NaN cast to an integer: undefined)
        np.testing.assert_array_equal(image, expect['image'])
    if kw['noise_size'] is not None:
        band = _preprocess.bandpass(raw, kw['noise_size'], kw['smoothing_size'], kw['threshold'])
        assert band.dtype == np.float64
        np.testing.assert_array_equal(band, expect['bandpass'])
        np.testing.assert_array_equal(_preprocess.lowpass(raw, kw['noise_size']), expect['lowpass'])
        if np.issubdtype(raw.dtype, np.integer):
            # the integer background of the fixture is the exact rule: rebuild the band from it
            ndim = raw.ndim
            lshort = _preprocess.validate_tuple(kw['noise_size'], ndim)
            llong = _preprocess.validate_tuple(kw['smoothing_size'], ndim)
            result = _preprocess._gaussian_chain(raw, lshort) - _preprocess.box_exact(raw, llong)
            thr = 1 if kw['threshold'] is None else kw['threshold']
            np.testing.assert_array_equal(np.where(result >= thr, result, 0), expect['bandpass'])


@pytest.mark.parametrize('dt', [np.uint8, np.uint16, np.int16, np.int32], ids=lambda d: np.dtype(d).name)
def test_box_exact_equals_scipy_in_type(dt):
    rng = np.random.RandomState(np.dtype(dt).itemsize * 7 + (np.dtype(dt).kind == 'i'))
    info = np.iinfo(dt)
    lo, hi = (info.min, info.max) if dt != np.int32 else (-2 ** 31, 2 ** 31 - 1)
    for shape, sizes in (((37, 41), (3, 5)), ((37, 41), (13, 21)), ((9, 11), (25, 7)), ((6, 9, 10), (3, 5, 13)),
                         ((1, 30), (5, 9)), ((64, 50), (1, 31))):
        for _ in range(4):
            im = rng.randint(lo, hi + 1, size=shape, dtype=np.int64).astype(dt)
            expect = im.copy()
            for axis, s in enumerate(sizes):
                if s > 1:
                    uniform_filter1d(expect, s, axis, output=expect, mode='nearest', cval=0)
            np.testing.assert_array_equal(_preprocess.box_exact(im, sizes), expect)
            np.testing.assert_array_equal(_preprocess.boxcar(im, sizes), expect)


def test_gaussian_kernel_is_the_yardsticks():
    for sigma in (0.1, 0.5, 1, 1.5, 2.7, 4):
        a, b = preprocessing.gaussian_kernel(sigma), _preprocess.gaussian_kernel(sigma)
        assert a.tobytes() == b.tobytes() and len(a) == 2 * int(4 * sigma + 0.5) + 1
        np.testing.assert_array_equal(a, a[::-1])       # exactly symmetric: SciPy takes its symmetric branch


def test_value_errors_before_any_gpu_call(monkeypatch):
    """even box, box not above the noise size, wrong tuple length: raised by the yardstick and by
    the package, by the package before it asks for an engine"""
    def no_engine(device=0):
        raise AssertionError("the engine was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, 'default_engine', no_engine)
    im = np.zeros((12, 12), np.uint8)
    for lshort, llong in ((1, 6), ((1, 1), (7, 4)), (3, 3), (5, 3), ((1, 2), (3, 1)), (1, 7.5)):
        with pytest.raises(ValueError):
            cta.bandpass(im, lshort, llong)
        with pytest.raises(ValueError):
            cta.preprocess(im, lshort, llong)
        with pytest.raises(ValueError):
            cta.locate(im[None], 5, noise_size=lshort, smoothing_size=llong)
        if llong != 7.5:
            with pytest.raises(ValueError):
                _preprocess.bandpass(im, lshort, llong)
    with pytest.raises(ValueError):
        cta.lowpass(im, (1, 1, 1))
    with pytest.raises(ValueError):
        cta.bandpass(im, 1, (5, 5, 5))
    with pytest.raises(ValueError):
        cta.locate(im[None], 6, noise_size=1)       # smoothing_size defaults to the separation: even
    with pytest.raises(ValueError):
        cta.lowpass(np.zeros(12, np.uint8), 1)      # one axis


def test_symbol_and_constants():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert 'int ctr_preprocess_device(ctr_handle* h, const ctr_preprocess* p, void* hip_stream);' in header
    assert 'ctr_preprocess_device' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'ctr_preprocess_device')
    assert '#define CTR_ABI_VERSION 8' in header and _abi.ABI_VERSION == 8     # an addition, not a new ABI
    for name, value in (('CTR_PRE_LOWPASS', _abi.PRE_LOWPASS), ('CTR_PRE_BANDPASS', _abi.PRE_BANDPASS),
                        ('CTR_PRE_PREPROCESS', _abi.PRE_PREPROCESS), ('CTR_PRE_SCALE', _abi.PRE_SCALE),
                        ('CTR_PRE_AUTO', _abi.PRE_AUTO), ('CTR_PRE_BAND_PLANE', _abi.PRE_BAND_PLANE),
                        ('CTR_PRE_TWICE', _abi.PRE_TWICE)):
        assert '%s = %d' % (name, value) in header


def test_struct_layout_matches_header(tmp_path):
    """ctypes mirror of ctr_preprocess vs the C compiler's view of include/ctrefine.h"""
    fields = [f[0] for f in _abi.Preprocess._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu\\n", sizeof(ctr_preprocess));\n'
    for f in fields:
        src += 'printf("%%zu\\n", offsetof(ctr_preprocess, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == ctypes.sizeof(_abi.Preprocess)
    assert out[1:] == [getattr(_abi.Preprocess, f).offset for f in fields]


def _descriptor():
    d = _abi.Preprocess()
    d.ndim, d.frame_dtype, d.n_frames = 2, 0, 1
    d.shape[0], d.shape[1] = 32, 40
    d.mode, d.strategy = _abi.PRE_PREPROCESS, _abi.PRE_AUTO
    for a in range(2):
        d.n_taps[a], d.box[a], d.taps[a] = 9, 13, 64
    d.threshold = 1.
    d.frames = d.out = d.scale_factor = 64     # never dereferenced: there is no handle
    return d


def test_descriptor_is_checked_without_a_device():
    """a bad descriptor is refused before the handle is looked at; a good one reaches the handle"""
    lib = _lib.load()
    call = lambda d: lib.ctr_preprocess_device(None, ctypes.byref(d), None)
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()
    assert call(_descriptor()) == _abi.ERR_INVALID and 'null handle' in msg()

    def bad(code, word, **kw):
        d = _descriptor()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        assert call(d) == code, kw
        assert word in msg(), (kw, msg())
    bad(_abi.ERR_INVALID, 'ndim', ndim=4)
    bad(_abi.ERR_INVALID, 'dtype', frame_dtype=6)
    bad(_abi.ERR_INVALID, 'mode', mode=4)
    bad(_abi.ERR_INVALID, 'strategy', strategy=3)
    bad(_abi.ERR_INVALID, 'n_taps', n_taps=(1, 8))
    bad(_abi.ERR_INVALID, 'taps', taps=(0, None))
    bad(_abi.ERR_INVALID, 'box', box=(0, 12))
    bad(_abi.ERR_INVALID, 'shape', shape=(1, 0))
    bad(_abi.ERR_INVALID, 'threshold', threshold=float('nan'))
    bad(_abi.ERR_INVALID, 'float frames', mode=_abi.PRE_SCALE)
    bad(_abi.ERR_INVALID, 'scale_factor', scale_factor=None)
    d = _descriptor()                 # a halo that no tile of 64 KiB holds
    d.frame_dtype = 5
    d.shape[0] = d.shape[1] = 4096
    d.box[0] = d.box[1] = 2001
    assert call(d) == _abi.ERR_UNSUPPORTED and 'LDS' in msg()


def test_reference_regenerates_the_fixtures(tmp_path):
    """with the reference present, its own functions write the committed file again, bit for bit"""
    import refshim
    if not refshim.available():
        pytest.skip('the reference is not on this machine')
    gen = os.path.join(_cases.ROOT, 'tests', 'golden', 'make_golden_preprocess.py')
    code = ("import sys, runpy, numpy as np; out = sys.argv[1]; save = np.savez_compressed; "
            "np.savez_compressed = lambda path, **kw: save(out, **kw); "
            "runpy.run_path(%r, run_name='__main__')" % gen)
    out = str(tmp_path / 'again.npz')
    subprocess.check_call([sys.executable, '-c', code, out], stdout=subprocess.DEVNULL)
    a, b = np.load(out), np.load(_preprocess.GOLDEN)
    assert sorted(a.files) == sorted(b.files)
    for k in b.files:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
