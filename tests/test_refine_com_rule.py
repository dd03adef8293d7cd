"""Centre-of-mass refinement, the rule: known answers of the yardstick
(tests/_refine_com.py), the C interface (header, ABI, ``_abi.RefineCom``, validation without a
device) and the constructed pair of videos on which the refinement decides whether a track
continues (tests/_find_link_refine.py).  No device."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np

import _cases
import _find_link as F
import _find_link_refine as R
import _refine_com as RC
import clustertracking_amd as cta
from clustertracking_amd import _abi, _lib

refine_com = importlib.import_module('clustertracking_amd.refine_com')    # (the package's attribute is the function)


def spot(shape, centre, dtype=np.uint8, peak=200.):
    """a Gaussian spot, symmetric about the pixel ``centre``"""
    grid = np.indices(shape).astype(np.float64)
    r2 = sum((g - c) ** 2 for g, c in zip(grid, centre))
    im = peak * np.exp(-r2 / 4.)
    return np.round(im).astype(dtype) if np.dtype(dtype).kind in 'ui' else im.astype(dtype)


def test_symmetric_spot_on_a_pixel_centre():
    pos, mass, n_iter, offs, clipped = RC.refine_one(spot((32, 40), (15, 20)), (15, 20), (4, 4))
    assert n_iter == 1 and not clipped and np.all(offs[0] == 0) and pos.tolist() == [15., 20.]
    im = spot((32, 40), (15, 20))
    assert mass == float((RC.mask_of((4, 4)) * im[11:20, 16:25].astype(np.int64)).sum())


def test_three_pixels_off_walks_in_four_windows():
    im = spot((32, 40), (15, 20))
    pos, mass, n_iter, offs, clipped = RC.refine_one(im, (15, 23), (4, 4))
    assert n_iter == 4 and pos.tolist() == [15., 20.]
    assert [o[1] < -0.6 for o in offs] == [True, True, True, False] and all(o[0] == 0 for o in offs)
    # the start is rounded half to even
    assert RC.refine_one(im, (14.5, 22.5), (4, 4))[0].tolist() == [15., 20.]       # (14, 22)
    assert RC.refine_one(im, (15.5, 23.5), (4, 4))[2] == 5                         # (16, 24): 4 moves


def test_start_outside_is_clipped():
    im = spot((32, 40), (5, 6))
    pos, mass, n_iter, offs, clipped = RC.refine_one(im, (-3, 1), (4, 4))     # clipped to (4, 4)
    assert clipped and pos.tolist() == [5., 6.] and n_iter == 3
    # a feature closer to the edge than the radius: the window stays in the frame, the centre of
    # mass of what it sees is returned
    im = spot((32, 40), (1, 38))
    pos, mass, n_iter, offs, clipped = RC.refine_one(im, (1, 38), (4, 4))
    assert clipped and n_iter == 10 and pos[0] < 4 and pos[1] > 35      # off beyond the threshold, no room to move


def test_all_zero_window():
    im = np.zeros((32, 40), dtype=np.uint16)
    pos, mass, n_iter, offs, clipped = RC.refine_one(im, (2.2, 50.7), (3, 3))
    assert pos.tolist() == [3., 36.] and mass == 0. and n_iter == 1 and clipped
    p, m, n = RC.refine_one(im.astype(np.float64), (10, 10), (3, 3))[:3]
    assert p.tolist() == [10., 10.] and m == 0. and n == 1


def test_max_iterations_returns_the_last_evaluated_window():
    im = spot((32, 40), (15, 20))
    pos, mass, n_iter, offs, clipped = RC.refine_one(im, (15, 23), (4, 4), max_iterations=2)
    # windows at x = 23 and 22 were evaluated: the result is the second window's, centred on 22,
    # not on 21 where the next one would have been
    assert n_iter == 2 and len(offs) == 2
    assert pos[1] == offs[1][1] + 22 and offs[1][1] < -0.6
    assert mass == float((RC.mask_of((4, 4)) * im[11:20, 18:27].astype(np.int64)).sum())


def test_offset_equal_to_the_threshold_neither_stops_nor_moves():
    im = np.zeros((16, 16), dtype=np.uint8)
    im[8, 8] = im[8, 9] = 100          # k = 0 and k = 1: off = 0.5 exactly
    for max_iterations in (3, 10):
        pos, mass, n_iter, offs, clipped = RC.refine_one(im, (8, 8), (3, 3), max_iterations, shift_thresh=0.5)
        assert n_iter == max_iterations and all(o.tolist() == [0., 0.5] for o in offs)
        assert pos.tolist() == [8., 8.5] and mass == 200.
    assert RC.refine_one(im, (8, 8), (3, 3), shift_thresh=0.6)[2] == 1


def test_3d_anisotropic_radius():
    im = np.zeros((12, 20, 20), dtype=np.uint16)
    im[5, 9, 10] = 1000
    im[7, 9, 10] = 1000          # beyond the radius of 1 along z from z = 5, within it from z = 6
    im[5, 12, 10] = im[5, 6, 10] = 500       # k = (0, +-3, 0): on the edge of the mask, inside
    im[5, 12, 11] = 700          # k = (0, 3, 1): outside
    mask = RC.mask_of((1, 3, 3))
    assert mask.shape == (3, 7, 7) and mask[1, 6, 3] and not mask[1, 6, 4] and not mask[0, 6, 3]
    pos, mass, n_iter, offs, clipped = RC.refine_one(im, (5, 9, 10), (1, 3, 3))
    assert n_iter == 1 and mass == 2000. and pos.tolist() == [5., 9., 10.]
    pos, mass, n_iter, offs, clipped = RC.refine_one(im, (6, 9, 10), (1, 3, 3))
    assert n_iter == 1 and mass == 2000. and pos.tolist() == [6., 9., 10.]      # (-1, +-3, 0) is outside
    im[5, 12, 10] = 0            # 500 on one side only: off_y = -1.5 / 1.5 ... the window walks along y
    pos, mass, n_iter, offs, clipped = RC.refine_one(im, (5, 9, 10), (1, 3, 3))
    assert n_iter == 2 and offs[0].tolist() == [0., -1., 0.] and pos.tolist() == [5., 8., 10.] and mass == 1500.


def test_compose_frames_and_offsets():
    frames = np.stack([spot((32, 40), (15, 20)), np.zeros((32, 40), np.uint8), spot((32, 40), (10, 30))])
    r = RC.compose(frames, [[15, 21], [16, 20], [11, 31]], [0, 2, 2, 3], (4, 4))
    assert r['pos'].tolist() == [[15., 20.], [15., 20.], [10., 30.]] and r['n_iter'].tolist() == [2, 2, 2]
    assert r['n_iter'].dtype == np.int32 and RC.min_gap(r['offs']) > 1e-9


# ---- the C interface ------------------------------------------------------------------------------
def test_header_declares_and_library_exports():
    header = open(os.path.join(_cases.ROOT, 'include', 'ctrefine.h')).read()
    assert re.search(r'\bint\s+ctr_refine_com_device\s*\(\s*ctr_handle\s*\*\s*h,\s*const\s+ctr_refine_com\s*\*', header)
    assert re.search(r'\bint\s+ctr_find_link_refine_device\s*\(\s*ctr_handle\s*\*\s*h,\s*const\s+ctr_find_link\s*\*\s*f,'
                     r'\s*const\s+ctr_refine_com\s*\*', header)
    assert 'typedef struct ctr_refine_com' in header
    assert re.search(r'#define\s+CTR_ABI_VERSION\s+8\b', header) and _abi.ABI_VERSION == 8
    lib = _lib.load()
    assert lib.ctr_abi_version() == 8
    for name in ('ctr_refine_com_device', 'ctr_find_link_refine_device'):
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS and hasattr(lib, name)
    assert {'refine_com', 'refine_com_arrays'} <= set(cta.__all__)
    assert cta.refine_com is refine_com.refine_com and cta.refine_com_arrays is refine_com.refine_com_arrays


def test_refine_com_struct_layout_matches_header(tmp_path):
    """ctypes mirror of ctr_refine_com vs the C compiler's view of include/ctrefine.h; ctr_find_link is
    where it was"""
    fields = [f[0] for f in _abi.RefineCom._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ctrefine.h"\nint main(void){\n'
    src += 'printf("%zu %zu\\n", sizeof(ctr_refine_com), sizeof(ctr_find_link));\n'
    for f in fields:
        src += 'printf("%%zu\\n", offsetof(ctr_refine_com, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(_cases.ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == ctypes.sizeof(_abi.RefineCom) and out[1] == ctypes.sizeof(_abi.FindLink)
    assert out[2:] == [getattr(_abi.RefineCom, f).offset for f in fields]
    assert fields == ['ndim', 'frame_dtype', 'n_frames', 'shape', 'radius', 'max_iterations', 'reserved0',
                      'shift_thresh', 'frames', 'n_features', 'frame_offset', 'pos', 'pos_out', 'mass', 'n_iter']


def _com(**change):
    d = refine_com.descriptor((32, 40), np.uint8, 2, (3, 3))
    d.n_features = 1
    for f in ('frames', 'frame_offset', 'pos', 'pos_out', 'mass', 'n_iter'):
        setattr(d, f, 8)      # never dereferenced: the descriptor is refused, or the handle is
    for k, v in change.items():
        setattr(d, k, v)
    return d


def _find_link_descriptor():
    d = _abi.FindLink()
    d.ndim, d.frame_dtype, d.n_frames, d.n_located = 2, _abi.DTYPE_CODES[np.dtype('uint8')], 2, 0
    for a in range(2):
        d.shape[a], d.radius[a], d.separation[a], d.search_range[a] = (32, 40)[a], 3, 7., 4.
    d.isotropic, d.max_queries, d.max_relocated, d.scale_factor, d.capacity = 1, 4, 4, 1., 4
    for f in ('frames', 'threshold', 'frame_offset', 'pos_out', 'frame_offset_out', 'particle', 'mass_out',
              'signal_out', 'size_out', 'relocated', 'n_tracks', 'coupled', 'status'):
        setattr(d, f, 8)
    return d


def test_validation_needs_no_device():
    """a bad descriptor is refused before the handle is looked at, under the entry point's name"""
    lib = _lib.load()
    msg = lambda: (lib.ctr_last_error(None) or b'').decode()     # noqa: E731

    def call(**change):
        return lib.ctr_refine_com_device(None, ctypes.byref(_com(**change)), None), msg()
    assert lib.ctr_refine_com_device(None, None, None) == _abi.ERR_INVALID and 'null descriptor' in msg()
    rc, m = call(ndim=4)
    assert rc == _abi.ERR_INVALID and m.startswith('ctr_refine_com_device: ') and 'ndim' in m
    for bad in (0, 101):
        rc, m = call(max_iterations=bad)
        assert rc == _abi.ERR_INVALID and 'max_iterations' in m
    for bad in (0., -1., float('nan')):
        rc, m = call(shift_thresh=bad)
        assert rc == _abi.ERR_INVALID and 'shift_thresh' in m
    wide = _com()
    wide.radius[0] = 16         # 33 rows of window in a frame of 32
    assert lib.ctr_refine_com_device(None, ctypes.byref(wide), None) == _abi.ERR_INVALID and 'radius' in msg()
    zero = _com()
    zero.radius[1] = 0
    assert lib.ctr_refine_com_device(None, ctypes.byref(zero), None) == _abi.ERR_INVALID and 'radius' in msg()
    assert 'null output' in call(n_iter=0)[1]
    rc, m = call()
    assert rc == _abi.ERR_INVALID and m == 'ctr_refine_com_device: null handle'
    for bad in (1, 100):
        assert call(max_iterations=bad)[1].endswith('null handle')


def test_find_link_refine_validation_needs_no_device():
    lib = _lib.load()
    f = _find_link_descriptor()

    def call(com, fl=f):
        rc = lib.ctr_find_link_refine_device(None, ctypes.byref(fl), None if com is None else ctypes.byref(com), None)
        return rc, (lib.ctr_last_error(None) or b'').decode()
    good = _com(n_features=0, frame_offset=0, pos=0, pos_out=0, mass=0, n_iter=0)     # its table is ignored
    rc, m = call(good)
    assert rc == _abi.ERR_INVALID and m == 'ctr_find_link_refine_device: null handle'
    assert call(None)[0] == _abi.ERR_INVALID and 'null' in call(None)[1] and 'null handle' not in call(None)[1]
    other = _com()
    other.radius[1] = 2
    rc, m = call(other)
    assert rc == _abi.ERR_INVALID and 'radius' in m and 'differs' in m
    other = _com()
    other.shape[0] = 31
    assert 'shape' in call(other)[1]
    assert 'n_frames' in call(_com(n_frames=3))[1]
    three = refine_com.descriptor((8, 32, 40), np.uint8, 2, (3, 3, 3))
    assert 'ndim' in call(three)[1]
    assert 'max_iterations' in call(_com(max_iterations=0))[1]
    assert 'frames' in call(_com(frames=0))[1]
    # the find-link descriptor's own checks come first, and are the ones of ctr_find_link_device
    bad = _abi.FindLink.from_buffer_copy(f)
    bad.max_queries = 0
    assert 'max_queries' in call(good, bad)[1]
    # a radius of 0 is fine for find_link and refused with the refinement
    flat, com0 = _abi.FindLink.from_buffer_copy(f), _com()
    flat.radius[0] = com0.radius[0] = 0
    assert lib.ctr_find_link_device(None, ctypes.byref(flat), None) == _abi.ERR_INVALID
    assert (lib.ctr_last_error(None) or b'').decode().endswith('null handle')
    assert 'radius must be >= 1' in call(com0, flat)[1]


def test_python_arguments():
    import pytest
    for bad in (0, 101, 2.5):
        with pytest.raises(ValueError):
            refine_com.check_arguments(bad, 0.6)
    for bad in (0, -0.1, float('nan')):
        with pytest.raises(ValueError):
            refine_com.check_arguments(10, bad)
    assert refine_com.check_arguments(10., 1) == (10, 1.)
    assert (refine_com.MAX_ITERATIONS, refine_com.SHIFT_THRESH) == (RC.MAX_ITERATIONS, RC.SHIFT_THRESH) == (10, 0.6)
    with pytest.raises(ValueError):
        refine_com.descriptor((32, 40), np.uint8, 1, (2.5, 2))


# ---- the constructed pair ---------------------------------------------------------------------------
def test_a_track_that_continues_only_with_refinement():
    frames, kw = R.pair_cases()['only_with']
    plain, refined = F.find_link(frames, **kw), R.find_link(frames, **kw)
    assert plain['pos'].tolist() == [[12., 20.], [12., 24.]] and refined['start'].tolist() == plain['pos'].tolist()
    assert refined['n_iter'].tolist() == [1, 1] and not refined['relocated'].any() and not plain['relocated'].any()
    assert abs(refined['pos'][0, 1] - 20.45) < 0.001 and refined['pos'][0, 0] == 12.
    assert kw['search_range'] == 3.9
    assert plain['particle'].tolist() == [0, 1] and plain['n_tracks'] == 2           # 4 whole pixels: lost
    assert refined['particle'].tolist() == [0, 0] and refined['n_tracks'] == 1       # 3.55 from the centre of mass


def test_a_track_that_continues_only_without_refinement():
    frames, kw = R.pair_cases()['only_without']
    plain, refined = F.find_link(frames, **kw), R.find_link(frames, **kw)
    assert plain['pos'].tolist() == [[12., 20.], [14., 23.]] and refined['start'].tolist() == plain['pos'].tolist()
    assert abs(refined['pos'][0, 1] - 19.55) < 0.001
    assert plain['particle'].tolist() == [0, 0] and plain['n_tracks'] == 1           # sqrt(13) = 3.61
    assert refined['particle'].tolist() == [0, 1] and refined['n_tracks'] == 2       # sqrt(4 + 3.45^2) = 3.99
