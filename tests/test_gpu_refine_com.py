"""``ctr_refine_com_device`` / ``clustertracking_amd.refine_com_arrays`` on the MI355X against the
yardstick of its rule (tests/_refine_com.py): both group sizes of the kernel (a 16-lane row for 2D
windows up to 17 x 17, the wavefront otherwise), every pixel type, partial groups at the end of a
block, frames without features, the known answers of tests/test_refine_com_rule.py.

Integer frames: pos, mass and n_iter bit for bit (both sides sum exactly).  Float frames: n_iter
exact, pos to 1e-10, mass to rtol 1e-12 -- both sides sum at most 51 * 51 = 2601 non-negative
float64 terms, so a sum is off by at most 2601 * 2^-53 = 3e-13 (relative), the quotient of two by
6e-13, and a window index is at most 50; the inputs are such that the yardstick meets no
``abs(off)`` within 1e-9 of the threshold (asserted), so both sides take the same decisions."""
import numpy as np
import pytest

import _find_link as F
import _refine_com as RC
import clustertracking_amd as cta
from clustertracking_amd.find import locate_arrays

pytestmark = pytest.mark.gpu

COUNTS = (1, 15, 16, 17, 300)
# (name, shape, radius): radii 2, 6 and 8 take a 16-lane row per feature, 9 and 3D the wavefront
GEOMETRY = [('2d_r2', (48, 56), (2, 2)), ('2d_r6', (48, 56), (6, 6)), ('2d_r8', (48, 56), (8, 8)),
            ('2d_r9', (48, 56), (9, 9)), ('3d_r233', (16, 24, 24), (2, 3, 3))]
DTYPES = ('uint8', 'uint16', 'float32', 'float64')
_cache = {}


def case(shape, radius, dtype):
    """(frames [3, *shape], starts [300, ndim], frame_offset with an empty frame, the yardstick's
    result), computed once"""
    key = (shape, radius, dtype)
    if key not in _cache:
        seed = 4000 + 10 * [g[1:] for g in GEOMETRY].index((shape, radius)) + DTYPES.index(dtype)
        made = 'float64' if dtype == 'float32' else dtype
        if len(shape) == 2:
            frames = F.video(shape, 3, 8, seed, made, walkers=0.3)
        else:
            frames = F.video(shape, 3, 4, seed, made, size=(1.3, 1.7, 1.7), drift=1., walkers=0.3, margin=(2, 3, 3))
        frames = frames.astype(dtype)
        rng = np.random.RandomState(seed)
        # starts all over the frame and up to 3 pixels beyond it (clipped), some on a half (rounded to even)
        starts = np.stack([rng.uniform(-3, n + 2, 300) for n in shape], axis=1)
        # ... every third near a bright pixel of its frame: the window walks
        for i in range(0, 300, 3):
            f = frames[0 if i < 140 else 2]
            bright = np.argwhere(f >= np.percentile(f, 98))
            starts[i] = bright[rng.randint(len(bright))] + rng.uniform(-3, 3, len(shape))
        starts[::7] = np.floor(starts[::7]) + 0.5
        starts[::5] = np.floor(starts[::5])
        offset = np.array([0, 140, 140, 300])     # frame 1 has no feature
        want = RC.compose(frames, starts, offset, radius)
        _cache[key] = frames, starts, offset, want
    return _cache[key]


def compare(got, want, rows, integer):
    pos, mass, n_iter = got
    assert pos.dtype == np.float64 and mass.dtype == np.float64 and n_iter.dtype == np.int32
    assert np.array_equal(n_iter, want['n_iter'][rows])
    if integer:
        assert np.array_equal(pos, want['pos'][rows]) and np.array_equal(mass, want['mass'][rows])
    else:
        np.testing.assert_allclose(pos, want['pos'][rows], rtol=0, atol=1e-10)
        np.testing.assert_allclose(mass, want['mass'][rows], rtol=1e-12, atol=0)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geometry', GEOMETRY, ids=[g[0] for g in GEOMETRY])
def test_device_equals_the_yardstick(engine, geometry, dtype):
    name, shape, radius = geometry
    frames, starts, offset, want = case(shape, radius, dtype)
    integer = np.dtype(dtype).kind in 'ui'
    if not integer:
        gap = RC.min_gap(want['offs'])
        print('%s %s: smallest | |off| - shift_thresh | = %.3g' % (name, dtype, gap))
        assert gap > 1e-9
    # what the cases are there for: walks, clipped starts, windows that stay
    assert (want['n_iter'] >= 2).sum() >= 20 and want['clipped'].sum() >= 20 and (want['n_iter'] == 1).sum() >= 20
    for n in COUNTS:
        got = cta.refine_com_arrays(frames, starts[:n], np.minimum(offset, n), radius)
        compare(got, want, slice(0, n), integer)


def test_limits_of_the_loop(engine):
    """max_iterations and shift_thresh reach the kernel"""
    frames, starts, offset, _ = case((48, 56), (6, 6), 'uint8')
    for max_iterations, shift_thresh in ((1, 0.6), (2, 0.6), (100, 0.6), (10, 0.3), (10, 1.5)):
        want = RC.compose(frames, starts, offset, (6, 6), max_iterations, shift_thresh)
        got = cta.refine_com_arrays(frames, starts, offset, (6, 6), max_iterations, shift_thresh)
        compare(got, want, slice(None), True)
        assert want['n_iter'].max() <= max_iterations
    frames, starts, offset, _ = case((16, 24, 24), (2, 3, 3), 'float64')
    want = RC.compose(frames, starts, offset, (2, 3, 3), 3, 0.45)
    assert RC.min_gap(want['offs'], 0.45) > 1e-9
    compare(cta.refine_com_arrays(frames, starts, offset, (2, 3, 3), 3, 0.45), want, slice(None), False)


def spot(shape, centre, dtype=np.uint8):
    grid = np.indices(shape).astype(np.float64)
    im = 200. * np.exp(-sum((g - c) ** 2 for g, c in zip(grid, centre)) / 4.)
    return np.round(im).astype(dtype)


def test_known_answers(engine):
    im = spot((32, 40), (15, 20))
    r = cta.refine_com(im, [[15, 20], [15, 23], [14.5, 22.5], [-3, 90]], 4)
    assert r.shape == (4, 3)
    assert r[:3, :2].tolist() == [[15., 20.]] * 3 and len(set(r[:3, 2])) == 1
    pos, mass, n_iter = cta.refine_com_arrays(im[None], [[15, 20], [15, 23], [-3, 90]], [0, 3], (4, 4))
    assert n_iter.tolist() == [1, 4, 1] and pos[2].tolist() == [4., 35.] and mass[2] == 0.      # clipped, all zero
    # max_iterations = 2 on the 3-pixel walk: the second window's centre of mass, not the moved one
    pos, mass, n_iter = cta.refine_com_arrays(im[None], [[15, 23]], [0, 1], (4, 4), max_iterations=2)
    w = RC.refine_one(im, (15, 23), (4, 4), max_iterations=2)
    assert n_iter.tolist() == [2] and pos[0].tolist() == w[0].tolist() and mass[0] == w[1] and pos[0, 1] < 21.4
    # an offset exactly on the threshold neither stops nor moves
    eq = np.zeros((16, 16), dtype=np.uint8)
    eq[8, 8] = eq[8, 9] = 100
    for dtype in (np.uint8, np.float32, np.float64):
        pos, mass, n_iter = cta.refine_com_arrays(eq.astype(dtype)[None], [[8, 8]], [0, 1], (3, 3), 7, 0.5)
        assert n_iter.tolist() == [7] and pos.tolist() == [[8., 8.5]] and mass.tolist() == [200.]
    # an all-zero window of a float frame: the clipped start, mass 0
    pos, mass, n_iter = cta.refine_com_arrays(np.zeros((1, 16, 16)), [[2.2, 50.7]], [0, 1], (3, 3))
    assert pos.tolist() == [[3., 12.]] and mass.tolist() == [0.] and n_iter.tolist() == [1]
    # 3D, anisotropic radius
    im3 = np.zeros((12, 20, 20), dtype=np.uint16)
    im3[5, 9, 10] = im3[7, 9, 10] = 1000
    im3[5, 6, 10] = 500
    im3[5, 12, 11] = 700
    pos, mass, n_iter = cta.refine_com_arrays(im3[None], [[5, 9, 10], [6, 9, 10]], [0, 2], (1, 3, 3))
    assert pos.tolist() == [[5., 8., 10.], [6., 9., 10.]] and mass.tolist() == [1500., 2000.] and n_iter.tolist() == [2, 1]


def test_arrays_in_arrays_out_tensors_in_tensors_out(engine):
    import torch
    for shape, radius, dtype in (((48, 56), (6, 6), 'uint16'), ((16, 24, 24), (2, 3, 3), 'float32')):
        frames, starts, offset, want = case(shape, radius, dtype)
        a = cta.refine_com_arrays(frames, starts, offset, radius)
        assert all(isinstance(x, np.ndarray) for x in a)
        host = frames.view(np.int16) if frames.dtype == np.uint16 else frames       # uint16 travels as int16
        t = torch.from_numpy(host).cuda()
        b = cta.refine_com_arrays(t, torch.from_numpy(starts).cuda(), torch.from_numpy(offset).cuda(), radius,
                                  dtype=frames.dtype)
        assert all(isinstance(x, torch.Tensor) and x.device == t.device for x in b)
        for x, y in zip(a, b):
            assert x.tobytes() == y.cpu().numpy().tobytes()
        # int32 positions, as locate_arrays returns them
        whole = np.floor(starts).astype(np.int32)
        c = cta.refine_com_arrays(t, torch.from_numpy(whole).cuda(), torch.from_numpy(offset).cuda(), radius,
                                  dtype=frames.dtype)
        d = cta.refine_com_arrays(frames, whole.astype(np.float64), offset, radius)
        for x, y in zip(c, d):
            assert x.cpu().numpy().tobytes() == y.tobytes()


def test_chains_from_locate_arrays(engine):
    name, frames, kw = F.random_cases()[0]
    pos, off, thr = locate_arrays(frames, kw['separation'])
    got = cta.refine_com_arrays(frames, pos, off, 4)
    want = RC.compose(frames, pos, off, (4, 4))
    compare(got, want, slice(None), True)
    assert len(pos) > 20


def test_refused_arguments(engine):
    frames, starts, offset, _ = case((48, 56), (6, 6), 'uint8')
    bad = starts.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        cta.refine_com_arrays(frames, bad, offset, 6)
    with pytest.raises(ValueError, match='radius'):
        cta.refine_com_arrays(frames, starts, offset, (24, 6))      # 49 rows of window, 48 of frame
    with pytest.raises(ValueError, match='radius'):
        cta.refine_com_arrays(frames, starts, offset, (0, 6))
    with pytest.raises(ValueError, match='max_iterations'):
        cta.refine_com_arrays(frames, starts, offset, 6, max_iterations=0)
    with pytest.raises(ValueError, match='shift_thresh'):
        cta.refine_com_arrays(frames, starts, offset, 6, shift_thresh=0)
    with pytest.raises(ValueError, match='frame_offset'):
        cta.refine_com_arrays(frames, starts, [0, 140, 300], 6)
    empty = cta.refine_com_arrays(frames, np.zeros((0, 2)), [0, 0, 0, 0], 6)
    assert [x.shape for x in empty] == [(0, 2), (0,), (0,)]
    # the call after the refusals computes
    got = cta.refine_com_arrays(frames, starts[:16], np.minimum(offset, 16), 6)
    compare(got, case((48, 56), (6, 6), 'uint8')[3], slice(0, 16), True)
