"""The launch decisions of the four front-end stages (preprocess, locate, characterize, link),
restated in plain Python from the host code that takes them, the cells those decisions fall into,
and one seeded case per cell.  tests/test_frontplan_cells.py checks every case against its cell
without a GPU; tests/test_gpu_frontend_matrix.py runs every case on the device against the stage's
own yardstick.  What tests/_dispatch.py is for the refine kernels.

The engine has no query for these decisions.  The restatement is pinned to it where a decision is
observable: per pixel type, the largest box the restatement fits at ``ty = 1`` is accepted by the
device and the next one raises ``EngineError`` (the ``ty1`` cells of preprocess and locate), and
the link cells at the solver's capacity raise or solve as the restatement says.

Line numbers refer to clustertracking_amd/csrc/.
"""
import collections
import math
import zlib

import numpy as np

DTYPES = (np.uint8, np.uint16, np.int16, np.int32, np.float32, np.float64)
SHORT = {'uint8': 'u8', 'uint16': 'u16', 'int16': 'i16', 'int32': 'i32', 'float32': 'f32', 'float64': 'f64'}
LONG = {v: np.dtype(k) for k, v in SHORT.items()}

Cell = collections.namedtuple('Cell', 'stage name want')      # want: {decision: outcome}


def cell_id(c):
    return '%s/%s' % (c.stage, c.name)


def seed_of(c):
    return zlib.crc32(cell_id(c).encode())


def _tuple(v, ndim):
    return tuple(v) if hasattr(v, '__iter__') else (v,) * ndim


class Case(object):
    """the concrete inputs of one cell (attributes differ per stage)"""

    def __init__(self, cell, **kw):
        self.cell = cell
        self.__dict__.update(kw)


# =============================================================================================
# preprocess: tu_preprocess.hip
# =============================================================================================
PRE_TX, PRE_THREADS, PRE_LDS_MAX = 64, 256, 64 * 1024       # preprocess_kernels.h:16-17, tu_preprocess.hip:18

PrePlan = collections.namedtuple('PrePlan', 'ok ty lds z_gauss z_box gin l h hx bpf')


def n_taps(sigma):
    """taps of preprocessing.gaussian_kernel(sigma, 4); a size <= 0 is the single tap 1"""
    return 2 * int(4.0 * sigma + 0.5) + 1 if sigma > 0 else 1


def pre_lds_bytes(l, h, with_box, ty, pix, gin):
    """tu_preprocess.hip:21-27"""
    gcols, grows = PRE_TX + 2 * l[2], ty + 2 * l[1]
    bcols, brows = PRE_TX + 2 * h[2], ty + 2 * h[1]
    b = 8 * ty * gcols + ((gin * grows * gcols + 7) & ~7)
    if with_box:
        b += pix * (ty * bcols + brows * bcols)
    return b


def pre_plan(shape, dtype, mode, noise=None, smooth=None):
    """mode: 'lowpass' | 'bandpass' | 'preprocess' | 'scale' (tu_preprocess.hip:126-172)"""
    ndim, a0 = len(shape), 3 - len(shape)
    stencil, with_box = mode != 'scale', mode in ('bandpass', 'preprocess')     # :126
    ext, lw, l, h, hx, bs = [1] * 3, [0] * 3, [0] * 3, [0] * 3, [0] * 3, [1] * 3
    noise = _tuple(noise, ndim) if stencil else None
    smooth = _tuple(smooth, ndim) if with_box else None
    E = 1
    for i in range(ndim):                                                        # :133-151
        a = a0 + i
        ext[a] = int(shape[i])
        E *= int(shape[i])
        if not stencil:
            continue
        lw[a] = n_taps(noise[i]) // 2                                           # :143
        l[a] = min(lw[a], ext[a] - 1)                                           # :144
        if not with_box:
            continue
        bs[a] = max(int(smooth[i]), 1)                                          # preprocessing._box; :148
        h[a] = min(bs[a] // 2, ext[a] - 1)                                      # :149
        hx[a] = bs[a] // 2 - h[a]                                               # :150
    z_gauss, z_box = stencil and lw[0] > 0, with_box and bs[0] > 1              # :163
    pix = np.dtype(dtype).itemsize
    gin = 8 if z_gauss else pix                                                 # :165
    ty, lds, ok = 16, 0, True                                                   # :166
    if stencil:
        while ty > 1 and pre_lds_bytes(l, h, with_box, ty, pix, gin) > PRE_LDS_MAX:     # :168
            ty //= 2
        lds = pre_lds_bytes(l, h, with_box, ty, pix, gin)
        ok = lds <= PRE_LDS_MAX                                                 # :169
    bpf = min(256, max(1, E // (PRE_THREADS * 8))) if mode == 'scale' else None  # :54
    return PrePlan(ok, ty, lds, z_gauss, z_box, gin, tuple(l), tuple(h), tuple(hx), bpf)


Z_PAIRS = {   # (z_gauss, z_box) -> (noise, smoothing z) of a stack; y and x sizes are appended
    'TT': (1, 3), 'TF': (0.5, 1), 'FT': (0, 3), 'FF': (0, 1)}


def pre_cells():
    cells = []
    for dt in ('u8', 'u16', 'f64'):
        for ty in (8, 4, 2):
            cells.append(Cell('preprocess', 'ty%d-%s' % (ty, dt), dict(ty=ty, hx=False)))
    for dt in SHORT.values():     # the pin: largest box that fits, the next one is refused
        cells.append(Cell('preprocess', 'ty1-%s' % dt, dict(ty=1, hx=False, limit=True)))
    for dt in ('u8', 'f64'):      # the Gaussian halo alone (lowpass: no box)
        for ty in (8, 2):
            cells.append(Cell('preprocess', 'gauss-ty%d-%s' % (ty, dt), dict(ty=ty, mode='lowpass')))
    for pair in ('TT', 'TF', 'FT', 'FF'):
        for dt in ('u8', 'i16', 'f32', 'f64'):
            cells.append(Cell('preprocess', 'z%s-%s' % (pair, dt),
                              dict(z_gauss=pair[0] == 'T', z_box=pair[1] == 'T',
                                   gin=8 if pair[0] == 'T' else LONG[dt].itemsize,
                                   ty=8 if dt == 'f64' else 16)))      # float64: a reduced tile behind the z passes
    for axis, dt in (('x', 'u8'), ('y', 'u16'), ('x', 'f64')):
        cells.append(Cell('preprocess', 'hx-%s-%s' % (axis, dt), dict(hx=axis, reduced=True)))
    for w in (63, 64, 65, 129):
        cells.append(Cell('preprocess', 'w%d-i32' % w, dict(ty=8, nx=w)))
    for dt in ('f32', 'f64'):
        cells.append(Cell('preprocess', 'scale-mid-%s' % dt, dict(bpf='mid')))
        cells.append(Cell('preprocess', 'scale-cap-%s' % dt, dict(bpf='cap')))
    return cells


def _rows_past_multiple(at_least, ty):
    """the smallest k * ty + 1 that is >= at_least"""
    return -(-(at_least - 1) // ty) * ty + 1


def _pre_frames(rng, shape, dt, n=2):
    from test_gpu_preprocess import _random_frame
    return np.stack([_random_frame(rng, shape, dt) for _ in range(n)])


def _search_box(ty, dt, shape_of, noise=1):
    """largest odd isotropic box whose plan has this ty on a frame shape_of(box, ty) (the frame
    holds the whole half-width, so that no halo is cut)"""
    best = None
    for box in range(3, 1001, 2):
        p = pre_plan(shape_of(box, ty), dt, 'preprocess', noise, box)
        if p.ok and p.ty == ty:
            best = box
        if not p.ok:
            break
    assert best is not None
    return best


def build_pre(cell):
    rng = np.random.RandomState(seed_of(cell))
    kind, _, rest = cell.name.partition('-')
    if kind.startswith('ty'):
        ty, dt = int(kind[2:]), LONG[rest]

        def shape_of(box, ty):      # (a float frame has well over 1000 pixels)
            return (_rows_past_multiple(box // 2 + 3, max(ty, 2)), box // 2 + 3 + 7 + (60 if dt.kind == 'f' else 0))
        box = _search_box(ty, dt, shape_of)
        shape = shape_of(box + 2 if ty == 1 else box, ty)     # ty1: the frame holds the next box too
        return Case(cell, mode='preprocess', frames=_pre_frames(rng, shape, dt), noise=1, smooth=box,
                    next_smooth=box + 2 if ty == 1 else None)
    if kind == 'gauss':
        ty, dt = int(rest.split('-')[0][2:]), LONG[rest.split('-')[1]]
        sigma = None
        for s4 in range(4, 2000):     # sigma in quarters: lw = int(4 sigma + .5) = s4
            shape = (_rows_past_multiple(s4 + 3, ty), s4 + 9)
            p = pre_plan(shape, dt, 'lowpass', s4 / 4.)
            if p.ok and p.ty == ty:
                sigma, keep = s4 / 4., shape
                break
        return Case(cell, mode='lowpass', frames=_pre_frames(rng, keep, dt), noise=sigma, smooth=None, next_smooth=None)
    if kind[0] == 'z':
        dt = LONG[rest]
        nz_, bz = Z_PAIRS[kind[1:]]
        yx = 31 if dt == np.float64 else 7        # float64: ty = 8 behind the z passes
        shape = (7, 33, 70) if dt.kind != 'f' else (7, 49, 80)
        return Case(cell, mode='preprocess', frames=_pre_frames(rng, shape, dt), noise=(nz_, 1, 1), smooth=(bz, yx, yx),
                    next_smooth=None)
    if kind == 'hx':
        axis, dt = rest.split('-')[0], LONG[rest.split('-')[1]]
        narrow, wide_box = (30, 101) if dt == np.float64 else (40, 201)
        for box in range(3, 2001, 2):     # the other axis' box is raised until the tile shrinks
            n = _rows_past_multiple(max(box // 2 + 3, 80), 8)    # (a float frame has well over 1000 pixels)
            shape, smooth = ((n, narrow), (box, wide_box)) if axis == 'x' else ((narrow, n), (wide_box, box))
            p = pre_plan(shape, dt, 'preprocess', 1, smooth)
            if p.ok and p.ty <= 8:
                break
        return Case(cell, mode='preprocess', frames=_pre_frames(rng, shape, dt), noise=1, smooth=smooth, next_smooth=None)
    if kind[0] == 'w':
        nx, dt = int(kind[1:]), LONG[rest]
        for box in range(3, 2001, 2):
            shape, smooth = (_rows_past_multiple(box // 2 + 3, 8), nx), (box, 9)
            p = pre_plan(shape, dt, 'preprocess', 1, smooth)
            if p.ok and p.ty == 8:
                break
        return Case(cell, mode='preprocess', frames=_pre_frames(rng, shape, dt), noise=1, smooth=smooth, next_smooth=None)
    if kind == 'scale':
        which, dt = rest.split('-')[0], LONG[rest.split('-')[1]]
        shape = (101, 203) if which == 'mid' else (725, 727)
        frames = _pre_frames(rng, shape, dt, 3) - np.asarray(0.02, dt)
        # the maximum in the last pixel (the last block's tail), in the first, and wherever it fell
        frames[0].flat[-1] = frames[0].max() * 2
        frames[1].flat[0] = frames[1].max() * 2
        return Case(cell, mode='scale', frames=frames, noise=None, smooth=None, next_smooth=None)
    raise KeyError(cell.name)


def pre_case_plan(case):
    return pre_plan(case.frames.shape[1:], case.frames.dtype, case.mode, case.noise, case.smooth)


def pre_in_cell(case):
    """the restated plan of the case against what the cell's name says"""
    p, want = pre_case_plan(case), case.cell.want
    shape = case.frames.shape[1:]
    assert p.ok, p
    if 'ty' in want:
        assert p.ty == want['ty'], p
        if p.ty > 1 and case.mode != 'scale':
            assert shape[-2] % p.ty == 1          # a height one past a multiple of ty
    if want.get('hx') is False:
        assert not any(p.hx), p
    if want.get('hx') in ('x', 'y'):
        assert p.hx[2 if want['hx'] == 'x' else 1] > 0, p
    if want.get('reduced'):
        assert p.ty < 16, p
    if want.get('limit'):       # nothing larger fits: the next box does not, on a frame that holds it
        nxt = pre_plan(shape, case.frames.dtype, case.mode, case.noise, case.next_smooth)
        assert not nxt.ok and not any(nxt.hx) and nxt.ty == 1, nxt
    for k in ('z_gauss', 'z_box', 'gin'):
        if k in want:
            assert getattr(p, k) == want[k], (k, p)
    if 'nx' in want:
        assert shape[-1] == want['nx']
    if want.get('mode'):
        assert case.mode == want['mode']
    if want.get('bpf') == 'mid':
        assert 1 < p.bpf < 256, p
    if want.get('bpf') == 'cap':
        assert p.bpf == 256 and int(np.prod(shape)) // (PRE_THREADS * 8) > 256, p
    return p


# =============================================================================================
# locate: tu_locate.hip
# =============================================================================================
LOC_TX, LOC_THREADS, LOC_CHUNK_WORDS, LOC_LDS_MAX = 64, 256, 1024, 64 * 1024   # locate_kernels.h:20-22, tu_locate.hip:17

LocPlan = collections.namedtuple('LocPlan', 'ok box lo reach ring ty lds nwx W bpf cpf suppress ytiles')


def loc_lds_bytes(b, ring, ty, es):
    """tu_locate.hip:142-145"""
    return es * ((ty + b[1] - 1) * (LOC_TX + b[2] - 1) + (ty + b[1] - 1) * LOC_TX + ring * ty * LOC_TX)


def loc_plan(shape, dtype, separation, precise=True):
    ndim, a0 = len(shape), 3 - len(shape)
    sep = _tuple(separation, ndim)
    ext, b, lo, reach, sp3 = [1] * 3, [1] * 3, [0] * 3, [0] * 3, [1.] * 3
    E = 1
    for i in range(ndim):                                              # tu_locate.hip:109-130
        a = a0 + i
        ext[a] = int(shape[i])
        E *= ext[a]
        sp3[a] = float(sep[i])
        bb = max(int(2. * sep[i] / math.sqrt(float(ndim))), 1)          # :122-123
        l_, h_ = min((bb - 1) // 2, ext[a]), min(bb // 2, ext[a])      # :124-126
        b[a], lo[a] = l_ + h_ + 1, l_                                   # :127-128
        reach[a] = int(min(math.floor(sep[i]), ext[a]))                 # :129
    nz, ny, nx = ext
    nwx = (nx + LOC_TX - 1) // LOC_TX                                   # :136
    W = nz * ny * nwx                                                   # :137
    ring = min(b[0], nz)                                                # :138
    es = np.dtype(dtype).itemsize
    ty = 16 if ndim == 2 else 8                                         # :141
    while ty > 1 and loc_lds_bytes(b, ring, ty, es) > LOC_LDS_MAX:      # :146
        ty //= 2
    lds = loc_lds_bytes(b, ring, ty, es)
    bpf = min(64, max(1, (E + LOC_THREADS * 16 - 1) // (LOC_THREADS * 16)))     # :22
    cpf = (W + LOC_CHUNK_WORDS - 1) // LOC_CHUNK_WORDS                  # :23
    suppress = bool(precise) and all(s > 0 for s in sp3)                # :24
    return LocPlan(lds <= LOC_LDS_MAX, tuple(b), tuple(lo), tuple(reach), ring, ty, lds, nwx, W, bpf, cpf,
                   suppress, (ny + ty - 1) // ty)


def sep_for_box(box, ndim):
    """a separation whose box int(2 s / sqrt(ndim)) is `box`"""
    s = (box + 0.5) * math.sqrt(ndim) / 2.
    assert int(2. * s / math.sqrt(float(ndim))) == box
    return s


def loc_cells():
    cells = []
    for dt in SHORT.values():       # several tiles wide and high, histogram over several blocks, two chunks
        cells.append(Cell('locate', 'tiles-%s' % dt, dict(nwx=4, bpf='mid', cpf=2)))
    cells.append(Cell('locate', 'big-u8', dict(bpf='cap', cpf='several', precise=True)))
    cells.append(Cell('locate', 'big-f32', dict(bpf='cap', cpf='several', precise=False)))
    cells.append(Cell('locate', 'narrow64-i16', dict(nwx=1, cpf=1, nx=64)))
    cells.append(Cell('locate', 'narrow65-i32', dict(nwx=2, cpf=1, nx=65)))
    for dt in ('u16', 'f32', 'f64'):
        for ty in (8, 4, 2):
            cells.append(Cell('locate', 'ty%d-%s' % (ty, dt), dict(ty=ty, ndim=2)))
    for dt in SHORT.values():       # the pin: largest box that fits, the next one is refused
        cells.append(Cell('locate', 'ty1-%s' % dt, dict(ty=1, ndim=2, limit=True)))
    for ty, dt in ((4, 'f64'), (2, 'i32'), (1, 'f32')):
        cells.append(Cell('locate', 'ty3d-%d-%s' % (ty, dt), dict(ty=ty, ndim=3)))
    cells.append(Cell('locate', 'ring-nz-u8', dict(ring_short=True)))
    cells.append(Cell('locate', 'clip-y-u16', dict(clip=1)))
    cells.append(Cell('locate', 'clip-x-u8', dict(clip=2)))
    cells.append(Cell('locate', 'seam-word-u8', dict(seam='word')))
    cells.append(Cell('locate', 'seam-word-f32', dict(seam='word')))
    cells.append(Cell('locate', 'seam-batch-u16', dict(seam='batch')))
    return cells


def _loc_frames(rng, shape, dt, n, blobs=None):
    from test_gpu_locate import _frame
    if blobs is None:
        blobs = max(4, int(np.prod(shape)) // 400)
    return np.stack([_frame(rng, shape, dt, rng.randint(blobs // 2, blobs + 1)) for _ in range(n)])


def _search_loc_box(ty, dt, ndim, shape_of):
    best = None
    for box in range(3, 400):
        p = loc_plan(shape_of(box), dt, sep_for_box(box, ndim))
        if p.ok and p.ty == ty:
            best = box
        if not p.ok:
            break
    assert best is not None
    return best


def _plant(frame, y, x, value):
    frame[y, x] = value


def _seam_word_frames(rng, dt):
    """separation 5 (box 7, half-width 3) on 40 x 200: pairs of peaks across x = 63 | 64 and
    127 | 128, equal and unequal, adjacent (inside the box) and 4 apart (outside the box, inside
    the separation: only the suppression sees both), and 5 apart (exactly the separation: kept)"""
    from test_gpu_locate import _frame
    frames = []
    dt = np.dtype(dt)
    for t in range(4):
        f = _frame(rng, (40, 200), dt, 3)
        top = float(f.max())
        hi, lo = top + 40, top + 25
        if dt.kind in 'ui':
            hi, lo = min(hi, np.iinfo(dt).max), min(lo, np.iinfo(dt).max - 1)
        rows = iter(range(4, 40, 8))
        for seam in (63, 127):
            for (xa, va), (xb, vb) in ((((seam, hi), (seam + 1, hi)), ((seam, hi), (seam + 1, lo)), ((seam - 2, hi), (seam + 2, hi)),
                                        ((seam - 2, lo), (seam + 2, hi)), ((seam - 2, hi), (seam + 2, lo)), ((seam - 2, hi), (seam + 3, hi)))
                                       [t::4] + (((seam - 2, hi), (seam + 2, hi)),)):
                y = next(rows, None)
                if y is None:
                    break
                f[y, xa], f[y, xb] = va, vb
        frames.append(f)
    return np.stack(frames)


def _seam_batch_frames(rng, dt):
    """peaks in the last rows of frame t and the first rows of frame t + 1, same columns, equal
    and unequal: neighbours in the flat word range, strangers in the rule"""
    from test_gpu_locate import _frame
    frames = np.stack([_frame(rng, (33, 130), dt, 3) for _ in range(4)])
    top = int(frames.max())
    for t in range(3):
        for k, x in enumerate((5, 40, 63, 64, 100, 128)):
            a, b = top + 50 + 3 * k, top + 50 + (3 * k if k % 2 else 3 * k + 7)
            frames[t, 32 - (k % 3), x] = a
            frames[t + 1, k % 2, x + (k % 3) - 1] = b
    return frames


def build_loc(cell):
    rng = np.random.RandomState(seed_of(cell))
    name = cell.name
    kind = name.split('-')[0]
    dt = LONG[name.split('-')[-1]]
    pct = (30, 64, 90)[seed_of(cell) % 3]
    kw = dict(percentile=pct, margin=None, precise=(True, False), next_separation=None)
    if kind == 'tiles':
        return Case(cell, frames=_loc_frames(rng, (300, 200), dt, 2), separation=(6, 7), **kw)
    if kind == 'big':
        kw['precise'] = (cell.want['precise'],)
        return Case(cell, frames=_loc_frames(rng, (600, 610), dt, 2, 600), separation=7, **kw)
    if kind in ('narrow64', 'narrow65'):
        return Case(cell, frames=_loc_frames(rng, (100, int(kind[6:])), dt, 3), separation=5, **kw)
    if kind.startswith('ty') and kind != 'ty3d':
        ty = int(kind[2:])

        def shape_of(box):          # two boxes high and wide: several maxima survive
            return (_rows_past_multiple(2 * box + 4, max(ty, 2)), 2 * box + 64)
        box = _search_loc_box(ty, dt, 2, shape_of)
        shape = shape_of(box + 1 if ty == 1 else box)
        kw['margin'] = 2
        if ty == 1:
            kw['next_separation'] = sep_for_box(box + 1, 2)
        return Case(cell, frames=_loc_frames(rng, shape, dt, 2, 120), separation=sep_for_box(box, 2), **kw)
    if kind == 'ty3d':
        ty = int(name.split('-')[1])

        def shape_of(box):
            return (6, _rows_past_multiple(2 * box + 4, max(ty, 2)), 2 * box + 20)
        # the z box stays small (separation 3 -> box 3): y and x drive the tile
        best = None
        for box in range(3, 400):
            s = sep_for_box(box, 3)
            p = loc_plan(shape_of(box), dt, (3, s, s))
            if p.ok and p.ty == ty:
                best = box
            if not p.ok:
                break
        s = sep_for_box(best, 3)
        kw['margin'] = 1
        return Case(cell, frames=_loc_frames(rng, shape_of(best), dt, 2, 120), separation=(3, s, s), **kw)
    if kind == 'ring':
        return Case(cell, frames=_loc_frames(rng, (3, 40, 70), dt, 4, 12), separation=(7, 5, 5), **dict(kw, margin=(0, 2, 2)))
    if kind == 'clip':
        if name.split('-')[1] == 'y':
            return Case(cell, frames=_loc_frames(rng, (20, 200), dt, 3, 20), separation=(30, 6), **dict(kw, margin=(0, 3)))
        return Case(cell, frames=_loc_frames(rng, (150, 24), dt, 3, 20), separation=(6, 40), **dict(kw, margin=(3, 0)))
    if kind == 'seam':
        if name.split('-')[1] == 'word':
            return Case(cell, frames=_seam_word_frames(rng, dt), separation=5, **dict(kw, margin=0, percentile=64))
        return Case(cell, frames=_seam_batch_frames(rng, dt), separation=5, **dict(kw, margin=0, percentile=64))
    raise KeyError(name)


def loc_case_plan(case, precise=True):
    return loc_plan(case.frames.shape[1:], case.frames.dtype, case.separation, precise)


def loc_in_cell(case):
    p, want = loc_case_plan(case), case.cell.want
    shape = case.frames.shape[1:]
    assert p.ok, p
    for k in ('nwx', 'ty'):
        if k in want:
            assert getattr(p, k) == want[k], (k, p)
    if 'ndim' in want:
        assert len(shape) == want['ndim']
    if want.get('ty', 0) > 1:
        assert shape[-2] % p.ty == 1
    if 'ty' in want:      # the whole box is inside the frame: nothing is clipped
        assert all(b_ // 2 <= n for b_, n in zip(p.box[3 - len(shape):], shape))
    if want.get('bpf') == 'mid':
        assert 1 < p.bpf < 64, p
    if want.get('bpf') == 'cap':
        assert p.bpf == 64 and int(np.prod(shape)) > 64 * LOC_THREADS * 16, p
    if want.get('cpf') == 'several':
        assert p.cpf > 2, p
    elif 'cpf' in want:
        assert p.cpf == want['cpf'], p
    if 'nx' in want:
        assert shape[-1] == want['nx']
    if want.get('limit'):
        nxt = loc_plan(shape, case.frames.dtype, case.next_separation)
        assert not nxt.ok and nxt.ty == 1 and nxt.box[1] == p.box[1] + 1 and nxt.box[2] == p.box[2] + 1, nxt
    if want.get('ring_short'):
        assert p.ring == shape[0] < int(2. * _tuple(case.separation, 3)[0] / math.sqrt(3.)), p
    if 'clip' in want:
        a = want['clip']
        full = int(2. * _tuple(case.separation, 2)[a - 1] / math.sqrt(2.))
        assert p.box[a] < full and p.reach[a] == shape[a - 1] and p.box[3 - a] < shape[2 - a], p
    if 'seam' in want:
        assert p.nwx >= 2 and p.suppress
    return p


# =============================================================================================
# characterize: tu_characterize.hip
# =============================================================================================
CHR_THREADS, CHR_ROW_WINDOW = 256, 17 * 17       # characterize_kernels.h:13, tu_characterize.hip:19

ChrPlan = collections.namedtuple('ChrPlan', 'vol lanes per_block grid tail')


def chr_plan(ndim, radius, n_features):
    vol = 1
    for r in radius:                                                        # tu_characterize.hip:57
        vol *= 2 * int(r) + 1
    lanes = 16 if ndim == 2 and vol <= CHR_ROW_WINDOW else 64               # :23
    per_block = CHR_THREADS // lanes
    grid = (n_features + per_block - 1) // per_block                       # :24, :27
    return ChrPlan(vol, lanes, per_block, grid, n_features % per_block)


CHR_COUNTS = (1, 15, 16, 17, 63, 64, 65, 202000)
CHR_RADII = {16: (8, 8), 64: (8, 9)}       # 289 window pixels: the last 16-lane window; 323: the first 64-lane


def chr_cells():
    cells = []
    for lanes in (16, 64):
        for dt in SHORT.values():
            cells.append(Cell('characterize', 'r%d_%d-%s' % (CHR_RADII[lanes] + (dt,)), dict(lanes=lanes)))
        for n in CHR_COUNTS:
            cells.append(Cell('characterize', 'n%d-g%d' % (n, lanes), dict(lanes=lanes, n=n)))
        cells.append(Cell('characterize', 'empty-g%d' % lanes, dict(lanes=lanes, empty=True)))
    return cells


def _chr_frames(rng, shape, dt, n):
    from test_gpu_characterize import _frame
    return np.stack([_frame(rng, shape, dt) for _ in range(n)])


def _chr_positions(rng, shape, radius, n):
    pos = np.stack([rng.uniform(-r, m - 1 + r, n) for m, r in zip(shape, radius)], 1)
    pos[::4] = np.round(pos[::4])
    pos[1::4] = np.floor(pos[1::4]) + 0.5
    return pos


def build_chr(cell):
    """frames [T, y, x], pos [N, 2], frame_offset [T + 1], radius, isotropic; ``repeat``: the table
    is `repeat` copies of its first N / repeat rows per frame (the yardstick is computed once)"""
    rng = np.random.RandomState(seed_of(cell))
    lanes = cell.want['lanes']
    radius = CHR_RADII[lanes]
    shape = (40, 44)
    isotropic = bool(seed_of(cell) & 1)
    if cell.name.startswith('r'):
        dt = LONG[cell.name.split('-')[1]]
        frames = _chr_frames(rng, shape, dt, 3)
        counts = [23, 31, 26]
        pos = _chr_positions(rng, shape, radius, sum(counts))
        return Case(cell, frames=frames, pos=pos, offset=np.r_[0, np.cumsum(counts)].astype(np.int64), radius=radius,
                    isotropic=isotropic, repeat=1)
    frames = _chr_frames(rng, shape, np.uint16, 4 if 'n' == cell.name[0] else 9)
    if cell.want.get('empty'):
        counts = [0, 0, 5, 0, 0, 7, 3, 0, 0]
        repeat = 1
    else:
        n = cell.want['n']
        if n >= 1000:       # 505 distinct rows per frame, 100 times each
            repeat, counts = 100, [n // 4] * 4
            assert n % 400 == 0
        else:
            repeat = 1
            counts = [n // 4, n - n // 4 - n // 2, 0, n // 2]      # uneven, one frame empty
    distinct = [c // repeat for c in counts]
    parts = [_chr_positions(rng, shape, radius, d) for d in distinct]
    pos = np.concatenate([np.tile(p, (repeat, 1)) for p in parts]) if sum(counts) else np.zeros((0, 2))
    return Case(cell, frames=frames, pos=pos, offset=np.r_[0, np.cumsum(counts)].astype(np.int64), radius=radius,
                isotropic=isotropic, repeat=repeat)


def chr_in_cell(case):
    p, want = chr_plan(2, case.radius, len(case.pos)), case.cell.want
    assert p.lanes == want['lanes'], p
    assert (p.vol <= CHR_ROW_WINDOW) == (want['lanes'] == 16)
    assert case.offset[-1] == len(case.pos) and len(case.offset) == len(case.frames) + 1
    if 'n' in want:
        assert len(case.pos) == want['n']
    if want.get('empty'):
        c = np.diff(case.offset)
        assert c[0] == 0 and c[-1] == 0 and np.any(c[1:-1] == 0) and c.sum() > 0
    return p


# =============================================================================================
# link: tu_link.hip, link_kernels.h
# =============================================================================================
LNK_THREADS, LNK_WAVES, LNK_MAX_SRC, LNK_MAX_DST = 256, 4, 30, 64      # link_kernels.h:43-47

LinkPlan = collections.namedtuple('LinkPlan', 'per_level_launches cand_blocks stride_rounds')


def link_plan(counts, memory):
    """tu_link.hip:44-59: memory 0 queues one candidate and one solve launch for the whole video,
    memory > 0 one pair per level with min(rows, 64) candidate blocks that stride"""
    n = int(sum(counts))
    rows = (n + LNK_THREADS - 1) // LNK_THREADS                          # :44
    if memory == 0 or len(counts) < 2:
        return LinkPlan(False, rows, 1)
    per_level = min(rows, 64)                                           # :54
    biggest = max(counts[1:])
    return LinkPlan(True, per_level, max(1, -(-biggest // (per_level * LNK_THREADS))))


def second_column(ns, nd):
    """link_kernels.h:300: lane l owns columns l + 1 and l + 65 of 1 .. ns + nd"""
    return ns + nd >= 65


def second_column_taken(nd, unlinked):
    """Columns nd + 1 .. ns + nd are the "no link" columns, all of cost 0, and the reduction takes
    the lowest index of equal ones (link_kernels.h:326-331): an unlinked source is assigned the
    lowest free one.  A column l + 65 is therefore assigned -- and the us1 / v1 half of the loop
    runs with effect -- only when more than 64 - nd sources of the sub-network stay unlinked."""
    return unlinked > LNK_MAX_DST - nd


SHAPES = [(30, 64), (30, 40), (12, 60), (29, 8), (20, 5),            # the issue's, and rectangular both ways
          (20, 44), (20, 45), (20, 46), (5, 59), (5, 60), (5, 61), (30, 34), (30, 35), (2, 62), (2, 63)]


STARS = [(3, 64), (3, 60), (3, 50), (2, 60), (1, 62)]      # (hubs, destinations): 9 hubs + 1 sources


COMBS = [12, 20, 24]       # destinations along the 30 sources of a 30 x 64 sub-network; the rest crowd at source 0


def link_cells():
    cells = []
    for k in COMBS:             # competition AND unlinked sources: augmenting paths through the columns beyond 64
        for memory in (0, 2):
            cells.append(Cell('link', 'comb30x64-k%d-m%d' % (k, memory),
                              dict(ns=30, nd=64, memory=memory, status=0, second=True, comb=k)))
    for hubs, nd in STARS:      # most sources stay unlinked: the "no link" columns beyond 64 are assigned
        for memory in (0, 2):
            cells.append(Cell('link', 'star%dx%d-m%d' % (hubs, nd, memory),
                              dict(ns=9 * hubs + 1, nd=nd, memory=memory, status=0, second=True, hubs=hubs)))
    for ns, nd in SHAPES:
        for memory in (0, 2):
            cells.append(Cell('link', '%dx%d-m%d' % (ns, nd, memory),
                              dict(ns=ns, nd=nd, memory=memory, status=0, second=second_column(ns, nd))))
    for memory in (0, 2):
        cells.append(Cell('link', '31x40-m%d' % memory, dict(ns=31, nd=40, memory=memory, status=1)))
        cells.append(Cell('link', '5x65-m%d' % memory, dict(ns=5, nd=65, memory=memory, status=2)))
    cells.append(Cell('link', 'many-subnets-m0', dict(memory=0, status=0, subnets=24)))
    cells.append(Cell('link', 'many-subnets-m2', dict(memory=2, status=0, subnets=24)))
    cells.append(Cell('link', 'big-level-m1', dict(memory=1, status=0, stride_rounds=2)))
    return cells


SEARCH_RANGE = 5.


def chain(rng, ns, nd, origin=(0., 0.), sr=SEARCH_RANGE):
    """one sub-network of ns sources and nd destinations: both along a line, the sources at most
    half a search range apart, the destinations at most 1.2 search ranges apart between them, all
    jittered (continuous positions: no ties).  Returns (sources [ns, 2], destinations [nd, 2])."""
    length = sr * min(0.5 * max(ns - 1, 1), 1.2 * max(nd - 1, 1) if nd > 1 else 0.8)
    def line(n):
        x = np.linspace(0., length, n) if n > 1 else np.array([length / 2.])
        step = length / max(n - 1, 1)
        x = x + rng.uniform(-0.2, 0.2, n) * min(step, 0.25 * sr)
        y = rng.uniform(-0.2, 0.2, n) * sr
        return np.stack([y + origin[0], x + origin[1]], 1)
    return line(ns), line(nd)


def star(rng, hubs, nd, origin=(0., 0.), sr=SEARCH_RANGE):
    """one sub-network of 9 hubs + 1 sources of which at most hubs + 1 can link: the sources on a
    line 0.2 search ranges apart; `hubs` destinations, each in the middle of ten sources (its ten
    candidates, the last shared with the next hub, so the graph is connected) and able to take one
    of them; nd - hubs more destinations crowded where only the first source is in range.  All
    jittered (no ties).  Returns (sources, destinations)."""
    ns = 9 * hubs + 1
    sx = 0.2 * np.arange(ns) + rng.uniform(-0.01, 0.01, ns)
    sy = rng.uniform(-0.03, 0.03, ns)
    hx = 0.2 * (9 * np.arange(hubs) + 4.5) + rng.uniform(-0.01, 0.01, hubs)
    hy = rng.uniform(-0.03, 0.03, hubs)
    cx = rng.uniform(-0.93, -0.85, nd - hubs)
    cy = rng.uniform(-0.25, 0.25, nd - hubs)
    src = np.stack([sy * sr + origin[0], sx * sr + origin[1]], 1)
    dst = np.stack([np.r_[hy, cy] * sr + origin[0], np.r_[hx, cx] * sr + origin[1]], 1)
    return src, dst


def comb(rng, ns, k, nd, origin=(0., 0.), sr=SEARCH_RANGE):
    """as :func:`star`, but k destinations spread along the sources, each within range of up to
    ten of them and of its neighbours' sources: k + 1 links at most, chosen in competition (the
    augmenting paths re-route earlier links), ns - k - 1 sources unlinked.  The first destination
    returned is one from the middle of the line."""
    sx = 0.2 * np.arange(ns) + rng.uniform(-0.01, 0.01, ns)
    sy = rng.uniform(-0.03, 0.03, ns)
    hx = np.linspace(0.5, 0.2 * (ns - 1) - 0.3, k) + rng.uniform(-0.05, 0.05, k)
    hy = rng.uniform(-0.3, 0.3, k)
    hx[[0, k // 2]], hy[[0, k // 2]] = hx[[k // 2, 0]], hy[[k // 2, 0]]
    cx = rng.uniform(-0.93, -0.85, nd - k)
    cy = rng.uniform(-0.25, 0.25, nd - k)
    src = np.stack([sy * sr + origin[0], sx * sr + origin[1]], 1)
    dst = np.stack([np.r_[hy, cy] * sr + origin[0], np.r_[hx, cx] * sr + origin[1]], 1)
    return src, dst


def _far(rng, n, where=-500.):
    """a few features far from every chain, 10 search ranges apart: they link one to one"""
    return np.stack([where + rng.uniform(-1, 1, n), 50. * np.arange(n) + rng.uniform(-1, 1, n)], 1)


def _with_memory(rng, src, dst, memory):
    """memory 0: [src, dst].  memory 2: [src, far, dst, far']: the sources are lost for one level
    and come back as remembered rows of an earlier level."""
    if memory == 0:
        return [src, dst]
    far = _far(rng, 3)
    return [np.concatenate([src, _far(rng, 2, -900.)]), far, np.concatenate([dst, far[:2] + rng.uniform(-1, 1, (2, 2))]),
            far + rng.uniform(-1, 1, (3, 2))]


MANY = [(3, 3), (2, 5), (20, 50), (4, 2), (7, 9), (1, 3), (12, 60), (3, 1), (2, 2), (30, 36), (5, 5), (9, 4)]


def build_link(cell):
    rng = np.random.RandomState(seed_of(cell))
    want = cell.want
    memory = want['memory']
    if 'ns' in want:
        if 'hubs' in want:
            src, dst = star(rng, want['hubs'], want['nd'], (100., 100.))
        elif 'comb' in want:
            src, dst = comb(rng, want['ns'], want['comb'], want['nd'], (100., 100.))
        else:
            src, dst = chain(rng, want['ns'], want['nd'], (100., 100.))
        # a second, small sub-network in the same level: the wavefronts do not all idle
        s2, d2 = chain(rng, 3, 4, (300., 100.))
        levels = _with_memory(rng, np.concatenate([src, s2]), np.concatenate([dst, d2]), memory)
        levels = [l[rng.permutation(len(l))] for l in levels]
        if 'comb' in want:
            # the sub-network's destination with the highest row owns column 64, the column next to
            # the second ones: it is a destination in competition, not one of the crowd
            lv = levels[2 if memory else 1]
            at = int(np.flatnonzero((lv == dst[0]).all(1))[0])
            lv[[at, -1]] = lv[[-1, at]]
        return Case(cell, levels=levels, memory=memory, sr=SEARCH_RANGE, pair=0)
    if 'subnets' in want:
        srcs, dsts = [], []
        for k in range(want['subnets']):
            s, d = chain(rng, *MANY[k % len(MANY)], origin=(80. * k, 100.))
            srcs.append(s)
            dsts.append(d)
        levels = _with_memory(rng, np.concatenate(srcs), np.concatenate(dsts), memory)
        return Case(cell, levels=[l[rng.permutation(len(l))] for l in levels], memory=memory, sr=SEARCH_RANGE,
                    pair=0)
    if cell.name.startswith('big-level'):
        from test_gpu_link import walkers
        levels = walkers(seed_of(cell) % 1000, 17000, 3, 2, 6000., 1.0, 0.02, 3.0)
        return Case(cell, levels=levels, memory=memory, sr=SEARCH_RANGE, pair=0)
    raise KeyError(cell.name)


def subnets(src, dst, sr):
    """[(ns, nd)] of the sub-networks of one level pair on the host: the connected components of
    the candidate graph link.link_levels builds (up to 10 nearest sources within the range)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    if not len(src) or not len(dst):
        return []
    d, i = cKDTree(src / sr).query(dst / sr, min(10, len(src)), distance_upper_bound=1 + 1e-7)
    d, i = d.reshape(len(dst), -1), i.reshape(len(dst), -1)
    ok = np.isfinite(d)
    s, t = i[ok], np.nonzero(ok)[0]
    if not len(s):
        return []
    g = coo_matrix((np.ones(len(s)), (s, t + len(src))), shape=(len(src) + len(dst),) * 2)
    _, comp = connected_components(g, directed=False)
    n = comp.max() + 1
    per_s = np.bincount(comp[np.unique(s)], minlength=n)
    per_d = np.bincount(comp[np.unique(t) + len(src)], minlength=n)
    return [(int(a), int(b)) for a, b in zip(per_s, per_d) if a and b]


def link_case_subnets(case):
    """the sub-networks of the case's level pair (memory 2: the remembered sources of the level
    before the gap against the level after it)"""
    a = case.pair
    src, dst = case.levels[a], case.levels[a + (2 if case.memory and len(case.levels) == 4 else 1)]
    return subnets(src, dst, case.sr)


def link_in_cell(case):
    want = case.cell.want
    nets = link_case_subnets(case)
    plan = link_plan([len(l) for l in case.levels], case.memory)
    assert plan.per_level_launches == (case.memory > 0)
    if 'ns' in want:
        big = max(nets, key=lambda sd: sd[0] + sd[1])
        assert big == (want['ns'], want['nd']), (big, nets)
        if want['status'] == 0:
            assert second_column(*big) == want['second']
        if 'hubs' in want:      # at most one link per hub and one for the crowd's only source
            assert second_column_taken(want['nd'], want['ns'] - want['hubs'] - 1)
        if 'comb' in want:
            assert second_column_taken(want['nd'], want['ns'] - want['comb'] - 1)
    if 'subnets' in want:
        hard = [sd for sd in nets if sd != (1, 1)]
        assert len(hard) >= 20 and len(hard) == want['subnets'], nets
        assert any(second_column(*sd) for sd in hard) and len(hard) > 4 * LNK_WAVES
    if 'stride_rounds' in want:
        assert plan.cand_blocks == 64 and plan.stride_rounds >= want['stride_rounds'], plan
        assert max(len(l) for l in case.levels[1:]) > 64 * LNK_THREADS
    return nets, plan


# =============================================================================================
STAGES = collections.OrderedDict([
    ('preprocess', (pre_cells, build_pre, pre_in_cell)),
    ('locate', (loc_cells, build_loc, loc_in_cell)),
    ('characterize', (chr_cells, build_chr, chr_in_cell)),
    ('link', (link_cells, build_link, link_in_cell)),
])


def cells(stage=None):
    """every cell, or those of one stage, as tests/_dispatch.launchable_cells() lists the refine ones"""
    out = []
    for name, (list_cells, _, _) in STAGES.items():
        if stage in (None, name):
            out.extend(list_cells())
    return out


def build_case(cell):
    """concrete inputs of a cell, seeded from the cell's name"""
    return STAGES[cell.stage][1](cell)


def in_cell(case):
    """asserts that the restated plan of the case lands in its cell; returns the plan"""
    return STAGES[case.cell.stage][2](case)
