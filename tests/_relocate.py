"""The yardstick of the relocation tests: the fixtures of
tests/golden/relocate/relocate_cases.npz, the rule of reference
``FindLinker.get_relocate_candidates`` (find_link.py:811-867) restated from NumPy and SciPy -- used
where the reference does not exist -- and the launch decision of ``ctr_relocate_device`` restated
from tu_relocate.hip / relocate_kernels.h.

Every comparison of the rule is written out in float64, in axis order, one rounding per operation
(NumPy does not contract): the pieces are functions of their own so that the tie tests can put
them next to cKDTree.  The characterisation is tests/_characterize.py's (with its two restated
trackpy weight tables: parity-unpinned)."""
import json
import os

import numpy as np
from scipy import ndimage

import _characterize

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'relocate', 'relocate_cases.npz')

MAX_SOURCES, MAX_MAXIMA, MAX_BACKGROUND, TILE_BYTES = 30, 256, 512, 32768   # include/ctrefine.h
OK, CAPACITY, BAD_FRAME = 0, 1, 2


def as_tuple(v, ndim):
    return tuple(v) if hasattr(v, '__iter__') else (v,) * ndim


def derived(diameter, separation, search_range):
    """find_link.py:754-784"""
    ndim = len(diameter)
    radius = tuple(int(d // 2) for d in diameter)
    slice_radius = tuple(int(s + r + 1) for s, r in zip(search_range, radius))
    bg_radius = tuple(sl + r + 1 for sl, r in zip(slice_radius, radius))
    return dict(radius=radius, box=tuple(int(2 * s / np.sqrt(ndim)) for s in separation),
                slice_radius=slice_radius, bg_radius=bg_radius,
                max_dist=max(a / b for a, b in zip(bg_radius, search_range)))


def _sum_sq(terms):
    """sum(t ** 2) over the axes, in axis order"""
    s = 0.
    for t in terms:
        s = s + t * t
    return s


# ---- the pieces of the rule -----------------------------------------------------------------
def box_of(sources, shape, slice_radius):
    """(origin, end) of the query's box, or None (step 1)"""
    r = np.clip(np.round(np.asarray(sources, dtype=np.float64)), -2. ** 40, 2. ** 40)
    slr, shp = np.asarray(slice_radius), np.asarray(shape)
    with np.errstate(invalid='ignore'):
        inside = np.all((r >= -slr) & (r < shp + slr), axis=1)
    if not inside.any():
        return None
    r = r[inside].astype(np.int64)
    return np.maximum(0, r.min(0) - slr), np.minimum(shp, r.max(0) + slr + 1)


def ellipse_sums(ext, centres, radius):
    """[n, *ext]: sum(((p - centre) / radius) ** 2) for every pixel p of a box and every centre"""
    grid = np.indices(tuple(ext)).astype(np.float64)
    out = np.empty((len(centres),) + tuple(ext))
    for i, c in enumerate(centres):
        out[i] = _sum_sq([(grid[a] - c[a]) / radius[a] for a in range(len(ext))])
    return out


def visible(ext, rel, slice_radius):
    """step 2: edge included"""
    return np.any(ellipse_sums(ext, rel, [float(r) for r in slice_radius]) <= 1, axis=0)


def background(known, sources, search_range, max_dist):
    """step 3, first half: boolean per known feature (frame coordinates, the division first)"""
    known = np.asarray(known, dtype=np.float64).reshape(-1, len(search_range))
    hit = np.zeros(len(known), dtype=bool)
    for s in np.asarray(sources, dtype=np.float64):
        d2 = _sum_sq([known[:, a] / search_range[a] - s[a] / search_range[a] for a in range(len(search_range))])
        hit |= d2 <= max_dist * max_dist
    return hit


def hidden(ext, krel, separation):
    """step 3, second half: strictly inside"""
    if len(krel) == 0:
        return np.zeros(tuple(ext), dtype=bool)
    return np.any(ellipse_sums(ext, krel, [float(s) for s in separation]) < 1, axis=0)


def within_reach(coords, rel, search_range):
    """step 7: boolean per row of coords (box coordinates)"""
    p = np.asarray(coords, dtype=np.float64)
    nd = p.shape[1]
    ok = np.zeros(len(p), dtype=bool)
    equal = all(s == search_range[0] for s in search_range)
    for r in rel:
        if equal:
            ok |= _sum_sq([p[:, a] - r[a] for a in range(nd)]) <= search_range[0] * search_range[0]
        else:
            ok |= _sum_sq([p[:, a] / search_range[a] - r[a] / search_range[a] for a in range(nd)]) <= 1.
    return ok


def close_losers(coords, separation, value):
    """step 8: boolean per row, True = dropped.  All pairs at once; a pair is close at a scaled
    distance <= 1 - 1e-7; the loser is the lower one in (value, sum of pos / separation, row)."""
    p = np.asarray(coords, dtype=np.float64)
    n, nd = p.shape
    q = [p[:, a] / separation[a] for a in range(nd)]
    ssum = 0.
    for a in range(nd):
        ssum = ssum + q[a]
    d2 = _sum_sq([q[a][:, None] - q[a][None, :] for a in range(nd)])
    r = 1 - 1e-7
    close = d2 <= r * r
    np.fill_diagonal(close, False)
    v = np.asarray(value)
    row = np.arange(n)
    beats = (v[None, :] > v[:, None]) | ((v[None, :] == v[:, None]) & (
        (ssum[None, :] > ssum[:, None]) | ((ssum[None, :] == ssum[:, None]) & (row[None, :] > row[:, None]))))
    return np.any(close & beats, axis=1)


def masked_box(frame, sources, known, d, separation, search_range):
    """(m over the box, origin, rel) of steps 1-4, or None without a box"""
    frame = np.asarray(frame)
    sources = np.asarray(sources, dtype=np.float64).reshape(-1, frame.ndim)
    bx = box_of(sources, frame.shape, d['slice_radius'])
    if bx is None:
        return None
    origin, end = bx
    box = frame[tuple(slice(o, e) for o, e in zip(origin, end))]
    rel = sources - origin
    keep = visible(box.shape, rel, d['slice_radius'])
    known = np.asarray(known, dtype=np.float64).reshape(-1, frame.ndim)
    if len(known):
        bg = known[background(known, sources, search_range, d['max_dist'])]
        keep &= ~hidden(box.shape, bg - origin, separation)
    return box * keep, origin, rel


def compose(frame, threshold, sources, known, diameter, separation, search_range, minmass=0,
            isotropic=None, scale_factor=1.):
    """(coords [n, ndim] int64 in frame coordinates, dict of mass, signal, size...) by mass
    descending (equal masses in C order), or (None, None) -- empty arrays when only the minmass
    cut left nothing, as the reference.  Steps 1-10 of the rule; the
    reference's two sum exits are implied for frames without negative pixels."""
    frame = np.asarray(frame)
    ndim = frame.ndim
    diameter, separation, search_range = (as_tuple(v, ndim) for v in (diameter, separation, search_range))
    if isotropic is None:
        isotropic = all(x == diameter[0] for x in diameter)
    d = derived(diameter, separation, search_range)
    if threshold is None or np.isnan(threshold):
        return None, None
    mb = masked_box(frame, sources, known, d, separation, search_range)
    if mb is None:
        return None, None
    m, origin, rel = mb
    thr = np.float32(threshold) if frame.dtype == np.float32 else threshold
    dil = ndimage.grey_dilation(m, [max(b, 1) for b in d['box']], mode='constant')
    coords = np.argwhere((m == dil) & (m > thr))
    if len(coords) == 0:
        return None, None
    coords = coords[within_reach(coords, rel, search_range)]
    if len(coords) == 0:
        return None, None
    coords = coords[~close_losers(coords, separation, m[tuple(coords.T)])]
    extra = _characterize.compose(coords, m, d['radius'], isotropic, scale_factor)
    with np.errstate(invalid='ignore'):
        keep = np.flatnonzero(extra['mass'] >= minmass)
    order = keep[np.argsort(-extra['mass'][keep], kind='stable')]     # none left: empty arrays, as the reference
    return coords[order] + origin, {k: v[order] for k, v in extra.items()}


def n_raw_maxima(frame, threshold, sources, known, diameter, separation, search_range):
    """raw maxima of the box (before reach): what CTR_RELOCATE_MAX_MAXIMA bounds"""
    frame = np.asarray(frame)
    ndim = frame.ndim
    diameter, separation, search_range = (as_tuple(v, ndim) for v in (diameter, separation, search_range))
    d = derived(diameter, separation, search_range)
    mb = masked_box(frame, sources, known, d, separation, search_range)
    if mb is None or np.isnan(threshold):
        return 0
    m = mb[0]
    dil = ndimage.grey_dilation(m, [max(b, 1) for b in d['box']], mode='constant')
    return int(np.sum((m == dil) & (m > threshold)))


# ---- constructed ties ----------------------------------------------------------------------------
def spots(points, shape=(48, 56), dtype=np.uint8):
    f = np.zeros(shape, dtype=dtype)
    for y, x, v in points:
        f[y, x] = v
    return f


TIE_THRESHOLD = 10.


def tie_cases():
    """[(name, frame, sources, known, kwargs)]: one query each, with a pixel, a known feature or a
    maximum exactly ON one of the rule's edges (or just off it, as a control).  Integer geometry:
    3-4-5 and 6-8-10 triangles around the source (24, 28).  slice_radius = 5 + 4 + 1 = 10,
    bg_radius = 15, max_dist = 3."""
    S = np.array([[24., 28.]])
    none = np.empty((0, 2))
    k11 = dict(diameter=9, separation=11, search_range=5)
    k10 = dict(diameter=9, separation=10, search_range=5)
    aniso = dict(diameter=(7, 9), separation=(9, 11), search_range=(4, 6))
    return [
        # a pixel ON the visible ellipse is part of m: it outshines the maximum next to it
        ('visible_edge_axis', spots([(24, 32, 100), (24, 38, 200)]), S, none, k11),
        ('visible_edge_6_8', spots([(27, 31, 100), (30, 36, 200)]), S, none, k11),
        ('visible_outside', spots([(27, 31, 100), (31, 36, 200)]), S, none, k11),
        # a pixel ON the separation ellipse of a known feature is not hidden
        ('background_edge_6_8', spots([(26, 31, 200)]), S, np.array([[20., 23.]]), k10),
        ('background_edge_axis', spots([(26, 31, 200)]), S, np.array([[16., 31.]]), k10),
        ('background_inside', spots([(26, 31, 200)]), S, np.array([[20., 23.5]]), k10),
        # a known feature AT max_dist (9-12-15 from the source) counts: it hides (26, 32)
        ('max_dist_on', spots([(26, 32, 200)]), S, np.array([[33., 40.]]), k11),
        ('max_dist_axis', spots([(29, 28, 200)]), S + [0.5, 0.], np.array([[39.5, 28.]]), k11),
        ('max_dist_beyond', spots([(26, 32, 200)]), S, np.array([[33., 41.]]), k11),
        # a maximum AT the search range is within reach
        ('reach_3_4', spots([(27, 32, 200)]), S, none, k11),
        ('reach_axis', spots([(24, 33, 200)]), S, none, k11),
        ('reach_offset_source', spots([(27, 32, 200)]), S + [0.25, 0.], none, k11),
        ('reach_beyond', spots([(28, 32, 200)]), S, none, k11),
        ('reach_aniso_axis', spots([(24, 34, 200)]), S, none, aniso),
        ('reach_aniso_axis0', spots([(28, 28, 200)]), S, none, aniso),
        ('reach_aniso_beyond', spots([(27, 33, 200)]), S, none, aniso),
        # equal pixels: drop-close keeps the larger sum of pos / separation, then the later in C order
        ('plateau_sum', spots([(24, 27, 200), (24, 30, 200)]), S, none, k11),
        ('plateau_c_order', spots([(24, 29, 200), (25, 28, 200)]), S, none, k11),
        ('plateau_2x2', spots([(24, 28, 200), (24, 29, 200), (25, 28, 200), (25, 29, 200)]), S, none, k11),
        ('plateau_aniso', spots([(23, 29, 200), (25, 27, 200)]), S, none, aniso),
    ]


# ---- the launch decision (tu_relocate.hip: ctr_relocate_launch) --------------------------------
def plan(shape, dtype, diameter, separation, search_range):
    """(pixels of the LDS tile, dynamic LDS bytes): the tile holds a one-source box (clipped to the
    frame) or the thinnest slab of a frame-wide box (dilation box of axis 0 x the other axes),
    whichever is larger, up to TILE_BYTES.  No frame is refused."""
    ndim = len(shape)
    diameter, separation, search_range = (as_tuple(v, ndim) for v in (diameter, separation, search_range))
    d = derived(diameter, separation, search_range)
    es = np.dtype(dtype).itemsize
    cap = TILE_BYTES // es
    one = 1
    for a in range(ndim):
        one *= min(2 * d['slice_radius'][a] + 1, shape[a])
    slab = min(dilation_box0(d, shape), shape[0]) * int(np.prod(shape[1:]))
    tile = min(cap, max(one, slab))
    return tile, (tile * es + 15) & ~15


def dilation_box0(d, shape):
    """the dilation box of axis 0 as the kernel takes it (0 -> 1, its reach clipped to the frame)"""
    b0 = max(d['box'][0], 1)
    return min((b0 - 1) // 2, shape[0]) + min(b0 // 2, shape[0]) + 1


def path(box_shape, tile, box0):
    """what the kernel does with a query's box: ('tile', 1), ('slabs', number of slabs), or
    ('direct', 1) where not one slab with its halo fits the tile: m is read from global memory"""
    vol = int(np.prod(box_shape))
    if vol <= tile:
        return 'tile', 1
    th = tile // int(np.prod(box_shape[1:])) - (box0 - 1)
    if th < 1:
        return 'direct', 1
    return 'slabs', -(-box_shape[0] // th)


# ---- fixtures ------------------------------------------------------------------------------------
def size_array(extra, ndim, isotropic):
    keys = _characterize.size_keys(ndim, isotropic)
    return extra['size'] if isotropic else np.stack([extra[k] for k in keys], 1)


class Case(object):
    """one fixture: a frame, its known features, the arguments and Q queries with the reference's
    answers (``expect[q]`` = None or (coords, mass, signal, size))"""

    def __init__(self, name, frame, known, args, threshold, sources, source_offset, expect):
        self.name, self.frame, self.known, self.args = name, frame, known, args
        self.threshold, self.sources, self.source_offset, self.expect = threshold, sources, source_offset, expect
        self.ndim = frame.ndim
        self.diameter, self.separation, self.search_range = (
            as_tuple(args[k], self.ndim) for k in ('diameter', 'separation', 'search_range'))
        self.minmass, self.scale_factor = args['minmass'], args['scale_factor']
        self.isotropic = all(x == self.diameter[0] for x in self.diameter)

    @property
    def n_queries(self):
        return len(self.source_offset) - 1

    def query(self, q):
        return self.sources[self.source_offset[q]:self.source_offset[q + 1]]

    def kwargs(self):
        return dict(diameter=self.diameter, separation=self.separation, search_range=self.search_range,
                    minmass=self.minmass, scale_factor=self.scale_factor)


def fixtures():
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(json.loads(str(z['names']))):
        args = json.loads(str(z['args_%d' % i]))
        roff, is_none = z['result_offset_%d' % i], z['is_none_%d' % i]
        expect = []
        for q in range(len(is_none)):
            sl = slice(roff[q], roff[q + 1])
            expect.append(None if is_none[q] else tuple(z['%s_%d' % (k, i)][sl] for k in ('coords', 'mass', 'signal', 'size')))
        out.append(Case(name, z['frame_%d' % i], z['known_%d' % i], args, float(z['threshold_%d' % i]),
                        z['sources_%d' % i], z['source_offset_%d' % i], expect))
    return out


def float_rtol(dtype, radius):
    return _characterize.float_rtol(dtype, radius)
