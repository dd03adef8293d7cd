"""Inputs at the exact ties and value edges of the small kernels of
clustertracking_amd/csrc/aux_kernels.h: cluster labelling (``find_clusters_kernel``), the
per-frame maximum (``frame_max_kernel``) and the result rows (``result_rows_kernel``).
Plain NumPy; nothing here needs a GPU or loads the engine.

Cluster labelling.  The rule is the reference's find.py:72-93,
``cKDTree(pos / separation).query_pairs(1)``: a pair when the scaled squared distance, summed in
axis order in float64 with every product rounded, is ``<= 1``.  ``tie_configs(sep)`` holds, each
as a frame of its own, every integer offset whose scaled squared length is exactly 1 in rational
arithmetic (Pythagorean triples and quadruples of the separation, axis-aligned ones included) at
the origin and at seeded integer origins -- the rounding of ``p / s - q / s`` depends on the
origin -- the same with one coordinate moved by one ulp either way, coincident features, and
chains a-b-c whose two links are ties while a-c is far.  ``pair_*`` evaluate one pair by the
rule, by cKDTree and by a sum whose products are fused into the additions (what a compiler that
contracts ``d2 += d * d`` computes); the cases are chosen so that the fused sum is wrong on some
of them in each direction.  ``population_case(ndim)`` holds the frame sizes at the edges of the
kernel's 256-thread stride.

Frame maximum.  ``FM_CHUNK_BYTES`` and the 16-byte vector load set the sizes: a workgroup takes a
chunk of 64 KiB of a frame, scalar loads up to the first 16-byte boundary (the head), vector
loads, scalar loads for the rest (the tail).  ``fm_placement_cases`` plants the single maximum at
every such edge for every frame size, frame count and base-pointer offset; ``fm_value_cases``
holds the ends of each pixel type's range; ``fm_nan_cases`` plants a NaN of either sign.
"""
import collections
import fractions
import itertools

import numpy as np

SEED = 20261017

# ---- cluster labelling ---------------------------------------------------------------------------

TIE_SEPARATIONS = ((5, 5), (10, 10), (13, 13), (25, 25), (26, 26), (29, 29), (39, 39), (58, 58),
                   (13, 26), (5, 10), (3, 3, 3), (7, 7, 7), (9, 9, 9), (3, 7, 9))
N_ORIGINS = 20
FC_THREADS = 256      # aux_kernels.h

Config = collections.namedtuple('Config', 'kind pts')
# kind: 'tie' (two features at scaled distance exactly 1), 'near' (a tie with one coordinate one
#       ulp off), 'dup' (coincident features), 'triple' (a-b and b-c ties, a-c far; rows a, c, b)


def tie_offsets(sep):
    """Every integer offset d with sum((d / sep)**2) == 1 exactly, one of each +-d."""
    F = fractions.Fraction
    sep = [int(s) for s in sep]
    out = []
    for d in itertools.product(*[range(-s, s + 1) for s in sep]):
        nz = [x for x in d if x]
        if not nz or nz[0] < 0:
            continue
        if sum(F(x * x, s * s) for x, s in zip(d, sep)) == 1:
            out.append(d)
    return out


def origins(sep):
    """The origin and N_ORIGINS seeded integer origins in [0, 64)^ndim."""
    rng = np.random.RandomState(SEED + sum((i + 1) * int(s) for i, s in enumerate(sep)))
    return np.concatenate([np.zeros((1, len(sep))), rng.randint(0, 64, (N_ORIGINS, len(sep)))]).astype(np.float64)


def tie_configs(sep):
    """The tie, near-tie, duplicate and triple configurations of one separation (a list of Config)."""
    F = fractions.Fraction
    nd = len(sep)
    offs = [np.array(d, dtype=np.float64) for d in tie_offsets(sep)]
    orgs = origins(sep)
    out = []
    for d in offs:
        for k, o in enumerate(orgs):
            out.append(Config('tie', np.stack([o, o + d])))
            for toward in (np.inf, -np.inf):
                q = o + d
                q[k % nd] = np.nextafter(q[k % nd], toward)
                out.append(Config('near', np.stack([o, q])))
    for i, d1 in enumerate(offs):
        for d2 in (d1, offs[(i + 1) % len(offs)]):
            far = sum(F(int(x)) ** 2 / F(int(s)) ** 2 for x, s in zip(d1 + d2, sep))
            if far <= F(3, 2):
                continue
            for o in orgs[:4]:
                out.append(Config('triple', np.stack([o, o + d1 + d2, o + d1])))
    for o in orgs[:6]:
        out.append(Config('dup', np.stack([o, o])))
        out.append(Config('dup', np.stack([o, o, o])))
        out.append(Config('dup', np.stack([o, o + offs[0], o])))
    return out


def assemble(configs, seed=SEED):
    """(pos [N, ndim], frames [N]) with every configuration in a frame of its own and the rows of
    the table in a seeded random order."""
    pos = np.concatenate([c.pts for c in configs])
    frames = np.repeat(np.arange(len(configs)), [len(c.pts) for c in configs])
    perm = np.random.RandomState(seed).permutation(len(pos))
    return pos[perm], frames[perm]


def _scaled_difference(p, q, sep):
    sep = np.asarray(sep, dtype=np.float64)
    return [float(x) for x in (np.asarray(p, np.float64) / sep - np.asarray(q, np.float64) / sep)]


def pair_by_rule(p, q, sep):
    """((p / s - q / s)**2) summed in axis order in float64, every product rounded: <= 1."""
    s = 0.
    for d in _scaled_difference(p, q, sep):
        s = s + d * d
    return s <= 1.


def pair_by_ckdtree(p, q, sep):
    """The yardstick: the pair is among cKDTree(pos / separation).query_pairs(1)."""
    from scipy.spatial import cKDTree
    return len(cKDTree(np.array([p, q], dtype=np.float64) / np.asarray(sep, np.float64)).query_pairs(1)) == 1


def pair_contracted(p, q, sep):
    """The same sum with the products fused into the additions, rounded once each: in 2D
    fma(d0, d0, rnd(d1 * d1)), in 3D fma(d2, d2, that).  Exact products in rational arithmetic."""
    F = fractions.Fraction
    d = _scaled_difference(p, q, sep)
    acc = float(F(d[0]) * F(d[0]) + F(d[1] * d[1]))
    if len(d) == 3:
        acc = float(F(d[2]) * F(d[2]) + F(acc))
    return acc <= 1.


def population_case(ndim):
    """Frames of 257, 0, 513, 1, 0, 255, 256 uniformly scattered features, a permuted chain of 300
    in which each feature touches only its neighbours, twice the same 40 features in consecutive
    frames, and an empty last frame.  Returns (pos [N, ndim] in frame order, frame_offset
    [T + 1] int32 with the empty frames, separation)."""
    rng = np.random.RandomState(SEED + ndim)
    sep = np.array({2: (2.5, 1.5), 3: (1.5, 2.5, 2.)}[ndim])
    frames = []
    for n in (FC_THREADS + 1, 0, 2 * FC_THREADS + 1, 1, 0, FC_THREADS - 1, FC_THREADS):
        # about one neighbour inside the separation per feature: clusters of many sizes
        unit = np.pi if ndim == 2 else 4. / 3. * np.pi
        side = (max(n, 1) * unit) ** (1. / ndim)
        frames.append(rng.uniform(0., side, (n, ndim)) * sep)
    chain = np.full((300, ndim), 10.)
    chain[:, -1] = np.arange(300) * 0.99 * sep[-1]
    frames.append(rng.permutation(chain))
    twin = rng.uniform(0., 6., (40, ndim)) * sep
    frames += [twin, twin.copy(), np.zeros((0, ndim))]
    offset = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int32)
    return np.concatenate(frames), offset, sep


def canonical_ids(ids):
    """Labels of the same partition whose id is the smallest row of the cluster."""
    ids = np.asarray(ids)
    first = {}
    for row, c in enumerate(ids):
        first.setdefault(c, row)
    return np.array([first[c] for c in ids], dtype=np.int64)


# ---- frame maximum -------------------------------------------------------------------------------

FM_THREADS = 256                   # aux_kernels.h
FM_CHUNK_BYTES = 64 * 1024
FM_DTYPES = (np.uint8, np.uint16, np.int16, np.int32, np.float32, np.float64)
FLOAT_PEAK = 12345.678             # above every background pixel; float32(12345.678) is not this double
NAN_BITS = {np.dtype(np.float32): (np.uint32, (0x7FC00000, 0xFFC00000)),
            np.dtype(np.float64): (np.uint64, (0x7FF8000000000000, 0xFFF8000000000000))}

FMCase = collections.namedtuple('FMCase', 'name buf offset n_frames frame_elems')
# buf: 1-D array whose elements [offset, offset + n_frames * frame_elems) are the frames; what
#      lies before and behind them is larger than every pixel where the pixel type has room


def fm_geometry(dtype):
    """(elements of a 16-byte vector, elements of a chunk)."""
    size = np.dtype(dtype).itemsize
    return 16 // size, FM_CHUNK_BYTES // size


def fm_sizes(dtype):
    v, chunk = fm_geometry(dtype)
    return sorted({1, v - 1, v, v + 1, chunk - 1, chunk, chunk + 1, 2 * chunk + v - 1})


def fm_offsets(dtype):
    v, _ = fm_geometry(dtype)
    return sorted({0, 1, v - 1})


def fm_frames(case):
    """The frames of a case, [n_frames, frame_elems]."""
    return case.buf[case.offset:case.offset + case.n_frames * case.frame_elems].reshape(case.n_frames, -1)


def fm_expected(case):
    with np.errstate(invalid='ignore'):
        return fm_frames(case).max(1).astype(np.float64)


def fm_nan_variants(dtype):
    """(quiet NaN with the sign bit clear, with the sign bit set), built from their bit patterns."""
    bits, patterns = NAN_BITS[np.dtype(dtype)]
    return np.array(patterns, dtype=bits).view(dtype)


def _head(start, n, v):
    """Elements before the first 16-byte boundary of a piece of n elements starting at element
    `start` of a 16-byte-aligned buffer."""
    return min((-start) % v, n)


def fm_placements(start, frame_elems, dtype):
    """{name: element of the frame}, for a frame that starts at element `start` of an aligned
    buffer: the edges of chunk_max's three loops and of the 64 KiB chunks (those the frame has)."""
    v, chunk = fm_geometry(dtype)
    out = collections.OrderedDict(first=0, last=frame_elems - 1)
    h = _head(start, min(frame_elems, chunk), v)
    if h > 0:
        out['head'] = h - 1
    if frame_elems >= chunk:
        out['chunk0_last'] = chunk - 1
    if frame_elems > chunk:
        out['chunk1_first'] = chunk
    begin = (frame_elems - 1) // chunk * chunk      # the last chunk (a chunk is whole vectors)
    n = frame_elems - begin
    h = _head(start + begin, n, v)
    tail = begin + h + (n - h) // v * v
    if tail < frame_elems:
        out['tail'] = tail
    return out


def _background(rng, dtype, n, low=None, high=None):
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        return (rng.standard_normal(n) * 100).astype(dtype)
    info = np.iinfo(dtype)
    low = info.min if low is None else low
    high = info.max if high is None else high
    return rng.randint(low, high + 1, n, dtype=np.int64).astype(dtype)


def _buffer(frames, offset, dtype, poison):
    v, _ = fm_geometry(dtype)
    buf = np.full(offset + frames.size + v, poison, dtype=dtype)
    buf[offset:offset + frames.size] = frames.ravel()
    return buf


def _poison(dtype):
    return np.inf if np.dtype(dtype).kind == 'f' else np.iinfo(dtype).max


def fm_layouts(dtype):
    for fe in fm_sizes(dtype):
        for nf in (1, 3):
            for off in fm_offsets(dtype):
                yield fe, nf, off


def fm_placement_cases(dtype):
    """The single maximum of every frame at one placement, the background strictly below it, for
    every frame size, 1 and 3 frames and every base offset.  The maximum is the type's largest
    value but one, so that the elements around the frames can be larger still."""
    dtype = np.dtype(dtype)
    rng = np.random.RandomState(SEED + dtype.itemsize + ord(dtype.kind))
    if dtype.kind == 'f':
        peak, high = dtype.type(FLOAT_PEAK), None
    else:
        peak, high = np.iinfo(dtype).max - 1, np.iinfo(dtype).max - 2
    for fe, nf, off in fm_layouts(dtype):
        bg = _background(rng, dtype, nf * fe, high=high).reshape(nf, fe)
        spots = [fm_placements(off + f * fe, fe, dtype) for f in range(nf)]
        for name in ('first', 'last', 'head', 'chunk0_last', 'chunk1_first', 'tail'):
            if not any(name in s for s in spots):
                continue
            frames = bg.copy()
            for f, s in enumerate(spots):       # (a frame without this edge: at its last element)
                frames[f, s.get(name, s['last'])] = peak
            yield FMCase('%s-%dx%d+%d' % (name, nf, fe, off), _buffer(frames, off, dtype, _poison(dtype)),
                         off, nf, fe)


def fm_value_cases(dtype):
    """The ends of the pixel type's range, in three frames that start off the 16-byte grid."""
    dtype = np.dtype(dtype)
    rng = np.random.RandomState(SEED + 100 + dtype.itemsize + ord(dtype.kind))
    v, chunk = fm_geometry(dtype)
    nf, off = 3, 1

    def case(name, frames):
        # nothing around the frames that is no pixel value of its own: the range is in use
        return FMCase('%s-%dx%d' % (name, nf, frames.shape[1]), _buffer(frames, off, dtype, frames[0, 0]),
                      off, nf, frames.shape[1])

    for fe in (v + 1, chunk + 1):
        spot = fm_placements(off + fe, fe, dtype)['last']

        def planted(low, high, peak):
            frames = _background(rng, dtype, nf * fe, low, high).reshape(nf, fe)
            frames[1, spot] = peak
            return frames

        if dtype.kind != 'f':
            info = np.iinfo(dtype)
            yield case('type_max', planted(info.min, info.max - 1, info.max))
            yield case('all_type_min', np.full((nf, fe), info.min, dtype=dtype))
            yield case('type_min_but_one', planted(info.min, info.min, info.min + 1))
            if info.min < 0:
                yield case('all_negative', planted(info.min, -2, -1))
            if dtype == np.uint16:      # (travels as int16: the upper half is negative there)
                yield case('max_32768', planted(0, 32767, 32768))
                yield case('all_above_32767', planted(32768, 65534, 65535))
            continue
        info = np.finfo(dtype)
        tiny = info.smallest_subnormal
        negative = -np.abs(_background(rng, dtype, nf * fe)).reshape(nf, fe) - dtype.type(1)
        yield case('all_neg_inf', np.full((nf, fe), -np.inf, dtype=dtype))
        frames = np.full((nf, fe), -np.inf, dtype=dtype)
        frames[1, spot] = -info.max
        yield case('neg_inf_and_lowest_finite', frames)
        frames = _background(rng, dtype, nf * fe).reshape(nf, fe)
        frames[1, spot] = np.inf
        yield case('pos_inf', frames)
        frames = _background(rng, dtype, nf * fe).reshape(nf, fe)
        frames[1, spot] = info.max
        frames[1, 0] = -info.max
        yield case('largest_finite', frames)
        yield case('all_negative', negative.copy())
        frames = negative.copy()
        frames[1, spot] = tiny
        yield case('subnormal_max', frames)
        frames = negative.copy()
        frames[1, spot] = -tiny
        yield case('negative_subnormal_max', frames)
        frames = np.full((nf, fe), -tiny, dtype=dtype) * dtype.type(3)
        frames[1, spot] = -tiny
        yield case('all_negative_subnormals', frames)
        frames = negative.copy()
        frames[1, spot] = dtype.type(0.1)        # float32(0.1) is not the double 0.1
        yield case('one_tenth', frames)


def fm_nan_cases(dtype):
    """One NaN of either sign in the middle frame (of 1 or 3), at every placement; in the lane that
    has already found the frame's largest finite value, FM_THREADS vectors behind it; and a frame
    of nothing but NaN.  The other frames stay finite."""
    dtype = np.dtype(dtype)
    rng = np.random.RandomState(SEED + 200 + dtype.itemsize)
    v, chunk = fm_geometry(dtype)
    for fe, nf, off in fm_layouts(dtype):
        bg = _background(rng, dtype, nf * fe).reshape(nf, fe)
        t = nf // 2
        start = off + t * fe
        for sign, nan in zip(('pos', 'neg'), fm_nan_variants(dtype)):
            def case(name, frames):
                return FMCase('%snan-%s-%dx%d+%d' % (sign, name, nf, fe, off),
                              _buffer(frames, off, dtype, np.inf), off, nf, fe)
            for name, spot in fm_placements(start, fe, dtype).items():
                frames = bg.copy()
                frames[t, spot] = nan
                yield case(name, frames)
            h = _head(start, min(fe, chunk), v)
            peak_at = h + 5 * v + 1
            if peak_at + FM_THREADS * v < min(fe, chunk) - v:      # both in chunk 0's vector loop
                frames = bg.copy()
                frames[t, peak_at] = FLOAT_PEAK
                frames[t, peak_at + FM_THREADS * v] = nan
                yield case('same_lane', frames)
            frames = bg.copy()
            frames[t] = nan
            yield case('all', frames)


# ---- one frame, two NaNs ---------------------------------------------------------------------------

def nan_twin_frames():
    """(frame with a positive NaN, frame with a negative NaN, start table, diameter): a 64 x 64
    float64 frame of a dozen features and one NaN pixel further than the mask radius from each."""
    import pandas as pd
    from clustertracking_amd import artificial
    diameter = 13
    im, truth, p0 = artificial.random_frame((64, 64), 12, 3., 100, 10, 8, margin=13)
    im = im.astype(np.float64)
    yy, xx = np.mgrid[:64, :64]
    away = np.min([(yy - p[0]) ** 2 + (xx - p[1]) ** 2 for p in p0], 0)
    spot = np.unravel_index(np.argmax(away), away.shape)
    assert away[spot] > (diameter // 2 + 3) ** 2
    twins = []
    for nan in fm_nan_variants(np.float64):
        twin = im.copy()
        twin[spot] = nan
        twins.append(twin)
    f0 = pd.DataFrame(p0, columns=['y', 'x'])
    f0['signal'], f0['size'], f0['background'] = 90., 3., 5.
    return twins[0], twins[1], f0, diameter
