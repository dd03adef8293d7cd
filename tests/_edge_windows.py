"""Refine windows and masks at the frame edge: cases and the NumPy yardstick.  No device code.

The window of a cluster (reference masks.py:42-68: round half-even, in-bounds filter, clip to the
frame) and the pixel addressing that follows it exist once per kernel family (small_kernel.h,
block_kernel.h ``window_of``, large_kernel.h, oracle/ctr_oracle.c).  Only a clipped window makes
them differ from their interior behaviour.  The cases here take the clusters of
``_dispatch.build_case`` and crop their frames by whole pixels, so that the patch sits at a face or
a corner of the frame, straddles it or leaves it (``placements`` below); the cut is subtracted
from the start positions, which keep their fractional parts.

The probe is the *pinned evaluation*: every bound pinned to the start (``low = high = params``).
No variable is free, so a minimiser returns the start after one evaluation and its ``cost`` is the
reference objective at the start on the start's window: it checks window, masks, the pixel count
P, ``norm``, the pixel loads and the model, and a single wrong pixel moves it by about 1 / (2 P).
``numpy_cost`` evaluates the same number with ``ref_numpy.subimage`` / ``Layout`` /
``make_objective``; ``mutated_cost`` evaluates it with one deliberate mistake in the window code
(test_edge_windows_cases.py proves that every case sees such a mistake).

Frames of one batch share a shape, so every placement of a cell is a batch of its own (one frame
per cluster, all cropped alike); where a cell's clusters leave different extents the common one is
taken on the side away from the face.
"""
import collections
import functools
from fractions import Fraction

import numpy as np

import _dispatch as D
import clustertracking_amd as cta
import ref_numpy
from clustertracking_amd import _abi

INSIDE, BEYOND = 1.3, -2.4   # px between the outermost centre and the face (negative: outside)
AXES = ('z', 'y', 'x')
OK, OUT_OF_BOUNDS = 0, 1


# ---- cells ------------------------------------------------------------------------------------

def cells():
    """The cells of the edge matrix: per geometry the singles at 8 and 64 lanes, the pairs at 64
    and 16 lanes, every block family at the lowest and highest NT of its table and its constrained
    NT 1, and both large-cluster kernels."""
    out = []
    for c in D.launchable_cells():
        if c.kind == 'block' and c.nt not in (1, D.MAXNT):
            continue
        if c.kind == 'cons' and c.nt != 1:
            continue
        out.append(c)
    return out


CELLS = collections.OrderedDict((D.cell_id(c), c) for c in cells())
# one singles, one block and one large cell also with uint16 and float32 pixels (low corner)
DTYPE_CELLS = ('small-2d-iso-single-8lanes', 'gauss-2d-aniso-nt1', 'large-3d-iso')
GAUSS_FAMILIES = ('small', 'gauss', 'gauss_tp', 'large')   # NumPy is the yardstick; else the oracle


def radius_of(case):
    return np.array([d // 2 for d in case.diameter])


# ---- placements ---------------------------------------------------------------------------------

class Placed(object):
    """One placement of one case: cropped frames, shifted start table, what it is."""

    def __init__(self, cid, case, name, frames, f0, clipped, well_posed, tags=()):
        self.cid, self.case, self.name = cid, case, name
        self.frames, self.f0 = np.ascontiguousarray(frames), f0
        self.clipped = clipped          # some window of it is cut by the frame
        self.well_posed = well_posed    # centres inside, window clipped: a converged fit is defined
        self.tags = set(tags)
        self._prep = None

    @property
    def id(self):
        return '%s/%s' % (self.cid, self.name)

    def prepare(self, compute_error=False):
        prep = cta.prepare_batch(self.f0.copy(), cta.ArrayReader(self.frames), self.case.diameter,
                                 compute_error=compute_error, **self.case.kwargs())
        prep.problem.flags |= self.case.flags
        return prep

    def prep(self):
        if self._prep is None:
            self._prep = self.prepare()
        return self._prep

    def pinned(self):
        """A fresh batch with every bound pinned to the start."""
        hb = self.prep().batch
        return _abi.HostBatch(hb.frames, hb.frame_index, hb.feat_offset, hb.params,
                              hb.params.copy(), hb.params.copy(), want_std=False)

    def free(self, compute_error=True):
        prep = self.prepare(compute_error=compute_error)
        hb = prep.batch
        return prep, _abi.HostBatch(hb.frames, hb.frame_index, hb.feat_offset, hb.params, hb.low,
                                    hb.high, want_std=hb.params_std is not None)


def _positions(case):
    """[cluster] -> (rows of f0, positions [n, nd])"""
    pc = list(AXES[-case.ndim:])
    out = []
    for k in range(len(case.clusters)):
        rows = np.flatnonzero(case.f0['frame'].values == k)
        out.append((rows, case.f0.loc[rows, pc].values))
    return out


def _crop(case, spec):
    """Crop every frame of the case as ``spec`` says per axis and shift the start positions.

    spec[a] is ('full',), ('low', inset), ('high', inset) or ('thin', extent).  -> (frames, f0)"""
    nd, shape = case.ndim, case.frames.shape[1:]
    pc = list(AXES[-nd:])
    pos = _positions(case)
    start = np.zeros((len(pos), nd), int)
    stop = np.tile(np.asarray(shape), (len(pos), 1))
    for a in range(nd):
        s = spec[a]
        for k, (_, p) in enumerate(pos):
            if s[0] == 'low':
                start[k, a] = int(np.floor(p[:, a].min() - s[1]))
            elif s[0] == 'high':
                stop[k, a] = int(np.ceil(p[:, a].max() + s[1])) + 1
            elif s[0] == 'thin':
                start[k, a] = int(np.round(p[:, a].mean())) - s[1] // 2
                stop[k, a] = start[k, a] + s[1]
        ext = int((stop[:, a] - start[:, a]).min())
        if s[0] == 'high':
            start[:, a] = stop[:, a] - ext
        else:
            stop[:, a] = start[:, a] + ext
    assert (start >= 0).all() and (stop <= np.asarray(shape)).all() and (stop > start).all()
    f0 = case.f0.copy()
    frames = []
    for k, (rows, p) in enumerate(pos):
        frames.append(case.frames[k][tuple(slice(i, j) for i, j in zip(start[k], stop[k]))])
        f0.loc[rows, pc] = p - start[k]
    return np.stack(frames), f0


def _set_outermost(case, frames, f0, axis, side, value):
    """Puts, per cluster, the feature outermost along ``axis`` on ``side`` at ``value`` there."""
    col = AXES[-case.ndim:][axis]
    f0 = f0.copy()
    for k in range(len(case.clusters)):
        rows = np.flatnonzero(f0['frame'].values == k)
        x = f0.loc[rows, col].values
        f0.loc[rows[np.argmin(x) if side == 'low' else np.argmax(x)], col] = value
    return frames, f0


def _translate_outermost(case, frames, f0, axis, side, value):
    """Moves, per cluster, the whole cluster along ``axis`` so that its outermost feature on
    ``side`` lies at ``value`` there."""
    col = AXES[-case.ndim:][axis]
    f0 = f0.copy()
    for k in range(len(case.clusters)):
        rows = np.flatnonzero(f0['frame'].values == k)
        x = f0.loc[rows, col].values
        f0.loc[rows, col] = x + (value - (x.min() if side == 'low' else x.max()))
    return frames, f0


FULL = ('full',)


def tie_fractions(radius):
    """-> [(f_y, f_x, differs, n_exact_one)] for the radii of the last two axes (see below)"""
    return list(_tie_fractions(tuple(int(v) for v in radius[-2:])))


@functools.lru_cache(maxsize=None)
def _tie_fractions(radius):
    """Fractional parts (tenths, last two axes) of a centre for which in-frame pixels lie on the
    mask ellipse in exact arithmetic and at least one of them is classified differently by
      - a contracted (fused) evaluation of sum(((idx - rel) / r) ** 2) against the plain one, or
      - rel = c - origin taken from the unclipped origin against the clipped one (origin 0),
    or has a plain sum of exactly 1 (where ``<`` and ``<=`` part)."""
    r = list(radius)
    out = []
    for ty in range(10):
        for tx in range(10):
            differs, exact_one = False, 0
            f = (ty / 10., tx / 10.)
            cin = [40 + f[0], 40 + f[1]]          # interior: origin = round(c) - r
            ccl = [2 + f[0], 2 + f[1]]            # clipped: origin 0
            oin = [int(np.round(cin[a])) - r[a] for a in range(2)]
            for dy in range(-r[0] - 1, r[0] + 2):
                for dx in range(-r[1] - 1, r[1] + 2):
                    # pixel at (round-free) integer offset from the integer part of the centre
                    off = (Fraction(10 * dy - ty, 10), Fraction(10 * dx - tx, 10))
                    if (off[0] * r[1]) ** 2 + (off[1] * r[0]) ** 2 != (r[0] * r[1]) ** 2:
                        continue
                    py, px = 2 + dy, 2 + dx       # the pixel in the clipped frame
                    if py < 0 or px < 0:
                        continue
                    rel_in = [cin[a] - oin[a] for a in range(2)]
                    idx_in = [40 + dy - oin[0], 40 + dx - oin[1]]
                    s_in = _ellipse(idx_in, rel_in, r, False)
                    s_cl = _ellipse([py, px], ccl, r, False)
                    s_fu = _ellipse([py, px], ccl, r, True)
                    if (s_in <= 1) != (s_cl <= 1) or (s_cl <= 1) != (s_fu <= 1):
                        differs = True
                    exact_one += int(s_cl == 1.) + int(s_in == 1.)
            if differs or exact_one:
                out.append((f[0], f[1], differs, exact_one))
    return out


def _ellipse(idx, rel, r, fused):
    s = 0.
    for i, c, rr in zip(idx, rel, r):
        t = (float(i) - c) / float(rr)
        s = float(Fraction(s) + Fraction(t) * Fraction(t)) if fused else s + t * t
    return s


def _snap(case, f0, frac):
    """Every start position at its rounded value plus the fractional parts ``frac`` on the last
    two axes (an integer on axis 0 in 3D)."""
    pc = list(AXES[-case.ndim:])
    f0 = f0.copy()
    p = np.round(f0[pc].values)
    p[:, -2] += frac[0]
    p[:, -1] += frac[1]
    f0[pc] = p
    return f0


def placements(cid):
    """Every placement of one cell's cases -> [Placed]"""
    return list(_placements(cid))


@functools.lru_cache(maxsize=None)
def _placements(cid):
    cell = CELLS[cid]
    out = []
    for ci, case in enumerate(D.build_case(cell)):
        nd = case.ndim
        rad = radius_of(case)
        tag = '' if ci == 0 else '#%d' % ci
        single = all(n == 1 for n in case.n_features)

        def add(name, frames, f0, clipped, well_posed=False, tags=()):
            if case.constraint is not None:
                if 'ties' in tags:
                    return    # (they move every feature by itself: no feasible start to pin)
                f0 = _feasible(case, f0)
            pos = f0[list(AXES[-nd:])].values
            well_posed = well_posed and bool((pos >= 0).all() and (pos <= np.asarray(frames.shape[1:]) - 1).all())
            out.append(Placed(cid, case, name + tag, frames, f0, clipped, well_posed, tags))

        def outermost(frames, f0, side, value):
            # an unconstrained cluster: that feature alone, the rest stay; a constrained one: the
            # rigid shape as a whole, which keeps the pinned start feasible
            if case.constraint is None:
                return _set_outermost(case, frames, f0, nd - 1, side, value)
            return _translate_outermost(case, frames, _feasible(case, f0), nd - 1, side, value)

        add('inside', case.frames, case.f0.copy(), False)
        for a in range(nd):
            for side in ('low', 'high'):
                spec = [FULL] * nd
                spec[a] = (side, INSIDE)
                add('%s-%s' % (side, AXES[-nd:][a]), *_crop(case, spec), clipped=True, well_posed=True)
        for side in ('low', 'high'):
            add('corner-%s' % side, *_crop(case, [(side, INSIDE)] * nd), clipped=True, well_posed=True)
        # thin: axis 0 clipped on both sides below 2 r + 1 (in 3D the z-stack with few slices)
        spec = [FULL] * nd
        spec[0] = ('thin', max(2, int(rad[0])))
        add('thin-%s' % AXES[-nd:][0], *_crop(case, spec), clipped=True, well_posed=True)
        # thin: the last axis with window widths of exactly 1, 2 and 3 (frames that narrow)
        for w in (1, 2, 3):
            spec = [FULL] * nd
            spec[-1] = ('thin', w)
            add('thin-x%d' % w, *_crop(case, spec), clipped=True)
        for side in ('low', 'high'):
            add('beyond-%s' % side, *_crop(case, [(side, BEYOND)] * nd), clipped=True)
        # limit twins on the last axis: the outermost feature's rounded centre exactly at the
        # last kept and the first filtered value of the in-bounds filter
        r = int(rad[-1])
        fr, f0 = _crop(case, [FULL] * (nd - 1) + [('low', -float(r))])
        add('limit-low-kept', *outermost(fr, f0, 'low', -r + 0.3), clipped=True, tags=['limit'])
        add('limit-low-filtered', *outermost(fr, f0, 'low', -r - 0.7), clipped=True, tags=['limit'])
        fr, f0 = _crop(case, [FULL] * (nd - 1) + [('high', -float(r))])
        w = fr.shape[-1]
        add('limit-high-kept', *outermost(fr, f0, 'high', w + r - 1 - 0.3), clipped=True, tags=['limit'])
        add('limit-high-filtered', *outermost(fr, f0, 'high', w + r - 1 + 0.7), clipped=True, tags=['limit'])
        if single:
            # kept by the filter (rounds to -r), but the mask reaches no pixel: status 1 through P = 0
            f0 = case.f0.copy()
            f0[AXES[-1]] = -r - 0.4
            add('kept_no_pixel', case.frames, f0, True)
        f0 = case.f0.copy()
        f0[AXES[-1]] = f0[AXES[-1]] - (f0[AXES[-1]].max() + r + 10)
        add('all_filtered', case.frames, f0, True)
        # ties: pixels on the mask ellipse
        # one rounding-sensitive tie where the radii have one, one tie off the integers whose plain
        # sum is exactly 1 where they have one (r = 5: a pixel at (1.4, 4.8)), and the integer centre
        # (the four axis points are exact ties at every radius; r = 13: 5-12-13)
        found = tie_fractions(rad)
        pick = [t for t in found if t[2]][:1]
        pick += [t for t in found if t[3] and t[:2] != (0., 0.) and t not in pick][:1]
        pick += [t for t in found if t[:2] == (0., 0.) and t not in pick]
        assert any(t[3] for t in pick), (cid, rad)
        for j, t in enumerate(pick):
            tags = ['ties'] + (['ties_differs'] if t[2] else []) + (['ties_exact'] if t[3] else [])
            f0 = _snap(case, case.f0, t[:2])
            add('ties%d-inside' % j, case.frames, f0, False, tags=tags)
            case_t = _with_f0(case, f0)
            spec = [FULL] * nd
            spec[-2], spec[-1] = ('low', 2.), ('low', 2.)
            fr, f0c = _crop(case_t, spec)
            add('ties%d-clipped' % j, fr, f0c, True, tags=tags)
            for pl in out[-2:]:
                if 'ties' in pl.tags:
                    pl.tie_fraction = t[:2]
        if cid in DTYPE_CELLS and ci == 0:
            fr, f0 = _crop(case, [('low', INSIDE)] * nd)
            fr = fr[..., :fr.shape[-1] - 1 + fr.shape[-1] % 2]   # an odd row length: unaligned rows
            add('corner-low-u16', fr.astype(np.uint16) * 251 + 3, f0, True, tags=['dtype'])
            add('corner-low-f32', fr.astype(np.float32) * 1.5 + 0.125, f0, True, tags=['dtype'])
    return tuple(out)


class _with_f0(D.Case):
    """A case with another start table (for _crop)."""

    def __init__(self, case, f0):
        self.__dict__.update(case.__dict__)
        self.f0 = f0


def _feasible(case, f0):
    """The start of a constrained cluster moved onto its constraints (the unit shape at the
    constraint distance about the cluster's centroid): with every bound pinned nothing else is
    feasible, and the oracle reports an infeasible start as status 3."""
    pc = list(AXES[-case.ndim:])
    dist = 0.7 * np.asarray(case.diameter, float)     # (Case.kwargs)
    f0 = f0.copy()
    for k, cl in enumerate(case.clusters):
        rows = np.flatnonzero(f0['frame'].values == k)
        u = D.UNIT_SHAPES[cl.constraint](case.ndim) * dist
        f0.loc[rows, pc] = u - u.mean(0) + f0.loc[rows, pc].values.mean(0)
    return f0


# ---- the yardstick ------------------------------------------------------------------------------

def _cluster(problem, batch, c):
    a, b = batch.feat_offset[c], batch.feat_offset[c + 1]
    nd = problem.ndim
    radius = np.array([problem.radius[k] for k in range(nd)])
    return batch.params[a:b], batch.frames[int(batch.frame_index[c])], nd, radius


def _cost_on(problem, params, frame, sub):
    if sub is None or len(sub[0]) == 0:
        return np.nan, 0, OUT_OF_BOUNDS
    lay = ref_numpy.Layout([problem.modes[k] for k in range(problem.n_params)], len(params))
    norm = float(frame.max()) ** 2 / problem.residual_factor
    res, _ = ref_numpy.make_objective(lay, params, sub[0], sub[1], sub[2], problem.ndim,
                                      bool(problem.isotropic), norm)
    return np.sqrt(res(lay.pack(params, np.mean)) / problem.residual_factor), len(sub[0]), OK


def numpy_cost(problem, batch, c):
    """(cost, P, status) of cluster c at its start: the reference objective on the start's window."""
    params, frame, nd, radius = _cluster(problem, batch, c)
    return _cost_on(problem, params, frame, ref_numpy.subimage(params[:, 2:2 + nd], frame, radius))


def numpy_yardstick(problem, batch):
    out = [numpy_cost(problem, batch, c) for c in range(batch.n_clusters)]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]),
            np.array([o[2] for o in out], np.int32))


def has_exact_tie(problem, batch, c):
    """Some in-frame pixel of cluster c has a mask sum of exactly 1 (NumPy's evaluation)."""
    params, frame, nd, radius = _cluster(problem, batch, c)
    coords = params[:, 2:2 + nd]
    win = ref_numpy.window(coords, frame.shape, radius)
    if win is None:
        return False
    lo, hi = win
    grid = np.indices(tuple(hi - lo)).T
    return any((np.sum(((grid - (p - lo)) / radius) ** 2, -1) == 1).any() for p in coords)


# ---- the same number with one mistake in the window code --------------------------------------

MUTATIONS = ('shift', 'noclip', 'lt', 'filter')


def mutated_subimage(coords, image, radius, mutation=None, axis=0):
    """``ref_numpy.subimage`` restated with a switch per mistake:
      'shift'   the pixels come from the window moved by one along ``axis`` (the flat index wraps);
      'noclip'  the window is not clipped to the frame (pixels beyond it come from the wrapped flat
                index, as (idx + origin) * stride would give);
      'lt'      the mask is ``< 1`` instead of ``<= 1``;
      'filter'  the in-bounds filter is one tighter on both sides."""
    shape = np.asarray(image.shape)
    c = np.round(coords).astype(int)
    t = 1 if mutation == 'filter' else 0
    keep = np.all((c >= -radius + t) & (c < shape + radius - t), axis=1)
    c = c[keep]
    if len(c) == 0:
        return None
    lo, hi = c.min(0) - radius, c.max(0) + radius + 1
    if mutation != 'noclip':
        lo, hi = np.maximum(lo, 0), np.minimum(hi, shape)
    grid = np.indices(tuple(hi - lo)).T
    rel = (lambda s: s < 1) if mutation == 'lt' else (lambda s: s <= 1)
    dist = []
    for p in coords:    # (the mask lies in the box of +- radius about the centre: only that is evaluated)
        d = np.zeros(grid.shape[:-1], bool)
        b0 = np.clip(np.floor(p - lo - radius).astype(int), 0, hi - lo)
        b1 = np.clip(np.ceil(p - lo + radius).astype(int) + 1, 0, hi - lo)
        box = tuple(slice(i, j) for i, j in zip(b0[::-1], b1[::-1]))     # (grid is transposed)
        d[box] = rel(np.sum(((grid[box] - (p - lo)) / radius) ** 2, -1))
        dist.append(d)
    total = np.any(dist, axis=0).T
    masks = np.array([d.T[total] for d in dist], dtype=bool).reshape(len(coords), -1)
    mesh = np.indices(tuple(hi - lo), dtype=np.float64)[:, total]
    mesh += np.asarray(lo, dtype=np.float64)[:, None]
    strides = np.concatenate([np.cumprod(shape[::-1])[::-1][1:], [1]])
    flat = (mesh.astype(np.int64) * strides[:, None]).sum(0)
    if mutation == 'shift':
        flat += strides[axis]
    return image.ravel()[flat % image.size].astype(np.float64), mesh, masks


def shifted(sub, image, axis):
    """``sub`` (of mutated_subimage) with the pixels one further along ``axis``."""
    shape = np.asarray(image.shape)
    strides = np.concatenate([np.cumprod(shape[::-1])[::-1][1:], [1]])
    flat = (sub[1].astype(np.int64) * strides[:, None]).sum(0) + strides[axis]
    return image.ravel()[flat % image.size].astype(np.float64), sub[1], sub[2]


def mutated_cost(problem, batch, c, mutation=None, axis=0):
    params, frame, nd, radius = _cluster(problem, batch, c)
    return _cost_on(problem, params, frame,
                    mutated_subimage(params[:, 2:2 + nd], frame, radius, mutation, axis))


def cost_on(problem, batch, c, sub):
    params, frame, _, _ = _cluster(problem, batch, c)
    return _cost_on(problem, params, frame, sub)


def moved(a, b, rtol=1e-6):
    """Two (cost, P, status) differ: another status, or costs more than rtol apart."""
    if a[2] != b[2]:
        return True
    if a[2] != OK:
        return False
    return abs(a[0] - b[0]) > rtol * abs(a[0])
