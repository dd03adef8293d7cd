"""The yardstick of the centre-of-mass refinement tests: the rule of
``ctr_refine_com_device`` (include/ctrefine.h) written with ``scipy.ndimage.center_of_mass`` on
``mask * image[window]``, one feature at a time.

The rule is trackpy's ``refine_com`` loop (``trackpy.refine(image, image, radius, coords,
separation=0, characterize=False)``, what the reference's ``find_link(refine=True)`` calls) restated
from its published source -- trackpy is not installed where the fixtures are made -- and made total
by the clip of step 1.  Parity with trackpy itself is not pinned."""
import numpy as np
from scipy import ndimage

import _characterize

MAX_ITERATIONS = 10
SHIFT_THRESH = 0.6


def mask_of(radius):
    """the window offsets with sum((k / radius)**2) <= 1: the support of characterise's weights"""
    return ~_characterize._offsets(tuple(int(r) for r in radius))[1]


def refine_one(image, start, radius, max_iterations=MAX_ITERATIONS, shift_thresh=SHIFT_THRESH):
    """(pos float64 [ndim], mass float64, n_iter, [off of every window evaluated], clipped) of one
    feature; ``clipped``: step 1 moved the rounded start"""
    image = np.asarray(image)
    ndim = image.ndim
    radius = np.array([int(r) for r in radius], dtype=np.int64)
    assert np.all(radius >= 1) and np.all(2 * radius + 1 <= image.shape)
    mask = mask_of(radius)
    lo, hi = radius, np.array(image.shape) - 1 - radius
    rounded = np.rint(np.asarray(start, dtype=np.float64)).astype(np.int64)     # half to even
    c = np.clip(rounded, lo, hi)
    clipped = bool(np.any(c != rounded))
    offs = []
    n_iter = 0
    while True:
        win = image[tuple(slice(ci - r, ci + r + 1) for ci, r in zip(c, radius))]
        # integer frames: exact sums (int64, and float64 products far below 2**53); float frames: float64
        win = win.astype(np.int64) if win.dtype.kind in 'ui' else win.astype(np.float64)
        masked = mask * win
        with np.errstate(divide='ignore', invalid='ignore'):
            cm = np.array(ndimage.center_of_mass(masked), dtype=np.float64)
        m = masked.sum()
        n_iter += 1
        off = cm - radius
        if np.any(np.isnan(cm)):
            off = np.zeros(ndim)
        offs.append(off)
        if np.all(np.abs(off) < shift_thresh) or n_iter >= max_iterations:
            break
        c = np.clip(c + (off > shift_thresh) - (off < -shift_thresh), lo, hi)
    return off + c, float(m), n_iter, offs, clipped


def compose(frames, pos, frame_offset, radius, max_iterations=MAX_ITERATIONS, shift_thresh=SHIFT_THRESH):
    """dict over the rows of ``pos`` [N, ndim] (rows [off[t], off[t + 1]) belong to frames[t]): pos
    float64 [N, ndim], mass float64 [N], n_iter int32 [N], offs (list of lists), clipped bool [N]"""
    frames = np.asarray(frames)
    ndim = frames.ndim - 1
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, ndim)
    out = dict(pos=np.empty((len(pos), ndim)), mass=np.empty(len(pos)), n_iter=np.empty(len(pos), dtype=np.int32),
               offs=[], clipped=np.zeros(len(pos), dtype=bool))
    for t in range(len(frames)):
        for i in range(int(frame_offset[t]), int(frame_offset[t + 1])):
            p, m, n, offs, clipped = refine_one(frames[t], pos[i], radius, max_iterations, shift_thresh)
            out['pos'][i], out['mass'][i], out['n_iter'][i], out['clipped'][i] = p, m, n, clipped
            out['offs'].append(offs)
    return out


def min_gap(offs, shift_thresh=SHIFT_THRESH):
    """the smallest | |off| - shift_thresh | over every window of every row of ``compose()['offs']``"""
    gaps = [np.min(np.abs(np.abs(o) - shift_thresh)) for row in offs for o in row]
    return min(gaps) if gaps else np.inf
