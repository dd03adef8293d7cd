"""The yardstick of the characterisation tests: the fixtures of
tests/golden/characterize/characterize_cases.npz and the rule of reference
``find_link.characterize`` composed from NumPy -- used where the reference does not exist.

The two weight tables are trackpy's ``r_squared_mask`` / ``x_squared_masks`` restated from its
published source (trackpy is not installed where the fixtures are made): parity-unpinned for
these two functions, DESIGN.md 7b."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'characterize', 'characterize_cases.npz')


def _offsets(radius):
    """(integer offsets k of the window per axis as a dense grid [ndim, *shape], the boolean
    support sum((k / radius)**2) <= 1 written as trackpy writes it: what is NOT ``> 1`` stays)"""
    points = [np.arange(-r, r + 1) for r in radius]
    grid = np.array(np.meshgrid(*points, indexing='ij'))
    with np.errstate(divide='ignore', invalid='ignore'):
        r = [(g / rad) ** 2 for g, rad in zip(grid, radius)]
        outside = sum(r) > 1
    return grid, outside


def r_squared_mask(radius, ndim):
    """trackpy.masks.r_squared_mask: r^2 of the window offsets inside the ellipse, 0 outside."""
    grid, outside = _offsets(radius)
    r2 = np.sum(grid ** 2, 0).astype(int)
    r2[outside] = 0
    return r2


def x_squared_masks(radius, ndim):
    """trackpy.masks.x_squared_masks: per axis, x^2 of the window offsets inside the ellipse."""
    grid, outside = _offsets(radius)
    masks = np.asarray(grid ** 2, dtype=int)
    masks[:, outside] = 0
    return masks


def window(image, center, radius):
    """The feature's window, zero-padded beyond the frame (reference masks.slice_pad), and its
    corner in frame coordinates."""
    corner = [int(round(c - r)) for c, r in zip(center, radius)]
    shape = [2 * r + 1 for r in radius]
    pad = [(max(-c, 0), max(c + s - n, 0)) for c, s, n in zip(corner, shape, image.shape)]
    start = corner
    if np.any(pad):
        image = np.pad(image, pad, mode='constant')
        start = [max(c, 0) for c in corner]
    return image[tuple(slice(c, c + s) for c, s in zip(start, shape))], corner


def compose(coords, image, radius, isotropic=True, scale_factor=1.):
    """dict of mass, signal, size (or size_z / size_y / size_x) of every row of ``coords``."""
    image = np.asarray(image)
    ndim = image.ndim
    radius = tuple(int(r) for r in radius)
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, ndim)
    n = len(coords)
    mass, signal = np.empty(n), np.empty(n)
    size = np.empty(n) if isotropic else np.empty((n, ndim))
    weights = r_squared_mask(radius, ndim) if isotropic else x_squared_masks(radius, ndim)
    with np.errstate(divide='ignore', invalid='ignore'):
        for i, c in enumerate(coords):
            win, corner = window(image, c, radius)
            rel = c - np.array(corner)
            inside = (np.sum(((np.indices(win.shape).T - rel) / radius) ** 2, -1) <= 1).T
            im = win * inside
            m = np.sum(im)
            mass[i] = m
            signal[i] = np.max(im)
            if isotropic:
                size[i] = np.sqrt(np.sum(weights * im) / m)
            else:
                size[i] = np.sqrt(ndim * np.sum(weights * im, axis=tuple(range(1, ndim + 1))) / m)
    result = dict(mass=mass / scale_factor, signal=signal / scale_factor)
    if isotropic:
        result['size'] = size
    else:
        for a, key in enumerate(['size_z', 'size_y', 'size_x'][3 - ndim:]):
            result[key] = size[:, a]
    return result


def size_keys(ndim, isotropic):
    return ['size'] if isotropic else ['size_z', 'size_y', 'size_x'][3 - ndim:]


def fixtures():
    """[(name, image, coords, kwargs, expected dict)]"""
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(json.loads(str(z['names']))):
        args = json.loads(str(z['args_%d' % i]))
        image = z['image_%d' % i]
        kw = dict(radius=tuple(args['radius']), isotropic=args['isotropic'], scale_factor=args['scale_factor'])
        expect = dict(mass=z['mass_%d' % i], signal=z['signal_%d' % i])
        size = z['size_%d' % i]
        for a, key in enumerate(size_keys(image.ndim, kw['isotropic'])):
            expect[key] = size if kw['isotropic'] else size[:, a]
        out.append((name, image, z['coords_%d' % i], kw, expect))
    return out


def n_window(radius):
    return int(np.prod([2 * r + 1 for r in radius]))


def float_rtol(dtype, radius):
    """Bound of plain summation of the window in the frame's own precision (float frames)."""
    return n_window(radius) * (2. ** -24 if np.dtype(dtype) == np.float32 else 2. ** -53)
