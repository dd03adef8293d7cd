"""The yardstick of the feature-location tests: the fixtures of
tests/golden/locate/locate_cases.npz and the rule of reference ``find.grey_dilation`` composed from
NumPy, SciPy and the host ``drop_close`` -- used where the reference does not exist."""
import json
import os

import numpy as np
from scipy import ndimage

from clustertracking_amd.find import drop_close, percentile_threshold
from clustertracking_amd.utils import validate_tuple

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'locate', 'locate_cases.npz')


def fixtures():
    """[(name, frame, kwargs, expected positions, expected threshold)]"""
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(json.loads(str(z['names']))):
        args = json.loads(str(z['args_%d' % i]))
        sep = args['separation']
        margin = args['margin']
        kw = dict(separation=tuple(sep) if isinstance(sep, list) else sep, percentile=args['percentile'],
                  margin=tuple(margin) if isinstance(margin, list) else margin, precise=args['precise'])
        out.append((name, z['frame_%d' % i], kw, z['pos_%d' % i], float(z['thr_%d' % i])))
    return out


def compose(frame, separation, percentile=64, margin=None, precise=True):
    """np.percentile + scipy.ndimage.grey_dilation + drop_close, step by step."""
    ndim = frame.ndim
    separation = validate_tuple(separation, ndim)
    if margin is None:
        margin = tuple(int(s / 2) for s in separation)
    thr = percentile_threshold(frame, percentile)
    if np.isnan(thr):
        return np.empty((0, ndim))
    box = [int(2 * s / np.sqrt(ndim)) for s in separation]
    peak = (frame == ndimage.grey_dilation(frame, box, mode='constant')) & (frame > thr)
    pos = np.argwhere(peak)
    value = frame[peak]
    inside = ~np.any((pos < margin) | (pos > np.array(frame.shape) - margin - 1), 1)
    pos, value = pos[inside], value[inside]
    if len(pos) == 0:
        return np.empty((0, ndim))
    if precise:
        pos = drop_close(pos, separation, value)
    return pos
