"""A second statement of the linker with prediction (clustertracking_amd/link.py's module text),
independent of ``link.link_levels``: plain loops over rows and axes, brute-force candidates, the
sub-networks and their optimum from tests/_link_adaptive.py (flood fill, exhaustive enumeration up
to 6 x 6, a maximum-weight matching beyond).  Without ``adaptive_stop`` every sub-network is
resolved at rho = 1.  Also the inputs that tests/test_link_predict_rule.py and
tests/test_gpu_link_predict.py share."""
import numpy as np

from _link_adaptive import blob40, candidates, components, plan, resolve

PARTS = 256


def own_velocity(p, t, source):
    return [(p[a] - source[0][a]) / float(t - source[2]) for a in range(len(p))]


def drift_sum(q, linked, axis):
    """S_a over one level in the order of the rule; q: per row a list or None"""
    part = [0.] * PARTS
    for l in range(PARTS):
        for i in range(l, len(q), PARTS):
            if linked[i]:
                part[l] += q[i][axis]
    h = PARTS // 2
    while h:
        for l in range(h):
            part[l] += part[l + h]
        h //= 2
    return part[0]


def link_levels(levels, search_range, memory, predictor, initial_velocity=None, adaptive_stop=None,
                adaptive_step=.95):
    """(ids, velocities, rounds): three lists of arrays aligned with ``levels``"""
    ndim = next((np.asarray(l).shape[1] for l in levels if len(l)), len(np.atleast_1d(search_range)))
    sr = [float(v) for v in np.broadcast_to(np.asarray(search_range, dtype=float), (ndim,))]
    v0 = [0.] * ndim if initial_velocity is None else [float(v) for v in np.broadcast_to(initial_velocity, (ndim,))]
    if adaptive_stop is None:
        stop_rel, rhos = 1., [1.]
    else:
        stop_rel, rhos = plan(sr, [float(v) for v in np.broadcast_to(adaptive_stop, (ndim,))], adaptive_step)
    next_id, ids_out, vel_out, rounds_out = 0, [], [], []
    sources = []            # (position, id, level, velocity)
    u = list(v0)            # the drift of the last level
    for t, pos in enumerate(levels):
        pos = [[float(x) for x in row] for row in np.asarray(pos, dtype=float).reshape(-1, ndim)]
        n = len(pos)
        ids, rounds, links = [-1] * n, [0] * n, {}
        if t == 0:
            ids = list(range(n))
            next_id = n
            w = [list(v0) for _ in range(n)]
        else:
            offered = []
            for p, _, ts, ws in sources:
                v = u if predictor == 'drift' else ws
                offered.append([p[a] + v[a] * float(t - ts) for a in range(ndim)])
            edges = candidates(pos, offered, sr)
            for part in components(edges):
                resolve(part, 0, stop_rel, rhos, t, links, rounds)
            for j, i in links.items():
                ids[j] = sources[i][1]
            for _, j in sorted((tuple(pos[j]), j) for j in range(n) if j not in links):
                ids[j] = next_id
                next_id += 1
            linked = [j in links for j in range(n)]
            q = [own_velocity(pos[j], t, sources[links[j]]) if linked[j] else None for j in range(n)]
            if predictor == 'drift':
                m = sum(linked)
                if m:
                    u = [drift_sum(q, linked, a) / float(m) for a in range(ndim)]
                w = [list(u) for _ in range(n)]
            else:
                w = []
                for i in range(n):
                    if linked[i]:
                        w.append(q[i])
                        continue
                    best, at = None, -1
                    for j in range(n):
                        if not linked[j]:
                            continue
                        d2 = 0.
                        for a in range(ndim):
                            df = pos[i][a] / sr[a] - pos[j][a] / sr[a]
                            d2 = d2 + df * df
                        if at < 0 or d2 < best:
                            best, at = d2, j
                    w.append(list(q[at]) if at >= 0 else list(v0))
        taken = set(links.values())
        kept = [s for k, s in enumerate(sources) if k not in taken and t - s[2] <= memory]
        sources = [(pos[j], ids[j], t, w[j]) for j in range(n)] + kept
        ids_out.append(np.array(ids, dtype=np.int64))
        vel_out.append(np.array(w, dtype=np.float64).reshape(n, ndim))
        rounds_out.append(np.array(rounds, dtype=np.int32))
    return ids_out, vel_out, rounds_out


def n_ids(ids):
    return len(set(np.concatenate(ids).tolist()))


# ---- the inputs that the CPU and the GPU tests share: a 5 x 6 grid of spacing 10, search_range 1.5,
# ---- Gaussian noise of at most 0.1 px
SEARCH_RANGE = 1.5


def grid():
    return np.stack(np.meshgrid(np.arange(5.), np.arange(6.), indexing='ij'), -1).reshape(-1, 2) * 10. + 20.


def noise(rng, shape):
    return np.clip(rng.normal(0, .04, shape), -.1, .1)


FLOW = (.3, 3.)


def flow(n_levels=6, step=FLOW, seed=1):
    rng = np.random.default_rng(seed)
    g = grid()
    return [g + t * np.asarray(step) + noise(rng, g.shape) for t in range(n_levels)]


def ramp():
    """10 levels; the step into level t is 0.4 t along x"""
    rng = np.random.default_rng(2)
    g, x, out = grid(), 0., []
    for t in range(10):
        x += .4 * t
        out.append(g + [0., x] + noise(rng, g.shape))
    return out


def shear():
    """9 levels; the rows with y < 40 move +x, the others -x, by min(0.5 t, 2.5) into level t; from
    level 6 on one more row travels inside the +x stream"""
    rng = np.random.default_rng(3)
    g = grid()
    sign = np.where(g[:, 0] < 40., 1., -1.)
    x, out = 0., []
    for t in range(9):
        x += min(.5 * t, 2.5)
        lvl = g + np.stack([np.zeros(len(g)), sign * x], -1)
        if t >= 6:
            lvl = np.concatenate([lvl, [[25., 45. + x]]])
        out.append(lvl + noise(rng, lvl.shape))
    return out


def dropout():
    """flow (0, 3) over 7 levels; row 0 is absent at levels 3 and 4.  Returns (levels, the row of
    the grid's row 0 per level or None)"""
    levels = flow(7, (0., 3.), seed=4)
    for t in (3, 4):
        levels[t] = levels[t][1:]
    return levels, [None if t in (3, 4) else 0 for t in range(7)]


def empty_level():
    levels = flow(5, seed=5)
    levels[2] = np.zeros((0, 2))
    return levels


def wide_level():
    """one level pair: 300 rows on a 15 x 20 grid in uniform flow, and 40 births shuffled in among
    the 300 of level 1: more rows than a workgroup has threads"""
    rng = np.random.default_rng(6)
    g = np.stack(np.meshgrid(np.arange(15.), np.arange(20.), indexing='ij'), -1).reshape(-1, 2) * 10. + 20.
    born = np.stack(np.meshgrid(np.arange(5.), np.arange(8.), indexing='ij'), -1).reshape(-1, 2) * 30. + 25.
    second = np.concatenate([g + FLOW, born])
    second = second + noise(rng, second.shape)
    return [g + noise(rng, g.shape), second[rng.permutation(len(second))]]


SEARCH_RANGE_3D = (1., 1.5, 1.5)
FLOW_3D = (.2, -.3, 3.)


def flow3d():
    rng = np.random.default_rng(7)
    g = np.stack(np.meshgrid(np.arange(3.), np.arange(3.), np.arange(4.), indexing='ij'), -1).reshape(-1, 3) * 10. + 20.
    return [g + t * np.asarray(FLOW_3D) + noise(rng, g.shape) for t in range(5)]


def shifted_blob():
    """``blob40`` of the adaptive tests (one sub-network of 40 x 40 at search_range 5) with level 1
    shifted by (3, 3)"""
    (a, b), perm = blob40()
    return [a, b + 3.], perm
