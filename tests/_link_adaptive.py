"""A second statement of the linker with the adaptive search range (clustertracking_amd/link.py's
module text), independent of ``link._assign_adaptive``: brute-force candidates, sub-networks by a
flood fill, the explicit recursion over the sub-networks of a shrinking range, and the optimum of a
sub-network of up to 6 x 6 by exhaustive enumeration (a larger one: a maximum-weight matching of the
profit matrix).  Used by tests/test_link_adaptive_rule.py and tests/test_gpu_link_adaptive.py."""
import numpy as np
from scipy.optimize import linear_sum_assignment

MAX_CANDIDATES, MAX_SOURCES, MAX_DESTINATIONS, ENUMERATE_UP_TO = 10, 30, 64, 6


class GaveUp(Exception):
    def __init__(self, level, size, what):
        Exception.__init__(self, "level %d: %d %s" % (level, size, what))
        self.level, self.size, self.what = level, size, what


def plan(search_range, adaptive_stop, adaptive_step):
    stop_rel = max(float(s) / float(r) for s, r in zip(adaptive_stop, search_range))
    rhos = [1.]
    while rhos[-1] > stop_rel:
        rhos.append(rhos[-1] * adaptive_step)
    return stop_rel, rhos


def scaled_d2(dst, src, sr):
    d2 = 0.
    for a in range(len(sr)):
        df = dst[a] / sr[a] - src[a] / sr[a]
        d2 = d2 + df * df
    return d2


def candidates(dst_pos, src_pos, sr):
    """{(src, dst): d2}: per destination its ten nearest sources within the range"""
    edges = {}
    bound = (1. + 1e-7) * (1. + 1e-7)
    for j, q in enumerate(dst_pos):
        near = sorted((scaled_d2(q, p, sr), i) for i, p in enumerate(src_pos))
        for d2, i in near[:MAX_CANDIDATES]:
            if d2 <= bound:
                edges[(i, j)] = d2
    return edges


def components(edges):
    """the connected components of the edges {(src, dst): d2}: a list of such dicts"""
    by_src, by_dst = {}, {}
    for (i, j) in edges:
        by_src.setdefault(i, []).append(j)
        by_dst.setdefault(j, []).append(i)
    seen, out = set(), []
    for start in sorted(by_dst):
        if ('d', start) in seen:
            continue
        seen.add(('d', start))
        stack, part = [('d', start)], {}
        while stack:
            side, v = stack.pop()
            for o in (by_dst[v] if side == 'd' else by_src[v]):
                e = (o, v) if side == 'd' else (v, o)
                part[e] = edges[e]
                other = ('s' if side == 'd' else 'd', o)
                if other not in seen:
                    seen.add(other)
                    stack.append(other)
        out.append(part)
    return out


def best_by_enumeration(srcs, dsts, edges, rho):
    """(sum of 2 rho^2 - d2, links {dst: src}) of the best set of links, every set tried"""
    best = [0., {}]

    def go(q, taken, total, links):
        if q == len(dsts):
            if total > best[0]:
                best[0], best[1] = total, dict(links)
            return
        go(q + 1, taken, total, links)
        j = dsts[q]
        for i in srcs:
            if i not in taken and (i, j) in edges:
                links[j] = i
                go(q + 1, taken | {i}, total + (2. * (rho * rho) - edges[(i, j)]), links)
                del links[j]
    go(0, frozenset(), 0., {})
    return best[0], best[1]


def best_by_matching(srcs, dsts, edges, rho):
    profit = np.zeros((len(srcs), len(dsts)))
    for (i, j), d2 in edges.items():
        profit[srcs.index(i), dsts.index(j)] = 2. * (rho * rho) - d2
    rows, cols = linear_sum_assignment(profit, maximize=True)
    links = {dsts[c]: srcs[r] for r, c in zip(rows, cols) if (srcs[r], dsts[c]) in edges}
    return sum(2. * (rho * rho) - edges[(i, j)] for j, i in links.items()), links


def resolve(edges, k, stop_rel, rhos, level, links, rounds):
    """one sub-network (its edges) at round k: links and rounds of its destinations, recursing into
    the pieces it falls into at the next range when it is beyond the limits"""
    srcs = sorted({i for i, _ in edges})
    dsts = sorted({j for _, j in edges})
    rho = rhos[k]
    if len(srcs) <= MAX_SOURCES and len(dsts) <= MAX_DESTINATIONS:
        for j in dsts:
            rounds[j] = k
        if len(srcs) == 1 and len(dsts) == 1:
            links[dsts[0]] = srcs[0]
        elif len(srcs) <= ENUMERATE_UP_TO and len(dsts) <= ENUMERATE_UP_TO:
            links.update(best_by_enumeration(srcs, dsts, edges, rho)[1])
        else:
            links.update(best_by_matching(srcs, dsts, edges, rho)[1])
        return
    if rho <= stop_rel:
        if len(srcs) > MAX_SOURCES:
            raise GaveUp(level, len(srcs), 'sources')
        raise GaveUp(level, len(dsts), 'destinations')
    b = rhos[k + 1] * (1. + 1e-7)
    kept = {e: d2 for e, d2 in edges.items() if d2 <= b * b}
    for j in dsts:
        if not any(e[1] == j for e in kept):
            rounds[j] = k + 1
    for part in components(kept):
        resolve(part, k + 1, stop_rel, rhos, level, links, rounds)


def link_levels(levels, search_range, memory, adaptive_stop, adaptive_step):
    """(ids, rounds): two lists of arrays aligned with ``levels``; ``GaveUp`` where the rule fails"""
    ndim = np.asarray(levels[0]).reshape(len(levels[0]), -1).shape[1] if len(levels[0]) else len(np.atleast_1d(search_range))
    sr = [float(v) for v in np.broadcast_to(np.asarray(search_range, dtype=float), (ndim,))]
    stop = [float(v) for v in np.broadcast_to(np.asarray(adaptive_stop, dtype=float), (ndim,))]
    stop_rel, rhos = plan(sr, stop, adaptive_step)
    next_id, ids_out, rounds_out = 0, [], []
    sources = []            # (position, id, levels since it was seen)
    for t, pos in enumerate(levels):
        pos = np.asarray(pos, dtype=float).reshape(-1, ndim)
        ids = [-1] * len(pos)
        rounds = [0] * len(pos)
        links = {}
        if t == 0:
            ids = list(range(len(pos)))
            next_id = len(pos)
        else:
            edges = candidates(pos, [s[0] for s in sources], sr)
            for part in components(edges):
                resolve(part, 0, stop_rel, rhos, t, links, rounds)
            for j, i in links.items():
                ids[j] = sources[i][1]
            born = sorted((tuple(pos[j]), j) for j in range(len(pos)) if j not in links)
            for _, j in born:
                ids[j] = next_id
                next_id += 1
        taken = set(links.values())
        kept = [(p, i, age + 1) for q, (p, i, age) in enumerate(sources) if q not in taken and age + 1 <= memory]
        sources = [(pos[j], ids[j], 0) for j in range(len(pos))] + kept
        ids_out.append(np.array(ids, dtype=np.int64))
        rounds_out.append(np.array(rounds, dtype=np.int32))
    return ids_out, rounds_out


# ---- the inputs that the CPU and the GPU tests share
def blob40():
    """40 points in a 12-box and their displaced, shuffled copy: one sub-network of 40 x 40 at
    search_range 5.  Returns (levels, the row of level 0 behind every row of level 1)."""
    rng = np.random.default_rng(3)
    a = rng.uniform(0, 12, (40, 2))
    perm = rng.permutation(40)
    return [a, (a + rng.normal(0, .3, a.shape))[perm]], perm


def blob100():
    """100 points in a 20-box: at search_range 5 a sub-network of more than 64 destinations"""
    rng = np.random.default_rng(5)
    a = rng.uniform(0, 20, (100, 2))
    return [a, (a + rng.normal(0, .3, a.shape))[rng.permutation(100)]]


def lattice():
    g = np.stack(np.meshgrid(np.arange(6.), np.arange(6.), indexing='ij'), -1).reshape(-1, 2)
    return [g, g.copy()]


def memory_case():
    """five levels, memory 2: every level holds the blob of 40 (oversize at search_range 5), but
    level 2 misses three of its points, whose sources of level 1 no link takes; levels 3 and 4 hold
    them again.  Returns (levels, ids -> the ids that level 2 did not continue)."""
    rng = np.random.default_rng(11)
    a = rng.uniform(0, 12, (40, 2))
    far = np.array([[100., 100.], [110., 100.]])        # something sparse beside the blob
    levels = []
    for t in range(5):
        lvl = (a + rng.normal(0, .1, a.shape))[rng.permutation(40)[:37 if t == 2 else 40]]
        levels.append(np.concatenate([lvl, far + .1 * t]))

    def lost(ids):
        return sorted(set(ids[1]) - set(ids[2]))
    return levels, lost


def eight_levels():
    """eight levels of 20 well-separated walkers; levels 2-3 and 5-6 hold the blob of 40 beside
    them, so levels 3 and 6 (and no other) meet an oversize sub-network"""
    rng = np.random.default_rng(21)
    walkers = np.stack(np.meshgrid(np.arange(5.), np.arange(4.), indexing='ij'), -1).reshape(-1, 2) * 30. + 100.
    blob = rng.uniform(0, 12, (40, 2))
    levels = []
    for t in range(8):
        walkers = walkers + rng.normal(0, .5, walkers.shape)
        lvl = walkers
        if t in (2, 3, 5, 6):
            lvl = np.concatenate([walkers, blob + rng.normal(0, .2, blob.shape)])
        levels.append(lvl[rng.permutation(len(lvl))])
    return levels


def blob3d():
    """40 points in 6 x 12 x 12 and their displaced copy; search_range (2.5, 5, 5) makes them one
    sub-network"""
    rng = np.random.default_rng(9)
    a = rng.uniform(0, 1, (40, 3)) * [6., 12., 12.]
    return [a, (a + rng.normal(0, .2, a.shape) * [.5, 1., 1.])[rng.permutation(40)]]


def six_blobs():
    """one level pair of 600 rows: six blobs of 70 (more oversize roots than the solver's workgroup
    has wavefronts, more rows than it has threads) and 90 sub-networks of 2 x 2"""
    rng = np.random.default_rng(13)
    parts = [rng.uniform(0, 16, (70, 2)) + [200. * b, 0.] for b in range(6)]
    pairs = np.array([[20. * q, 500.] for q in range(90)])
    parts += [pairs, pairs + [0., 2.]]
    a = np.concatenate(parts)
    assert len(a) == 600
    return [a[rng.permutation(600)], (a + rng.normal(0, .3, a.shape))[rng.permutation(600)]]
