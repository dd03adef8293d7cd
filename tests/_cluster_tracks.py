"""The cluster-track rule (include/ctrefine.h) restated with plain loops and
``scipy.sparse.csgraph.connected_components``: the yardstick of the device path.  No engine, no
oracle.  Also the generators of the test tables, and a vectorised NumPy form that serves as the
host baseline of ``tools/cluster_tracks_time.py``."""
import collections
import itertools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

Tracks = collections.namedtuple('Tracks', ['track_of_particle', 'n_tracks', 'n_members'])


def cluster_tracks(frame_offset, particle, cluster, cluster_size, min_frames=1, n_particles=None):
    frame_offset = np.asarray(frame_offset, dtype=np.int64)
    particle = np.asarray(particle, dtype=np.int64)
    cluster = np.asarray(cluster, dtype=np.int64)
    P = int(n_particles) if n_particles is not None else (max(int(particle.max()) + 1, 0) if len(particle) else 0)
    bonds = collections.Counter()
    for t in range(len(frame_offset) - 1):
        groups = collections.defaultdict(list)
        for i in range(frame_offset[t], frame_offset[t + 1]):
            groups[int(cluster[i])].append(int(particle[i]))
        for members in groups.values():
            if len(members) != cluster_size or min(members) < 0 or len(set(members)) != cluster_size:
                continue
            for p, q in itertools.combinations(sorted(members), 2):
                bonds[(p, q)] += 1
    edges = [pq for pq, b in bonds.items() if b >= min_frames]
    rows = np.array([e[0] for e in edges], dtype=np.int64)
    cols = np.array([e[1] for e in edges], dtype=np.int64)
    graph = coo_matrix((np.ones(len(edges)), (rows, cols)), shape=(P, P))
    _, label = connected_components(graph, directed=False) if P else (0, np.zeros(0, dtype=np.int64))
    size = np.bincount(label, minlength=1) if P else np.zeros(0, dtype=np.int64)
    track_of = np.full(P, -1, dtype=np.int32)
    n_members = []
    number = {}
    for p in range(P):                      # ascending: a component is numbered at its smallest id
        if size[label[p]] < 2:
            continue
        if label[p] not in number:
            number[label[p]] = len(number)
            n_members.append(size[label[p]])
        track_of[p] = number[label[p]]
    return Tracks(track_of, len(number), np.array(n_members, dtype=np.int32))


def track_positions(pos, frame_offset, particle, track_of_particle, n_tracks, cluster_size):
    pos = np.asarray(pos, dtype=np.float64)
    frame_offset = np.asarray(frame_offset, dtype=np.int64)
    T, ndim = len(frame_offset) - 1, pos.shape[1]
    out = np.full((n_tracks, T, cluster_size, ndim), np.nan)
    present = np.zeros((n_tracks, T), dtype=np.int32)
    for t in range(T):
        rows = collections.defaultdict(list)
        for i in range(frame_offset[t], frame_offset[t + 1]):
            p = int(particle[i])
            if p >= 0 and track_of_particle[p] >= 0:
                rows[int(track_of_particle[p])].append((p, i))
        for k, members in rows.items():
            present[k, t] = len(members)
            if len(members) == cluster_size:
                for j, (_, i) in enumerate(sorted(members)):
                    out[k, t, j] = pos[i]
    return out, present


def tracks_vectorised(frame_offset, particle, cluster, pos, cluster_size, min_frames=1):
    """The same rule in vectorised NumPy + SciPy: what a user would write on the host.  Returns
    ``(track_of_particle, n_tracks, pos_out, present)``; timed as a baseline, checked against the loops."""
    frame_offset = np.asarray(frame_offset, dtype=np.int64)
    particle = np.asarray(particle, dtype=np.int64)
    cluster = np.asarray(cluster, dtype=np.int64)
    N, T = len(particle), len(frame_offset) - 1
    P = max(int(particle.max()) + 1, 0) if N else 0
    frame = np.repeat(np.arange(T, dtype=np.int64), np.diff(frame_offset))
    rows = np.arange(frame_offset[0], frame_offset[-1])
    par, clu = particle[rows], cluster[rows]
    order = np.lexsort((par, clu, frame))
    fr, cl, pa = frame[order], clu[order], par[order]
    new = np.r_[True, (fr[1:] != fr[:-1]) | (cl[1:] != cl[:-1])] if len(order) else np.zeros(0, dtype=bool)
    first = np.flatnonzero(new)
    count = np.diff(np.r_[first, len(order)])
    first = first[count == cluster_size]
    members = pa[first[:, None] + np.arange(cluster_size)[None, :]]      # sorted by particle
    ok = (members[:, 0] >= 0) & (np.diff(members, axis=1) > 0).all(axis=1)
    members = members[ok]
    a, b = np.triu_indices(cluster_size, 1)
    keys = (members[:, a] << 32 | members[:, b]).reshape(-1)
    uniq, cnt = np.unique(keys, return_counts=True)
    uniq = uniq[cnt >= min_frames]
    graph = coo_matrix((np.ones(len(uniq)), (uniq >> 32, uniq & 0xffffffff)), shape=(P, P))
    _, label = connected_components(graph, directed=False) if P else (0, np.zeros(0, dtype=np.int64))
    size = np.bincount(label, minlength=1) if P else np.zeros(0, dtype=np.int64)
    smallest = np.full(len(size), P, dtype=np.int64)
    np.minimum.at(smallest, label, np.arange(P))
    is_track = size >= 2
    number = np.full(len(size), -1, dtype=np.int64)
    roots = np.sort(smallest[is_track])
    number[label[roots]] = np.arange(len(roots))
    track_of = number[label].astype(np.int32) if P else np.zeros(0, dtype=np.int32)
    n_tracks = len(roots)
    trk = np.where(par >= 0, track_of[np.maximum(par, 0)], -1) if N else np.zeros(0, dtype=np.int32)
    sel = np.flatnonzero(trk >= 0)
    present = np.zeros((n_tracks, T), dtype=np.int32)
    np.add.at(present, (trk[sel], frame[sel]), 1)
    order = sel[np.lexsort((rows[sel], par[sel], frame[sel], trk[sel]))]
    full = present[trk[order], frame[order]] == cluster_size
    order = order[full]
    out = np.full((n_tracks, T, cluster_size, pos.shape[1]), np.nan)
    out.reshape(-1, pos.shape[1])[(trk[order] * T + frame[order]) * cluster_size
                                  + np.arange(len(order)) % cluster_size] = pos[rows[order]]
    return track_of, n_tracks, out, present


# ---- tables ----
def table(frames):
    """frames: a list (one per frame) of lists of (particle, cluster) or (particle, cluster, pos) rows.
    Returns (frame_offset, particle, cluster, pos [N, 2]); a row without a position gets a distinct one."""
    off, par, clu, pos = [0], [], [], []
    for rows in frames:
        for row in rows:
            par.append(row[0])
            clu.append(row[1])
            pos.append(row[2] if len(row) > 2 else (len(pos) + 0.25, 2. * len(pos) + 0.5))
        off.append(len(par))
    return (np.array(off, dtype=np.int64), np.array(par, dtype=np.int64), np.array(clu, dtype=np.int64),
            np.array(pos, dtype=np.float64).reshape(-1, 2))


def chain_table(n, star=False, seed=0):
    """n particles with shuffled ids, cluster_size 2, one bond per frame: a path i - i + 1 (or a star
    0 - i), every bond in a frame of its own.  The largest component has n members."""
    ids = np.random.RandomState(seed).permutation(n).astype(np.int64)
    a = np.zeros(n - 1, dtype=np.int64) if star else np.arange(n - 1)
    b = np.arange(1, n)
    particle = np.stack([ids[a], ids[b]], axis=1).reshape(-1)
    cluster = np.repeat(np.arange(n - 1, dtype=np.int64) % 7, 2)
    return np.arange(0, 2 * n - 1, 2, dtype=np.int64), particle, cluster


def random_video(seed, n_frames=40, n_clusters=30, cluster_size=2, ndim=2, extra=0, p_drop=0.1, p_stranger=0.1,
                 p_touch=0.05, p_relabel=0.03, p_unlinked=0.02):
    """A seeded video of clusters with what goes wrong in practice: features dropped, strangers
    within `separation` (a group one too large), two clusters touching (one group of both), ids
    changed mid-track, unlinked rows; cluster labels restart in every frame (and some are negative).
    extra: lone particles per frame.  Returns (frame_offset, particle, cluster, pos [N, ndim])."""
    rng = np.random.RandomState(seed)
    ids = np.arange(n_clusters * cluster_size, dtype=np.int64).reshape(n_clusters, cluster_size)
    ids = rng.permutation(ids.size).astype(np.int64).reshape(ids.shape)
    next_id = ids.size
    lone = np.arange(next_id, next_id + extra, dtype=np.int64)
    next_id += extra
    off, par, clu = [0], [], []
    for t in range(n_frames):
        label = rng.permutation(n_clusters + 4) - 2        # labels of this frame, some negative
        touch = {}
        for c in range(0, n_clusters - 1, 2):
            if rng.rand() < p_touch:
                touch[c + 1] = c
        for c in range(n_clusters):
            for j in range(cluster_size):
                if rng.rand() < p_relabel:
                    ids[c, j] = next_id
                    next_id += 1
                if rng.rand() < p_drop:
                    continue
                par.append(-1 if rng.rand() < p_unlinked else ids[c, j])
                clu.append(label[touch.get(c, c)])
            if rng.rand() < p_stranger:
                par.append(next_id)
                next_id += 1
                clu.append(label[c])
        for p in lone:
            par.append(p)
            clu.append(1000 + p)
        off.append(len(par))
    order = np.concatenate([o + rng.permutation(n) for o, n in zip(off[:-1], np.diff(off))]) if par else np.zeros(0, int)
    par, clu = np.array(par, dtype=np.int64)[order], np.array(clu, dtype=np.int64)[order]
    pos = rng.uniform(0, 512, (len(par), ndim))
    return np.array(off, dtype=np.int64), par, clu, pos


def clean_video(seed, n_frames, n_clusters, cluster_size, ndim, spread=3.):
    """Every cluster complete in every frame, one group per cluster and frame, positions of a
    drifting rigid-ish cluster: where this rule and orientation_df(track_column=...) coincide."""
    rng = np.random.RandomState(seed)
    ids = rng.permutation(n_clusters * cluster_size).astype(np.int64).reshape(n_clusters, cluster_size)
    centre = rng.uniform(20, 200, (n_clusters, ndim))
    shape = rng.uniform(-spread, spread, (n_clusters, cluster_size, ndim))
    off, par, clu, pos = [0], [], [], []
    for t in range(n_frames):
        centre = centre + rng.normal(0, 0.3, centre.shape)
        for c in rng.permutation(n_clusters):
            for j in rng.permutation(cluster_size):
                par.append(ids[c, j])
                clu.append(c)
                pos.append(centre[c] + shape[c, j] + rng.normal(0, 0.1, ndim))
        off.append(len(par))
    return (np.array(off, dtype=np.int64), np.array(par, dtype=np.int64), np.array(clu, dtype=np.int64),
            np.array(pos, dtype=np.float64))


# ---- hand-written known answers: name -> (frames, cluster_size, min_frames, expected) ----
# expected: track_of_particle, n_members, present [n_tracks][T]
A, B, C, D, E = 0, 1, 2, 3, 4
KNOWN = {
    'one_dimer_three_frames': (
        [[(A, 7), (B, 7)], [(B, 3), (A, 3)], [(A, 7), (B, 7)]], 2, 1,
        ([0, 0], [2], [[2, 2, 2]])),
    # A-B, then the linker loses B and calls it B' (= C): one track of three members, no conflict
    'lost_and_renamed': (
        [[(A, 0), (B, 0)], [(A, 0), (B, 0)], [(A, 1), (C, 1)], [(A, 1), (C, 1)]], 2, 1,
        ([0, 0, 0], [3], [[2, 2, 2, 2]])),
    # two dimers; in frame 1 they touch: one group of four bonds nothing, and both keep the frame
    'two_dimers_touch': (
        [[(A, 0), (B, 0), (C, 1), (D, 1)], [(A, 5), (B, 5), (C, 5), (D, 5)], [(A, 0), (B, 0), (C, 1), (D, 1)]], 2, 1,
        ([0, 0, 1, 1], [2, 2], [[2, 2, 2], [2, 2, 2]])),
    # A-B seen three times, C-D twice: min_frames = 3 keeps the first alone
    'bond_below_min_frames': (
        [[(A, 0), (B, 0), (C, 1), (D, 1)], [(A, 0), (B, 0), (C, 1), (D, 1)], [(A, 0), (B, 0), (C, 2), (D, 3)]], 2, 3,
        ([0, 0, -1, -1], [2], [[2, 2, 2]])),
    'bond_at_min_frames': (
        [[(A, 0), (B, 0), (C, 1), (D, 1)], [(A, 0), (B, 0), (C, 1), (D, 1)], [(A, 0), (B, 0), (C, 2), (D, 3)]], 2, 2,
        ([0, 0, 1, 1], [2, 2], [[2, 2, 2], [2, 2, 2]])),
    # frame 0: a group of two rows of the same particle is not complete
    'duplicate_particle': (
        [[(A, 0), (A, 0), (B, 1), (C, 1)], [(B, 1), (C, 1)]], 2, 1,
        ([-1, 0, 0], [2], [[2, 2]])),
    # a group with an unlinked row is not complete; the trimer is bonded in frame 1 alone
    'negative_particle': (
        [[(A, 0), (-1, 0), (B, 0)], [(A, 0), (C, 0), (B, 0)], [(A, 4), (-1, 4), (C, 4)]], 3, 1,
        ([0, 0, 0], [3], [[2, 3, 2]])),
    # A-B, later A-B' (= C) while B is still there: three member rows in frame 2, a conflict
    'conflict_frame': (
        [[(A, 0), (B, 0)], [(A, 0), (C, 0), (B, 9)], [(A, 0), (B, 0), (C, 9)]], 2, 1,
        ([0, 0, 0], [3], [[2, 3, 3]])),
    # E is alone in its group in every frame
    'singleton': (
        [[(A, 0), (B, 0), (E, 2)], [(A, 0), (B, 0), (E, 2)]], 2, 1,
        ([0, 0, -1, -1, -1], [2], [[2, 2]])),
    # ids shuffled: the tracks are numbered by their smallest particle id, {0, 4} {1, 3} {2, 5}
    'numbering': (
        [[(5, 0), (2, 0), (3, 1), (1, 1), (4, 2), (0, 2)]], 2, 1,
        ([0, 1, 2, 1, 0, 2], [2, 2, 2], [[2], [2], [2]])),
}


def known(name):
    frames, cs, mf, (track_of, n_members, present) = KNOWN[name]
    return table(frames), cs, mf, (np.array(track_of, dtype=np.int32), np.array(n_members, dtype=np.int32),
                                   np.array(present, dtype=np.int32).reshape(len(n_members), len(frames)))
