"""The contact rule of ``clustertracking_amd/contacts.py`` (include/ctrefine.h) restated in
NumPy and plain Python, clause by clause: the yardstick of ``test_contacts_rule.py`` and
``test_gpu_contacts.py``, and the builders of their cases.  The entries of a frame are vectorised, what
follows the sort is a loop over the entries.  Nothing here imports the package."""
import collections

import numpy as np

from _pair_correlation import assert_equal_bits

FIELDS = ['n_entries', 'duplicates', 'n_episodes', 'n_pairs', 'status',
          'a', 'b', 'first', 'last', 'lifetime', 'n_seen', 'left_open', 'right_open', 'min_d2', 'max_d2',
          'pair_a', 'pair_b', 'pair_episodes', 'pair_frames', 'pair_first', 'pair_last',
          'first_seen', 'last_seen', 'formed', 'broken', 'active', 'lifetime_count', 'lifetime_above']
Result = collections.namedtuple('Result', FIELDS)
SCALARS, EPISODE, PAIR = FIELDS[:5], FIELDS[5:15], FIELDS[15:21]
OK, BAD_TABLE, OVERFLOW = 0, 1, 2
TILE = 256          # rows of a work item of the device path, and values of a scan tile


def entries(pos, frame_offset, particle, r_off, mpp=1., group=None, pairs='all'):
    """clauses 1 and 3: ``(a, b, frame, d2)`` of every entry, in (frame, i, j) order, and the rows that take part"""
    pos = np.asarray(pos, dtype=np.float64)
    off = np.asarray(frame_offset, dtype=np.int64)
    particle = np.asarray(particle, dtype=np.int64)
    ndim = pos.shape[1]
    q = pos * (np.asarray(mpp, dtype=np.float64) * np.ones(ndim))               # 1: one rounding
    takes = np.isfinite(q).all(1) & (particle >= 0)
    off2 = np.float64(r_off) * np.float64(r_off)                                # 2
    out = [[], [], [], []]
    for t in range(len(off) - 1):
        rows = np.arange(off[t], off[t + 1])
        rows = rows[takes[rows]]
        if not len(rows):
            continue
        d = q[rows][None, :, :] - q[rows][:, None, :]                           # [i, j, axis]: q_j - q_i
        d2 = d[..., 0] * d[..., 0]
        for a in range(1, ndim):
            d2 = d2 + d[..., a] * d[..., a]
        keep = (d2 < off2) & (particle[rows][None, :] > particle[rows][:, None])
        if pairs != 'all':
            same = (group[rows][None, :] == group[rows][:, None]) & (group[rows][:, None] >= 0)
            keep &= same if pairs == 'same' else ~same
        i, j = np.nonzero(keep)                                                 # row-major: i, then ascending j
        out[0].append(particle[rows][i])
        out[1].append(particle[rows][j])
        out[2].append(np.full(len(i), t, dtype=np.int64))
        out[3].append(d2[i, j])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    return cat(out[0], np.int64), cat(out[1], np.int64), cat(out[2], np.int64), cat(out[3], np.float64), takes


def contacts(pos, frame_offset, particle, r_on, r_off=None, gap=0, mpp=1., group=None, pairs='all', max_lifetime=None,
             n_particles=None):
    """clauses 1 to 11 for a table that is not refused, with room for every entry"""
    off = np.asarray(frame_offset, dtype=np.int64)
    particle = np.asarray(particle, dtype=np.int64)
    T = len(off) - 1
    P = (max(int(particle.max()) + 1, 0) if len(particle) else 0) if n_particles is None else int(n_particles)
    r_off = r_on if r_off is None else r_off
    on2 = np.float64(r_on) * np.float64(r_on)
    L = max(T, 1) if max_lifetime is None else int(max_lifetime)
    a, b, frame, d2, takes = entries(pos, off, particle, r_off, mpp, group, pairs)
    n_entries = len(a)
    key = a * P + b                                                             # 4
    order = np.argsort(key, kind='stable')
    key, frame, d2 = key[order].tolist(), frame[order].tolist(), d2[order]
    first_seen, last_seen = np.full(P, T, dtype=np.int64), np.full(P, -1, dtype=np.int64)      # 8
    for t in range(T):
        seen = particle[off[t]:off[t + 1]][takes[off[t]:off[t + 1]]]
        first_seen[seen] = np.minimum(first_seen[seen], t)
        last_seen[seen] = t
    duplicates, chains = 0, []
    for e in range(n_entries):
        if e > 0 and key[e] == key[e - 1] and frame[e] == frame[e - 1]:         # 5
            duplicates += 1
        elif e == 0 or key[e] != key[e - 1] or frame[e] - frame[e - 1] > gap + 1:          # 6
            chains.append([e])
        else:
            chains[-1].append(e)
    rows = []
    formed, broken, active = (np.zeros(T, dtype=np.int64) for _ in range(3))
    count, above = np.zeros((2, L), dtype=np.int64), np.zeros(2, dtype=np.int64)
    for chain in chains:                                                        # 7
        on = [m for m, e in enumerate(chain) if d2[e] < on2]
        if not on:
            continue
        kept = chain[on[0]:]
        pa, pb = divmod(key[kept[0]], P)
        first, last = frame[kept[0]], frame[chain[-1]]
        left = on[0] == 0 and first - max(first_seen[pa], first_seen[pb]) <= gap             # 8
        right = min(last_seen[pa], last_seen[pb]) - last <= gap
        rows.append((pa, pb, first, last, last - first + 1, len(kept), left, right, d2[kept].min(), d2[kept].max()))
        if not left:                                                            # 9
            formed[first] += 1
        if not right:
            broken[last + 1] += 1
        active[first:last + 1] += 1
        life = last - first + 1                                                 # 10
        if life <= L:
            count[1 if left or right else 0, life - 1] += 1
        else:
            above[1 if left or right else 0] += 1
    types = [np.int64] * 6 + [bool] * 2 + [np.float64] * 2
    episode = [np.array([r[c] for r in rows], dtype=dt) for c, dt in enumerate(types)]
    pairs_ = collections.OrderedDict()                                           # 11
    for r in rows:
        pairs_.setdefault((r[0], r[1]), []).append(r)
    pair = [np.array(x, dtype=np.int64) for x in (
        [k[0] for k in pairs_], [k[1] for k in pairs_], [len(v) for v in pairs_.values()],
        [sum(r[4] for r in v) for v in pairs_.values()], [v[0][2] for v in pairs_.values()], [v[-1][3] for v in pairs_.values()])]
    return Result(n_entries, duplicates, len(rows), len(pairs_), OK, *episode, *pair, first_seen, last_seen, formed, broken,
                  active, count, above)


def defaults(n_frames, n_particles, max_lifetime=None, status=BAD_TABLE, n_entries=0):
    """clauses 12 and 13: what a refused table, or one with more entries than room, gives (trimmed columns)"""
    L = max(n_frames, 1) if max_lifetime is None else int(max_lifetime)
    i64 = lambda n, v=0: np.full(n, v, dtype=np.int64)
    return Result(n_entries, 0, 0, 0, status, *(i64(0) for _ in range(6)), np.zeros(0, dtype=bool), np.zeros(0, dtype=bool),
                  np.zeros(0), np.zeros(0), *(i64(0) for _ in range(6)), i64(n_particles, -1), i64(n_particles, -1),
                  i64(n_frames), i64(n_frames), i64(n_frames), np.zeros((2, L), dtype=np.int64), i64(2))


def assert_same(got, want, what=''):
    """every field of two results: the same integers, the same bytes of the doubles"""
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        if name in SCALARS:
            assert int(g) == int(w), (what, name, g, w)
        elif name in ('min_d2', 'max_d2'):
            assert_equal_bits(np.asarray(g), np.asarray(w), (what, name))
        else:
            g, w = np.asarray(g), np.asarray(w)
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, name, g[:8], w[:8])


def of_tensors(res, max_entries):
    """a result of tensors as one of trimmed ndarrays, after a look at the padding: -1 and NaN beyond
    the counts, in columns of ``max_entries`` rows"""
    host = {name: getattr(res, name).cpu().numpy() for name in FIELDS}
    scalars = {name: int(host[name][0]) for name in SCALARS}
    out = dict(scalars)
    for names, m in ((EPISODE, scalars['n_episodes']), (PAIR, scalars['n_pairs'])):
        for name in names:
            col = host[name]
            assert col.shape == (max_entries,), (name, col.shape)
            pad = col[m:]
            assert np.isnan(pad).all() if col.dtype == np.float64 else (pad == -1).all(), name
            out[name] = col[:m].astype(bool) if name in ('left_open', 'right_open') else col[:m]
    for name in FIELDS[21:]:
        out[name] = host[name]
    return Result(**out)


# ---- the cases -----------------------------------------------------------------------------------
R_ON, R_OFF = 11., 13.


def mixed_table(ndim=2, seed=5):
    """``(pos, frame_offset, particle, group, P)``: 40 frames; 10 dimers with a bond near ``R_ON`` and 24 walkers
    in a box of 150, each row dropped with 5 %; three unlinked rows per frame; frames 3 and 20 empty;
    frame 7 with 600 rows (three tiles, three work items), most of them particles of that frame alone;
    NaN positions; particle 4 twice in frame 12; the rows of a frame shuffled, so that the row order is
    not the particle order.  3D: the first axis is stored halved, for ``mpp = (2, 1, 1)``.  group: the
    dimer of a dimer's particle, a group of its own for every other particle, -2 for unlinked rows."""
    rng = np.random.RandomState(seed)
    T, box, n_dimers, n_walkers = 40, 150., 10, 24
    n_tracked = 2 * n_dimers + n_walkers
    centre = rng.uniform(20, box - 20, (n_dimers, ndim))
    walker = rng.uniform(0, box, (n_walkers, ndim))
    pos, particle, off = [], [], [0]
    extra = n_tracked
    for t in range(T):
        centre = centre + rng.normal(0, 1.2, centre.shape)
        walker = walker + rng.normal(0, 4., walker.shape)
        rows, ids = [], []
        if t not in (3, 20):
            for k in range(n_dimers):
                u = rng.normal(0, 1, ndim)
                u *= 5. / np.sqrt((u * u).sum())
                for m, sign in enumerate((-1., 1.)):
                    rows.append(centre[k] + sign * u + rng.normal(0, 0.6, ndim))
                    ids.append(2 * k + m)
            rows += list(walker)
            ids += list(range(2 * n_dimers, n_tracked))
            keep = rng.uniform(size=len(rows)) > 0.05
            rows, ids = [r for r, k in zip(rows, keep) if k], [i for i, k in zip(ids, keep) if k]
            for _ in range(3):
                rows.append(rng.uniform(0, box, ndim))
                ids.append(-1)
            if t == 12:
                rows.append(centre[2] + rng.normal(0, 2., ndim))
                ids.append(4)
            if t == 7:
                while len(rows) < 600:
                    rows.append(rng.uniform(0, box, ndim))
                    ids.append(extra if len(rows) % 9 else -1)
                    extra += 1 if ids[-1] >= 0 else 0
            order = rng.permutation(len(rows))
            rows, ids = [rows[o] for o in order], [ids[o] for o in order]
        pos += rows
        particle += ids
        off.append(len(pos))
    pos = np.array(pos, dtype=np.float64).reshape(-1, ndim)
    particle = np.array(particle, dtype=np.int64)
    off = np.array(off, dtype=np.int64)
    for r in (5, off[7] + 300, off[30] + 2):
        pos[r, r % ndim] = np.nan
    if ndim == 3:
        pos[:, 0] /= 2.
    group = np.where(particle < 0, -2, np.where(particle < 2 * n_dimers, particle // 2, 1000 + particle)).astype(np.int64)
    return pos, off, particle, group, extra


MIXED_MPP = {2: 1., 3: (2., 1., 1.)}


def dense_frames(seed=11):
    """``(pos, frame_offset, particle)``: 300 particles inside a disc of diameter 12 < ``R_OFF`` in frames 1, 2 and
    3 -- 44 850 entries per frame, 526 scan tiles in all: more than one trip of the scan over the tiles'
    sums -- and far apart from each other in frames 0 and 4; frame 5 is empty."""
    rng = np.random.RandomState(seed)
    n = 300
    pos, particle, off = [], [], [0]
    for t in range(5):
        if t in (0, 4):
            rows = np.stack([np.arange(n) * 40., np.full(n, 1000. * t)], axis=1)
        else:
            r, phi = 6. * np.sqrt(rng.uniform(size=n)), rng.uniform(0, 2 * np.pi, n)
            rows = np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)
        order = rng.permutation(n)
        pos.append(rows[order])
        particle.append(order)
        off.append(off[-1] + n)
    off.append(off[-1])
    return np.concatenate(pos), np.array(off, dtype=np.int64), np.concatenate(particle).astype(np.int64)


LONG_T = 3000
LONG_R_ON, LONG_R_OFF, LONG_GAP = 6., 8., 1


def long_chain():
    """``(pos, frame_offset, particle, episodes)``: particles 0 and 1 over 3000 frames, 5 apart (d2 = 25, on) but:
    particle 1 is missing in frame 100 (bridged by gap 1) and in frames 500, 501 (not bridged); both are
    missing in 1200 .. 1202; they are 7 apart (d2 = 49, in the band) in 1203 .. 1205 and in 2500 .. 2510,
    and 9 apart (beyond ``r_off``) in frame 2000 (bridged).  The episodes at ``LONG_R_ON, LONG_R_OFF, LONG_GAP``,
    written by hand: ``(a, b, first, last, lifetime, n_seen, left_open, right_open, min_d2, max_d2)``."""
    pos, particle, off = [], [], [0]
    for t in range(LONG_T):
        if not 1200 <= t <= 1202:
            dist = 9. if t == 2000 else 7. if 1203 <= t <= 1205 or 2500 <= t <= 2510 else 5.
            pos.append((0., 3.))
            particle.append(0)
            if t not in (100, 500, 501):
                pos.append((dist, 3.))
                particle.append(1)
        off.append(len(pos))
    episodes = [(0, 1, 0, 499, 500, 499, True, False, 25., 25.),         # open at the table's first frame
                (0, 1, 502, 1199, 698, 698, False, False, 25., 25.),
                (0, 1, 1206, 2999, 1794, 1793, False, True, 25., 49.)]   # begins in the band: not left_open
    return np.array(pos, dtype=np.float64), np.array(off, dtype=np.int64), np.array(particle, dtype=np.int64), episodes
