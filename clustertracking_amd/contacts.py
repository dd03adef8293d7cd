"""Contact episodes and bond lifetimes of linked particles on the MI355X: *how long* two particles stay
together.  g(r) (``pair_correlation``) gives the bond length, ``neighbors`` says how close rows come and
``twopoint`` whether they move together; the time two particles spend within reach of each other is what
separates a bonded cluster from a collision, what ``min_frames`` of ``cluster_tracks`` is compared with,
and for self-assembling or flexible clusters the physics itself: association and dissociation rates and
the survival curve of a bond.  The pair is the only unit that exists in every frame of every sample,
whatever the sizes of its clusters.  The reference has nothing here; its users loop in pandas over a
kd-tree per frame.

Two knobs keep a lifetime from measuring the localisation noise and the dropout rate instead of the
bonds: hysteresis (a contact switches on below ``r_on`` and off at ``r_off >= r_on``, a Schmitt trigger)
and gap bridging (up to ``gap`` frames without the pair do not end a contact).

The rule is the project's own (``include/ctrefine.h`` has it too; ``tests/_contacts.py``
restates it in NumPy).  Everything returned is an integer or a minimum / maximum of doubles, so it
equals the restatement exactly and every call returns the same bytes.

1. Inputs.  ``pos`` float64 ``[N, ndim]``, ndim 2 or 3, rows sorted by frame; ``frame_offset`` int64
   ``[T + 1]``; ``particle`` int64 ``[N]``, dense ids ``0 .. P - 1``, negative = unlinked: what
   ``find_link_arrays``, ``link_arrays`` and ``subtract_drift_arrays`` return.  ``q = pos * mpp`` per axis, one
   rounding.  A row *takes part* when every coordinate of ``q`` is finite and ``particle >= 0``.
2. Thresholds.  ``r_on > 0``, ``r_off >= r_on`` (default ``r_on``), in the units of ``pos * mpp``; ``on2 = r_on *
   r_on`` and ``off2 = r_off * r_off`` are computed once on the host.  ``gap`` is an int ``>= 0``.
3. Entries.  For every frame ``t`` and every ordered pair of rows ``(i, j)`` of that frame that take part,
   with ``particle[i] < particle[j]`` and ``d2 < off2``, there is an *entry* ``(a = particle[i], b =
   particle[j], t, d2)``; ``d2`` is the sum over the axes, in axis order, of the squared differences, every
   product and sum rounded on its own (``pair_walk``'s).  ``group`` with ``pairs='same'`` / ``'other'`` filters
   the entries as clause 6 of g(r) does.  The entries of row ``i`` are emitted in ascending ``j``; entries
   lie in (frame, ``i``, ``j``) order.  ``n_entries`` counts them.
4. Pair order.  The entries are sorted stably by ``key = a * P + b`` (``P <= 2^31 - 1``, so the key is below
   ``2^62``); within a pair they stay in frame order.
5. Duplicates.  An entry with the key and the frame of the entry before it can only come from a particle
   repeated in a frame; it is a *duplicate*: counted in ``duplicates`` and otherwise ignored.  The first
   in (frame, ``i``, ``j``) order counts.
6. Chains.  An entry that is no duplicate *heads a chain* when it is the first of its pair, or when its
   frame exceeds the frame of the entry before it by more than ``gap + 1``.  So up to ``gap`` frames
   without an entry are bridged, whether one of the two particles was missing in them or the two were
   ``r_off`` or more apart: the rule does not tell the two apart.
7. Episodes.  A chain holds at most one episode.  It begins at the chain's first entry with ``d2 < on2``
   and ends at the chain's last entry; a chain without such an entry has no episode.  Its fields: ``a``,
   ``b``; ``first``, ``last`` (frames); ``lifetime = last - first + 1``; ``n_seen``, the entries that are no
   duplicates from the first on-entry on; ``min_d2``, ``max_d2`` over those.
8. Censoring.  ``first_seen[p]`` / ``last_seen[p]`` are the first and last frame with a row of ``p`` that takes
   part; ``T`` and ``-1`` for a particle that never does.  An episode is ``left_open`` when its first on-entry
   heads the chain and ``first - max(first_seen[a], first_seen[b]) <= gap``; ``right_open`` when
   ``min(last_seen[a], last_seen[b]) - last <= gap``; *complete* when neither holds.
9. Series, int64 ``[T]``.  ``formed[first] += 1`` for the episodes that are not ``left_open``; ``broken[last +
   1] += 1`` for those that are not ``right_open`` (the index is ``<= T - 1`` by clause 8); ``active[t]`` is the
   number of episodes with ``first <= t <= last``.
10. Lifetimes.  ``lifetime_count`` int64 ``[2, L]``: row 0 the complete episodes, row 1 the open ones (either
    side), at index ``lifetime - 1``; ``lifetime_above [2]`` those with a lifetime ``> L``; ``L = max_lifetime``,
    default ``T``.  ``count.sum() + above.sum() == n_episodes``.
11. Pairs.  Episodes lie in ``(a, b, first)`` order.  Every pair with at least one episode has a row:
    ``pair_a, pair_b, pair_episodes, pair_frames`` (the sum of its lifetimes), ``pair_first, pair_last``;
    ``n_pairs`` counts the rows.  ``pair_frames`` is what ``min_frames`` of ``cluster_tracks`` is compared with.
12. A refused table.  A ``frame_offset`` that does not rise within ``[0, N]`` or a ``particle[i] >= P``:
    ``status = _abi.CON_BAD_TABLE``; counts, series and histogram 0, every column and ``first_seen`` /
    ``last_seen`` -1, the doubles NaN; ``ValueError`` for ndarrays.
13. Capacity.  Every per-entry, per-episode and per-pair buffer has ``max_entries`` rows.  ``n_entries >
    max_entries`` gives ``status = _abi.CON_OVERFLOW`` with ``n_entries`` as counted, so that a caller can call
    again; everything else as in clause 12.

So ``sum(lifetime) == active.sum()``; ``formed.sum()`` is the number of episodes that are not ``left_open``
and ``broken.sum()`` of those not ``right_open``; ``n_entries`` of ``'all'`` is that of ``'same'`` plus that of
``'other'``; and the number of episodes does not rise with ``gap``.

There is no CPU fallback: without the library or a GPU the calls raise ``EngineError``; argument
errors are raised before that.
"""
import collections
import math

import numpy as np

from . import _abi, _tables, static

Contacts = collections.namedtuple('Contacts', [
    'n_entries', 'duplicates', 'n_episodes', 'n_pairs', 'status',
    'a', 'b', 'first', 'last', 'lifetime', 'n_seen', 'left_open', 'right_open', 'min_d2', 'max_d2',
    'pair_a', 'pair_b', 'pair_episodes', 'pair_frames', 'pair_first', 'pair_last',
    'first_seen', 'last_seen', 'formed', 'broken', 'active', 'lifetime_count', 'lifetime_above'])

_REFUSED = "contacts_arrays: frame_offset must rise within [0, N] and particle must be below n_particles"


def _thresholds(r_on, r_off, gap):
    """clause 2: ``(on2, off2, gap)``"""
    r_on = _tables.positive(r_on, 'r_on')
    r_off = r_on if r_off is None else _tables.positive(r_off, 'r_off')
    if r_off < r_on:
        raise ValueError("r_off must be at least r_on (%r), not %r" % (r_on, r_off))
    on2, off2 = r_on * r_on, r_off * r_off
    if not (on2 > 0 and math.isfinite(off2)):
        raise ValueError("r_on and r_off must have finite positive squares")
    if isinstance(gap, bool) or not isinstance(gap, (int, float, np.integer, np.floating)) or not math.isfinite(gap):
        raise ValueError("gap must be an integer >= 0, not %r" % (gap,))
    return on2, off2, _tables.integer(gap, 0, 'gap')


def _max_lifetime(max_lifetime, n_frames):
    """clause 10: L; the default is T, within ``[1, _abi.CON_MAX_LIFETIME]``"""
    if max_lifetime is None:
        return min(max(n_frames, 1), _abi.CON_MAX_LIFETIME)
    if isinstance(max_lifetime, bool) or not isinstance(max_lifetime, (int, np.integer)) \
            or not 1 <= max_lifetime <= _abi.CON_MAX_LIFETIME:
        raise ValueError("max_lifetime must be an integer within [1, 2^20], not %r" % (max_lifetime,))
    return int(max_lifetime)


def _max_entries(max_entries):
    if max_entries is None:
        return None
    if isinstance(max_entries, bool) or not isinstance(max_entries, (int, np.integer)) or max_entries < 0:
        raise ValueError("max_entries must be an integer >= 0, not %r" % (max_entries,))
    if max_entries > 2 ** 40:
        raise ValueError("max_entries must be at most 2^40")
    return int(max_entries)


def descriptor(phase, ndim, pairs, n_frames, n_features, n_particles, on2, off2, gap, scale, max_lifetime=1, max_entries=0):
    """An ``_abi.Contacts`` with its scalars (no pointers)."""
    d = _abi.Contacts()
    d.phase, d.ndim, d.pairs = phase, ndim, _abi.PCF_PAIRS_CODES[pairs]
    d.n_frames, d.n_features, d.n_particles, d.gap = n_frames, n_features, n_particles, gap
    d.max_lifetime, d.max_entries = max_lifetime, max_entries
    d.on2, d.off2 = on2, off2
    for a, s in enumerate(scale):
        d.mpp[a] = float(s)
    return d


def contacts_arrays(pos, frame_offset, particle, r_on, r_off=None, gap=0, mpp=1., group=None, pairs='all', max_lifetime=None,
                    n_particles=None, max_entries=None, device=0, _mark=None):
    """The contact episodes of a linked table, the bonds they add up to, and the series and the histogram
    of their lifetimes (``ctr_contacts_device``; the module's rule).

    pos float64 ``[N, ndim]``, ndim 2 or 3, rows sorted by frame; frame_offset int64 ``[T + 1]``; particle
    int64 ``[N]``, dense ids ``0 .. P - 1``, negative = unlinked: what ``find_link_arrays``, ``link_arrays`` and
    ``subtract_drift_arrays`` produce, as ndarrays or as tensors on ``cuda:device``.  r_on, r_off: a contact
    switches on below ``r_on`` and off at ``r_off >= r_on`` (default ``r_on``), in the units of ``pos * mpp``.
    gap: frames without the pair that a contact survives, whether one of the two was missing or they
    were ``r_off`` or more apart.  mpp: microns per pixel, a number or one per axis.  group: int64 ``[N]``,
    e.g. the cluster labels; pairs: ``'all'``, ``'same'`` (both rows of one group ``>= 0``) or ``'other'``.
    max_lifetime: L, the length of the histogram, within ``[1, 2^20]``; default T.  n_particles: P; default
    ``particle.max() + 1``, which for a tensor is one host read.  max_entries: the rows of every per-entry,
    per-episode and per-pair buffer.  Default None: after the count pass the host reads the one word
    ``n_entries`` and allocates exactly -- one synchronisation.  With ``max_entries`` and ``n_particles`` given and
    tensors in, nothing is read back and nothing waits; more entries than that is
    ``status == _abi.CON_OVERFLOW`` with ``n_entries`` as counted and every other output at its default.  A
    call allocates about 224 bytes per entry (``include/ctrefine.h`` has the account).

    Returns ``Contacts(n_entries, duplicates, n_episodes, n_pairs, status; a, b, first, last, lifetime, n_seen,
    left_open, right_open, min_d2, max_d2 per episode; pair_a, pair_b, pair_episodes, pair_frames, pair_first,
    pair_last per pair; first_seen, last_seen [P]; formed, broken, active [T]; lifetime_count [2, L],
    lifetime_above [2])``.  For ndarrays: ints, and ndarrays trimmed to ``n_episodes`` / ``n_pairs`` (``left_open``
    and ``right_open`` as bool); a refused table raises ``ValueError``.  For a tensor ``pos``: tensors of capacity
    length, -1 / NaN beyond the counts (``left_open`` / ``right_open`` int32), the counts int64 ``[1]`` and
    ``status`` int32 ``[1]``.  Between the two phases torch sorts the keys stably; the same bytes on every
    call.  _mark: for ``tools/contacts_time.py``, called with ``'entries'``, ``'sort'`` and ``'episodes'`` after each
    is queued."""
    pos, n, ndim = _tables.positions(pos)
    on2, off2, gap = _thresholds(r_on, r_off, gap)
    scale = static._scales(mpp, ndim)
    static._pairs(pairs, group)
    frame_offset, n_frames = _tables.offsets(frame_offset)
    particle, n_particles = _tables.particles(_tables.int64_column(particle, n, 'particle'), n, n_particles)
    if group is not None:
        group = _tables.int64_column(group, n, 'group')
    if n_frames > 2 ** 31 - 3 or n > 2 ** 31 - 1:
        raise ValueError("too many frames or features for one call")
    n_life = _max_lifetime(max_lifetime, n_frames)
    max_entries = _max_entries(max_entries)
    as_tensor = _tables.is_tensor(pos)
    with _tables.stage(device) as (eng, dev):
        import torch
        pos_t = _tables.on_device(pos, dev, torch.float64, 'pos')
        off_t = _tables.on_device(frame_offset, dev, torch.int64, 'frame_offset')
        par_t = _tables.on_device(particle, dev, torch.int64, 'particle')
        group_t = None if group is None else _tables.on_device(group, dev, torch.int64, 'group')
        if n_particles is None:
            n_particles = _tables.count_particles(par_t, n)
        i64 = dict(dtype=torch.int64, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        entry_start = torch.empty(n + 1, **i64)
        words = torch.zeros(4, **i64)                    # n_entries, duplicates, n_episodes, n_pairs
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        first_seen, last_seen = torch.empty(n_particles, **i64), torch.empty(n_particles, **i64)
        d = descriptor(_abi.CON_COUNT, ndim, pairs, n_frames, n, n_particles, on2, off2, gap, scale, n_life)
        d.pos, d.frame_offset = pos_t.data_ptr() or None, off_t.data_ptr()
        d.particle = par_t.data_ptr() or None
        d.group = None if group_t is None else (group_t.data_ptr() or None)
        d.entry_start, d.n_entries, d.status = entry_start.data_ptr(), words.data_ptr(), status.data_ptr()
        d.first_seen, d.last_seen = first_seen.data_ptr() or None, last_seen.data_ptr() or None
        eng.on_current_stream(eng.contacts_device, d, dev=dev)
        if max_entries is None:
            max_entries = int(words[0].item())           # the one synchronisation of the default path
        key, frame = torch.empty(max_entries, **i64), torch.empty(max_entries, dtype=torch.int32, device=dev)
        d2 = torch.empty(max_entries, **f64)
        d.phase, d.max_entries = _abi.CON_FILL, max_entries
        d.key, d.frame, d.d2 = key.data_ptr() or None, frame.data_ptr() or None, d2.data_ptr() or None
        eng.on_current_stream(eng.contacts_device, d, dev=dev)
        mark = _mark or (lambda name: None)
        mark('entries')
        key, order = torch.sort(key, stable=True)        # plumbing: the entries of a pair side by side, in frame order
        frame, d2 = frame[order], d2[order]
        mark('sort')
        episode = [torch.empty(max_entries, **i64) for _ in range(6)]
        flags = [torch.empty(max_entries, dtype=torch.int32, device=dev) for _ in range(2)]
        reach = [torch.empty(max_entries, **f64) for _ in range(2)]
        pair = [torch.empty(max_entries, **i64) for _ in range(6)]
        series = [torch.empty(n_frames, **i64) for _ in range(3)]
        count, above = torch.empty((2, n_life), **i64), torch.empty(2, **i64)
        d.phase = _abi.CON_EPISODES
        d.key, d.frame, d.d2 = key.data_ptr() or None, frame.data_ptr() or None, d2.data_ptr() or None
        d.a, d.b, d.first, d.last, d.lifetime, d.n_seen = (x.data_ptr() or None for x in episode)
        d.left_open, d.right_open = (x.data_ptr() or None for x in flags)
        d.min_d2, d.max_d2 = (x.data_ptr() or None for x in reach)
        d.pair_a, d.pair_b, d.pair_episodes, d.pair_frames, d.pair_first, d.pair_last = (x.data_ptr() or None for x in pair)
        d.formed, d.broken, d.active = (x.data_ptr() or None for x in series)
        d.lifetime_count, d.lifetime_above = count.data_ptr(), above.data_ptr()
        d.duplicates, d.n_episodes, d.n_pairs = words[1:].data_ptr(), words[2:].data_ptr(), words[3:].data_ptr()
        eng.on_current_stream(eng.contacts_device, d, dev=dev)
        mark('episodes')
        if as_tensor:
            return Contacts(words[0:1], words[1:2], words[2:3], words[3:4], status, *episode, *flags, *reach, *pair,
                            first_seen, last_seen, *series, count, above)
        code = int(status.item())
        if code == _abi.CON_BAD_TABLE:
            raise ValueError(_REFUSED)
        n_entries, duplicates, n_episodes, n_pairs = (int(v) for v in words.cpu())
        host = lambda x, m: x[:m].cpu().numpy()
        return Contacts(n_entries, duplicates, n_episodes, n_pairs, code,
                        *(host(x, n_episodes) for x in episode), *(host(x, n_episodes).astype(bool) for x in flags),
                        *(host(x, n_episodes) for x in reach), *(host(x, n_pairs) for x in pair),
                        first_seen.cpu().numpy(), last_seen.cpu().numpy(), *(x.cpu().numpy() for x in series),
                        count.cpu().numpy(), above.cpu().numpy())


def _of_table(f, r_on, r_off, gap, mpp, group_column, pairs, pos_columns, t_column, max_lifetime, device):
    """the argument checks that need no table, then the table and its call: ``(res, ids, first_frame)``"""
    _thresholds(r_on, r_off, gap)
    static._pairs(pairs, group_column, 'group_column')
    _max_lifetime(max_lifetime, 1)
    ndim = len(pos_columns) if pos_columns is not None else (3 if 'z' in f else 2)
    if ndim in (2, 3):
        static._scales(mpp, ndim)
    _, offset, first, ids, dense, _, pos, *group = _tables.frame_sorted(
        f, pos_columns, t_column, () if group_column is None else (group_column,))
    res = contacts_arrays(pos, offset, dense, r_on, r_off, gap, mpp, group[0] if group else None, pairs, max_lifetime,
                          n_particles=len(ids), device=device)
    return res, ids, first


def _counts(res):
    return {'n_entries': res.n_entries, 'duplicates': res.duplicates, 'n_episodes': res.n_episodes, 'n_pairs': res.n_pairs}


def contacts(f, r_on, r_off=None, gap=0, mpp=1., group_column=None, pairs='all', pos_columns=None, t_column='frame', device=0):
    """The contact episodes of a linked table: a DataFrame with one row per episode, in ``(particle_a,
    particle_b, first_frame)`` order, with the columns ``particle_a < particle_b`` (the table's own ids),
    ``first_frame``, ``last_frame`` (the table's own frame numbers), ``lifetime`` (frames, both ends counted),
    ``n_seen`` (the frames of it in which the pair was seen within ``r_off``), ``left_open`` / ``right_open`` (it
    began within ``gap`` frames of the first, or ended within ``gap`` frames of the last, frame of one of the
    two particles: its lifetime is a lower bound) and ``min_dist`` / ``max_dist``, the smallest and largest
    distance seen.  ``attrs`` carries ``n_entries``, ``duplicates``, ``n_episodes`` and ``n_pairs``.

    f: a DataFrame with the position columns (default ``['y', 'x']``, with ``'z'`` in front where the table
    has one), ``t_column`` and ``'particle'``; the frames are taken dense from the first to the last.
    group_column: an integer column such as ``'cluster'`` for ``pairs='same'`` / ``'other'``.  The other
    arguments as for :func:`contacts_arrays`, which also returns the series and the histogram."""
    import pandas as pd
    res, ids, first = _of_table(f, r_on, r_off, gap, mpp, group_column, pairs, pos_columns, t_column, None, device)
    out = pd.DataFrame(collections.OrderedDict([
        ('particle_a', ids[res.a]), ('particle_b', ids[res.b]), ('first_frame', res.first + first),
        ('last_frame', res.last + first), ('lifetime', res.lifetime), ('n_seen', res.n_seen), ('left_open', res.left_open),
        ('right_open', res.right_open), ('min_dist', np.sqrt(res.min_d2)), ('max_dist', np.sqrt(res.max_d2))]))
    out.attrs.update(_counts(res))
    return out


def bonds(f, r_on, r_off=None, gap=0, mpp=1., group_column=None, pairs='all', pos_columns=None, t_column='frame',
          min_frames=1, device=0):
    """The pairs of a linked table that were in contact for at least ``min_frames`` frames in all: a
    DataFrame with the columns ``particle_a``, ``particle_b``, ``episodes``, ``frames`` (the sum of the lifetimes of
    the pair's episodes: what ``min_frames`` of ``cluster_tracks`` is compared with), ``first_frame`` and
    ``last_frame``; ``attrs`` as for :func:`contacts`, whose arguments the others are."""
    import pandas as pd
    min_frames = _tables.integer(min_frames, 1, 'min_frames')
    res, ids, first = _of_table(f, r_on, r_off, gap, mpp, group_column, pairs, pos_columns, t_column, None, device)
    keep = res.pair_frames >= min_frames
    out = pd.DataFrame(collections.OrderedDict([
        ('particle_a', ids[res.pair_a[keep]]), ('particle_b', ids[res.pair_b[keep]]), ('episodes', res.pair_episodes[keep]),
        ('frames', res.pair_frames[keep]), ('first_frame', res.pair_first[keep] + first),
        ('last_frame', res.pair_last[keep] + first)]))
    out.attrs.update(_counts(res))
    return out


def contact_lifetimes(f, r_on, r_off=None, gap=0, mpp=1., group_column=None, pairs='all', pos_columns=None, t_column='frame',
                      max_lifetime=None, device=0):
    """The histogram of the lifetimes of a linked table's contact episodes: a DataFrame indexed by
    ``lifetime`` (1 .. ``max_lifetime``, default the number of frames) with the columns ``complete`` (episodes
    seen from their beginning to their end) and ``open`` (censored on either side: a lower bound).  ``attrs``
    carries ``above_complete`` and ``above_open``, the episodes longer than ``max_lifetime``, besides those of
    :func:`contacts`, whose arguments the others are."""
    import pandas as pd
    res, _, _ = _of_table(f, r_on, r_off, gap, mpp, group_column, pairs, pos_columns, t_column, max_lifetime, device)
    index = pd.Index(np.arange(1, res.lifetime_count.shape[1] + 1, dtype=np.int64), name='lifetime')
    out = pd.DataFrame({'complete': res.lifetime_count[0], 'open': res.lifetime_count[1]}, index=index, columns=['complete', 'open'])
    out.attrs.update(_counts(res))
    out.attrs.update(above_complete=int(res.lifetime_above[0]), above_open=int(res.lifetime_above[1]))
    return out
