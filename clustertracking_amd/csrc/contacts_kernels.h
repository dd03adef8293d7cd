// contacts_kernels.h -- contact episodes and bond lifetimes of linked particles: how long two
// particles stay together (ctr_contacts_device; include/ctrefine.h has the rule).
// Included by tu_contacts.hip inside its anonymous namespace, after stage_common.h and pair_walk.h,
// which has the table, the work items and the walk over a frame's rows.  Three phases with the
// caller's stable sort between the last two: COUNT (the entries of every row, their scan), FILL (the
// same walk writes them where the scan says) and EPISODES (chains, episodes, pairs, series and
// histogram of the sorted entries).  The kernel boundary is the only synchronisation between
// workgroups; every loop is bounded by the launch's arguments, by row ranges of a frame_offset that
// cont_check_kernel has passed, or by counts that an earlier kernel of the call wrote.  An entry, a
// chain, an episode and a pair row each have one owner; the only atomics are 64-bit integer minima,
// maxima and additions, where the order cannot matter, and there is no sum of doubles at all.
#ifndef CTREFINE_CONTACTS_KERNELS_H
#define CTREFINE_CONTACTS_KERNELS_H

constexpr int CONT_THREADS = PAIR_THREADS;       // a workgroup of every kernel here: 4 wavefronts
constexpr int CONT_TILE = PAIR_TILE;             // rows of a frame that a work item owns
constexpr int CONT_WAVES = CONT_THREADS / 64;    // chains, or pairs, of a workgroup at a time
constexpr long long CONT_NO_KEY = 0x7fffffffffffffffLL;   // above every key: a slot without an entry sorts last
constexpr long long CONT_NONE = 0x7fffffffffffffffLL;     // no on-entry among a lane's entries

static_assert(CTR_CON_OK == 0, "status[0] == 0: the table of a pair stage was not refused");

// which scan the three scan kernels run
enum { CONT_SCAN_ROWS = 0, CONT_SCAN_HEADS = 1, CONT_SCAN_CHAINS = 2, CONT_SCAN_PAIRS = 3 };

struct ContArgs {
  PairTable tab;
  long long P, gap, L, M;
  double on2, off2;
  const long long* particle;
  // the entries: unsorted out of FILL, sorted into EPISODES
  long long* entry_start;     // [N + 1] the entries of a row, then the first entry of a row
  long long* key;             // [M]
  int* frame;                 // [M]
  double* d2;                 // [M]
  long long* n_entries;       // [1]
  long long* first_seen;      // [P]
  long long* last_seen;       // [P]
  // scratch
  long long* sums;            // a word per scan tile
  long long* chain_start;     // [M] the first entry of a chain
  long long* c_on;            // [M] the first on-entry of a chain, or -1
  long long* c_seen;          // [M] the entries that count from there on
  double* c_min;              // [M] ... and their smallest and largest d2
  double* c_max;
  long long* ep_chain;        // [M] the chain of an episode
  long long* pair_start;      // [M] the first episode of a pair
  long long* diff;            // [T + 1] the episodes that begin at t less those that ended at t - 1
  long long* n_chains;        // [1]
  // out
  long long *ep_a, *ep_b, *ep_first, *ep_last, *ep_lifetime, *ep_seen;
  int *ep_left, *ep_right;
  double *ep_min, *ep_max;
  long long *pair_a, *pair_b, *pair_episodes, *pair_frames, *pair_first, *pair_last;
  long long *formed, *broken, *active, *lifetime_count, *lifetime_above;
  long long *duplicates, *n_episodes, *n_pairs;
};

__device__ __forceinline__ void cont_add(long long* p, long long v) {
  atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

// the entries that the later kernels may follow: those of a call that was not refused and did not overflow
__device__ __forceinline__ long long cont_entries(const ContArgs& a) {
  if (!pair_ok(a.tab)) return 0;
  const long long n = a.n_entries[0];
  return n < 0 ? 0 : n > a.M ? a.M : n;
}

// ---- COUNT and FILL ---------------------------------------------------------------------------
__global__ void __launch_bounds__(CONT_THREADS) cont_check_kernel(const ContArgs a) {
  pair_check(a.tab, CTR_CON_BAD_TABLE);
  const long long stride = (long long)gridDim.x * CONT_THREADS;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * CONT_THREADS + threadIdx.x; i < a.tab.N; i += stride) bad |= a.particle[i] >= a.P;
  if (bad) st_agent(a.tab.status, CTR_CON_BAD_TABLE);
}

// COUNT: no row has an entry and no particle has been seen, whatever the status
__global__ void __launch_bounds__(CONT_THREADS) cont_count_defaults_kernel(const ContArgs a) {
  const long long stride = (long long)gridDim.x * CONT_THREADS;
  for (long long i = (long long)blockIdx.x * CONT_THREADS + threadIdx.x; i <= a.tab.N || i < a.P; i += stride) {
    if (i <= a.tab.N) a.entry_start[i] = 0;
    if (i < a.P) { a.first_seen[i] = a.tab.T; a.last_seen[i] = -1; }
  }
}

__global__ void __launch_bounds__(CONT_THREADS) cont_items_kernel(const ContArgs a) { pair_items(a.tab); }

// One workgroup per work item w (striding past the grid), as the neighbours' kernel: a thread owns row
// i of frame t and walks the frame's rows (pair_walk: a candidate exists when it is finite and
// linked), in ascending j; an entry is a candidate within off2 of a larger particle.  COUNT counts
// them into entry_start[i] and notes the frame in first_seen / last_seen of the row's particle; FILL
// repeats the walk and writes key, frame and d2 from entry_start[i] on: the place of an entry is
// decided by the scan, not by an atomic append.
template <bool FILL>
__device__ __forceinline__ void cont_walk(const ContArgs& a, PairTile& s_tile) {
  if (!pair_ok(a.tab)) return;
  const long long total = a.tab.item_start[a.tab.T];
  if ((long long)blockIdx.x >= total) return;
  const int tid = threadIdx.x;
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long t = pair_item_frame(a.tab, w), r0 = a.tab.frame_offset[t], r1 = a.tab.frame_offset[t + 1];
    const long long i = r0 + (w - a.tab.item_start[t]) * CONT_TILE + tid;
    PairRow me = {};
    long long gi = -1, pi = -1;
    if (i < r1) {
      me = pair_row(a.tab, i);
      pi = a.particle[i];                    // below P (cont_check_kernel)
      me.exists = me.exists && pi >= 0;
      if (a.tab.group) gi = a.tab.group[i];
    }
    if (!FILL && me.exists) {
      __hip_atomic_fetch_min(a.first_seen + pi, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(a.last_seen + pi, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    long long at = FILL && i < r1 ? a.entry_start[i] : 0;
    const long long key0 = pi * a.P;         // below 2^62
    pair_walk(
        a.tab, s_tile, r0, r1, me.exists, me.q, gi, i, a.off2,
        [&](long long j) {
          PairRow r = pair_row(a.tab, j);
          r.exists = r.exists && a.particle[j] >= 0;
          return r;
        },
        [&](long long j, double d2) {
          const long long pj = a.particle[j];
          if (pj <= pi) return;
          if (FILL && at < a.M) {
            a.key[at] = key0 + pj;
            a.frame[at] = (int)t;            // T < 2^31
            a.d2[at] = d2;
          }
          ++at;
        },
        []() {});
    if (!FILL && i < r1) a.entry_start[i] = at;
  }
}

__global__ void __launch_bounds__(CONT_THREADS) cont_count_kernel(const ContArgs a) {
  __shared__ PairTile s_tile;
  cont_walk<false>(a, s_tile);
}

__global__ void __launch_bounds__(CONT_THREADS) cont_fill_kernel(const ContArgs a) {
  __shared__ PairTile s_tile;
  cont_walk<true>(a, s_tile);
}

// FILL: more entries than the caller has room for is CTR_CON_OVERFLOW; every slot without an entry
// gets the key that sorts last; a call that was refused or overflowed has seen no particle
__global__ void __launch_bounds__(CONT_THREADS) cont_fill_defaults_kernel(const ContArgs a) {
  const long long n = a.n_entries[0];
  const bool over = n > a.M, ok = pair_ok(a.tab) && !over;
  const long long kept = ok ? n : 0, stride = (long long)gridDim.x * CONT_THREADS;
  const long long first = (long long)blockIdx.x * CONT_THREADS + threadIdx.x;
  if (over && first == 0 && pair_ok(a.tab)) st_agent(a.tab.status, CTR_CON_OVERFLOW);
  for (long long e = first; e < a.M || e < a.P; e += stride) {
    if (e >= kept && e < a.M) { a.key[e] = CONT_NO_KEY; a.frame[e] = -1; a.d2[e] = __builtin_nan(""); }
    if (!ok && e < a.P) { a.first_seen[e] = -1; a.last_seen[e] = -1; }
  }
}

// ---- EPISODES ---------------------------------------------------------------------------------
// every output at its default, whatever the status: a refused or overflowed call leaves them so
__global__ void __launch_bounds__(CONT_THREADS) cont_episode_defaults_kernel(const ContArgs a) {
  const double nan = __builtin_nan("");
  const long long stride = (long long)gridDim.x * CONT_THREADS, T = a.tab.T;
  for (long long e = (long long)blockIdx.x * CONT_THREADS + threadIdx.x; e < a.M || e <= T || e < 2 * a.L; e += stride) {
    if (e < a.M) {
      a.ep_a[e] = -1; a.ep_b[e] = -1; a.ep_first[e] = -1; a.ep_last[e] = -1; a.ep_lifetime[e] = -1; a.ep_seen[e] = -1;
      a.ep_left[e] = -1; a.ep_right[e] = -1; a.ep_min[e] = nan; a.ep_max[e] = nan;
      a.pair_a[e] = -1; a.pair_b[e] = -1; a.pair_episodes[e] = -1; a.pair_frames[e] = -1; a.pair_first[e] = -1; a.pair_last[e] = -1;
    }
    if (e <= T) a.diff[e] = 0;
    if (e < T) { a.formed[e] = 0; a.broken[e] = 0; a.active[e] = 0; }
    if (e < 2 * a.L) a.lifetime_count[e] = 0;
    if (e < 2) a.lifetime_above[e] = 0;
    if (e == 0) { a.duplicates[0] = 0; a.n_episodes[0] = 0; a.n_pairs[0] = 0; a.n_chains[0] = 0; }
  }
}

// clause 5: entry e of the sorted entries repeats the pair and frame of the entry before it
__device__ __forceinline__ bool cont_duplicate(const ContArgs& a, long long e) {
  return e > 0 && a.key[e] == a.key[e - 1] && a.frame[e] == a.frame[e - 1];
}

// clause 6: entry e heads a chain: the first of its pair, or more than gap + 1 frames after the entry before it
__device__ __forceinline__ bool cont_head(const ContArgs& a, long long e) {
  if (e == 0 || a.key[e] != a.key[e - 1]) return true;
  return (long long)a.frame[e] - (long long)a.frame[e - 1] > a.gap + 1;
}

// clause 11: episode x is the first of its pair
__device__ __forceinline__ bool cont_pair_head(const ContArgs& a, long long x) {
  return x == 0 || a.ep_a[x] != a.ep_a[x - 1] || a.ep_b[x] != a.ep_b[x - 1];
}

// the three scan kernels (stage_common.h: grid_scan_*): how many values, the value of one, what its
// prefix places, and where the sum goes
__device__ __forceinline__ long long cont_scan_n(const ContArgs& a, int which) {
  if (which == CONT_SCAN_ROWS) return a.tab.N;       // zeros where the table was refused
  const long long n = cont_entries(a);
  const long long m = which == CONT_SCAN_HEADS ? n : which == CONT_SCAN_CHAINS ? a.n_chains[0] : a.n_episodes[0];
  return m < n ? m : n;                              // chains and episodes: no more than entries
}

__device__ __forceinline__ long long cont_scan_value(const ContArgs& a, int which, long long i) {
  switch (which) {
    case CONT_SCAN_ROWS: return a.entry_start[i];
    case CONT_SCAN_HEADS: return cont_head(a, i) ? 1 : 0;
    case CONT_SCAN_CHAINS: return a.c_on[i] >= 0 ? 1 : 0;
    default: return cont_pair_head(a, i) ? 1 : 0;
  }
}

__device__ __forceinline__ void cont_scan_place(const ContArgs& a, int which, long long i, long long before) {
  switch (which) {
    case CONT_SCAN_ROWS: a.entry_start[i] = before; break;
    case CONT_SCAN_HEADS: if (cont_head(a, i)) a.chain_start[before] = i; break;
    case CONT_SCAN_CHAINS: if (a.c_on[i] >= 0) a.ep_chain[before] = i; break;
    default: if (cont_pair_head(a, i)) a.pair_start[before] = i; break;
  }
}

__global__ void __launch_bounds__(CONT_THREADS) cont_scan_sums_kernel(const ContArgs a, const int which) {
  grid_scan_sums<CONT_THREADS>(cont_scan_n(a, which), a.sums, [&](long long i) { return cont_scan_value(a, which, i); });
}

__global__ void __launch_bounds__(CONT_THREADS) cont_scan_top_kernel(const ContArgs a, const int which) {
  const long long total = grid_scan_top<CONT_THREADS>(cont_scan_n(a, which), a.sums);
  if (threadIdx.x != 0) return;
  switch (which) {
    case CONT_SCAN_ROWS: a.entry_start[a.tab.N] = total; a.n_entries[0] = total; break;
    case CONT_SCAN_HEADS: a.n_chains[0] = total; break;
    case CONT_SCAN_CHAINS: a.n_episodes[0] = total; break;
    default: a.n_pairs[0] = total; break;
  }
}

__global__ void __launch_bounds__(CONT_THREADS) cont_scan_apply_kernel(const ContArgs a, const int which) {
  grid_scan_apply<CONT_THREADS>(
      cont_scan_n(a, which), a.sums, [&](long long i) { return cont_scan_value(a, which, i); },
      [&](long long i, long long before) { cont_scan_place(a, which, i, before); });
}

// reductions over the 64 lanes of a wavefront, every lane active; the result in every lane
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ long long wave_min(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const long long o = __shfl_xor(v, d); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(v, d); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(v, d); v = o > v ? o : v; }
  return v;
}

// One chain per wavefront (striding): the 64 lanes stride its entries, so a bond of 10 000 frames is
// no thread's serial walk.  First over the whole chain: its duplicates, and the first entry that is
// none and lies below on2 (clause 7); then from that entry on: the entries that count and the
// smallest and largest d2 -- minima and maxima of non-negative doubles and integer sums, whose order
// cannot matter.  Within a chain the key is one, so a duplicate is an entry with the frame of the
// entry before it.
__global__ void __launch_bounds__(CONT_THREADS) cont_chains_kernel(const ContArgs a) {
  const long long n = cont_entries(a), nc = a.n_chains[0] < n ? a.n_chains[0] : n;
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * CONT_WAVES;
  for (long long c = (long long)blockIdx.x * CONT_WAVES + (threadIdx.x >> 6); c < nc; c += waves) {
    const long long e0 = a.chain_start[c], e1 = c + 1 < nc ? a.chain_start[c + 1] : n;
    long long on = CONT_NONE, dups = 0;
    for (long long e = e0 + lane; e < e1; e += 64) {
      if (e > e0 && a.frame[e] == a.frame[e - 1]) ++dups;
      else if (a.d2[e] < a.on2 && e < on) on = e;
    }
    on = wave_min(on);
    dups = wave_sum(dups);
    if (lane == 0 && dups > 0) cont_add(a.duplicates, dups);
    if (on == CONT_NONE) {
      if (lane == 0) a.c_on[c] = -1;
      continue;
    }
    long long seen = 0;
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (long long e = on + lane; e < e1; e += 64) {
      if (e > on && a.frame[e] == a.frame[e - 1]) continue;
      const double d2 = a.d2[e];
      ++seen;
      lo = d2 < lo ? d2 : lo;
      hi = d2 > hi ? d2 : hi;
    }
    seen = wave_sum(seen);
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (lane == 0) { a.c_on[c] = on; a.c_seen[c] = seen; a.c_min[c] = lo; a.c_max[c] = hi; }
  }
}

// Every lane of a wavefront calls it: base[index] += sign for every active lane, one atomic per distinct
// index among them -- the lanes that share the first active lane's index leave with it, so 64 episodes of
// one lifetime are one addition to their bin, not 64 to one address.
__device__ __forceinline__ void cont_add_grouped(long long* base, long long index, bool active, long long sign) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const long long at = __shfl(index, leader);
    const bool mine = active && index == at;
    const unsigned long long group = __ballot(mine);
    if (lane == leader) cont_add(base + at, sign * (long long)__popcll(group));
    if (mine) active = false;
    todo &= ~group;
  }
}

// One thread per episode (striding): its row (clauses 7 and 8), and with integer atomics, grouped by
// address within a wavefront, its part of the series and of the histogram (clauses 9 and 10).
__global__ void __launch_bounds__(CONT_THREADS) cont_episodes_kernel(const ContArgs a) {
  const long long n = cont_entries(a), nc = a.n_chains[0] < n ? a.n_chains[0] : n;
  const long long ne = a.n_episodes[0] < nc ? a.n_episodes[0] : nc, T = a.tab.T;
  const long long stride = (long long)gridDim.x * CONT_THREADS;
  for (long long x0 = (long long)blockIdx.x * CONT_THREADS; x0 < ne; x0 += stride) {
    const long long x = x0 + threadIdx.x;
    long long first = 0, last = 0, lifetime = 0;
    bool left = false, right = false, counts = false;
    if (x < ne) {
      const long long c = a.ep_chain[x], e0 = a.chain_start[c], e1 = c + 1 < nc ? a.chain_start[c + 1] : n, on = a.c_on[c];
      const long long key = a.key[on], pa = key / a.P, pb = key - pa * a.P;
      first = a.frame[on];
      last = a.frame[e1 - 1];
      lifetime = last - first + 1;
      if (key >= 0 && pa < a.P) {              // the caller's sorted keys are not followed blindly
        const long long fa = a.first_seen[pa], fb = a.first_seen[pb], la = a.last_seen[pa], lb = a.last_seen[pb];
        left = on == e0 && first - (fa > fb ? fa : fb) <= a.gap;
        right = (la < lb ? la : lb) - last <= a.gap;
      }
      a.ep_a[x] = pa; a.ep_b[x] = pb; a.ep_first[x] = first; a.ep_last[x] = last; a.ep_lifetime[x] = lifetime;
      a.ep_seen[x] = a.c_seen[c]; a.ep_left[x] = left ? 1 : 0; a.ep_right[x] = right ? 1 : 0;
      a.ep_min[x] = a.c_min[c]; a.ep_max[x] = a.c_max[c];
      counts = first >= 0 && last >= first && last < T;      // ... nor their frames
    }
    const long long open = left || right ? 1 : 0;
    cont_add_grouped(a.formed, first, counts && !left, 1);
    cont_add_grouped(a.broken, last + 1, counts && !right && last + 1 < T, 1);
    cont_add_grouped(a.diff, first, counts, 1);
    cont_add_grouped(a.diff, last + 1, counts, -1);
    cont_add_grouped(a.lifetime_count, open * a.L + lifetime - 1, counts && lifetime <= a.L, 1);
    cont_add_grouped(a.lifetime_above, open, counts && lifetime > a.L, 1);
  }
}

// One pair per wavefront (striding), as the chains: the episodes of a pair lie side by side in (a, b, first) order.
__global__ void __launch_bounds__(CONT_THREADS) cont_pairs_kernel(const ContArgs a) {
  const long long n = cont_entries(a), ne = a.n_episodes[0] < n ? a.n_episodes[0] : n;
  const long long np = a.n_pairs[0] < ne ? a.n_pairs[0] : ne;
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * CONT_WAVES;
  for (long long p = (long long)blockIdx.x * CONT_WAVES + (threadIdx.x >> 6); p < np; p += waves) {
    const long long x0 = a.pair_start[p], x1 = p + 1 < np ? a.pair_start[p + 1] : ne;
    long long frames = 0;
    for (long long x = x0 + lane; x < x1; x += 64) frames += a.ep_lifetime[x];
    frames = wave_sum(frames);
    if (lane == 0) {
      a.pair_a[p] = a.ep_a[x0]; a.pair_b[p] = a.ep_b[x0]; a.pair_episodes[p] = x1 - x0; a.pair_frames[p] = frames;
      a.pair_first[p] = a.ep_first[x0]; a.pair_last[p] = a.ep_last[x1 - 1];
    }
  }
}

// One workgroup: active[t] = the running sum of diff up to t, an integer scan.
__global__ void __launch_bounds__(CONT_THREADS) cont_active_kernel(const ContArgs a) {
  if (!pair_ok(a.tab)) return;
  workgroup_scan_n<CONT_THREADS, long long>(
      a.tab.T, [&](long long t) { return a.diff[t]; }, [&](long long t, long long before) { a.active[t] = before + a.diff[t]; });
}

#endif  // CTREFINE_CONTACTS_KERNELS_H
