// pair_walk.h -- what the pair stages share (g(r): pair_corr_kernels.h; nearest neighbours:
// neighbors_kernels.h): the table of a call, the check of its frame_offset, the work
// items (a frame's tiles of PAIR_TILE rows), the scaled position of a row, and the walk of a thread
// over a range of candidate rows -- one d2, one limit, one group filter for every stage.  Included
// inside the anonymous namespace of a unit after stage_common.h.  Every product and sum of d2 is a
// statement of its own, and the units are compiled with fp contract(off): nothing here may be fused.
// A stage supplies what a candidate row is (its position and whether it exists), what happens to a
// pair, and what happens after a tile.
#ifndef CTREFINE_PAIR_WALK_H
#define CTREFINE_PAIR_WALK_H

constexpr int PAIR_THREADS = 256;                // a workgroup of every kernel of a pair stage: 4 wavefronts
constexpr int PAIR_TILE = PAIR_THREADS;          // rows of a frame that a work item owns, and that it stages at a time

static_assert(CTR_PCF_OK == 0 && CTR_NBR_OK == 0, "status[0] == 0: the table of a pair stage was not refused");

struct PairTable {
  int ndim, pairs;
  long long T, N;
  double mpp[CTR_MAX_NDIM];
  const double* pos;
  const long long* frame_offset;
  const long long* group;
  long long* item_start;      // scratch [T + 1]: the first work item of a frame; [T]: their number
  int* status;
};

// a tile of candidate rows in LDS: 8192 B
struct PairTile {
  double q[CTR_MAX_NDIM][PAIR_TILE];
  long long grp[PAIR_TILE];
};

__device__ __forceinline__ bool pair_ok(const PairTable& p) { return ld_agent(p.status) == 0; }

// The body of a stage's check kernel: the caller's frame_offset, before any kernel follows it.
// status[0] was zeroed in front of the kernel.
__device__ __forceinline__ void pair_check(const PairTable& p, int bad_table) {
  const long long stride = (long long)gridDim.x * PAIR_THREADS;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * PAIR_THREADS + threadIdx.x; i <= p.T; i += stride)
    bad |= offsets_bad(p.frame_offset, i, p.T, p.N);
  if (bad) st_agent(p.status, bad_table);
}

// The body of a stage's items kernel, one workgroup: item_start, the exclusive scan of the frames'
// tiles of PAIR_TILE rows.  A refused table has no work item.
__device__ __forceinline__ void pair_items(const PairTable& p) {
  const bool ok = pair_ok(p);
  const long long total = workgroup_scan_n<PAIR_THREADS, long long>(
      p.T,
      [&](long long t) { return ok ? (p.frame_offset[t + 1] - p.frame_offset[t] + PAIR_TILE - 1) / PAIR_TILE : 0LL; },
      [&](long long t, long long before) { p.item_start[t] = before; });
  if (threadIdx.x == 0) p.item_start[p.T] = total;
}

// the frame of work item w < item_start[T]: the last t with item_start[t] <= w; its tile is w - item_start[t]
__device__ __forceinline__ long long pair_item_frame(const PairTable& p, long long w) {
  long long lo = 0, hi = p.T;
  while (hi - lo > 1) {
    const long long mid = (lo + hi) / 2;
    if (p.item_start[mid] <= w) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the scaled position of row r (q = pos * mpp per axis, one rounding) and whether it exists: finite on
// every axis, where within(d, q) holds too (a stage with a box)
struct PairRow {
  double q[CTR_MAX_NDIM];
  bool exists;
};

template <typename Within>
__device__ __forceinline__ PairRow pair_row(const PairTable& p, long long r, Within within) {
  PairRow o;
  o.exists = true;
#pragma unroll
  for (int d = 0; d < CTR_MAX_NDIM; ++d) {
    o.q[d] = 0.;
    if (d < p.ndim) {
      const double q = p.pos[r * p.ndim + d] * p.mpp[d];
      o.q[d] = q;
      o.exists = o.exists && fabs(q) < __builtin_inf() && within(d, q);      // false for a NaN
    }
  }
  return o;
}

__device__ __forceinline__ PairRow pair_row(const PairTable& p, long long r) {
  return pair_row(p, r, [](int, double) { return true; });
}

// Every thread of the workgroup calls it for the candidate rows [c0, c1), the same for all of them.
// The rows are staged a tile at a time in LDS with their group ids; row(j) gives a candidate's .q and
// .exists, and a row that does not exist is staged as NaN: its d2 fails d2 < limit2.  A thread that
// is `active` has the scaled position `me`, the group id gi (-1 without groups) and skips row `self`
// (-1: none); it walks the tile -- every lane reads the same LDS address, a broadcast -- and calls
// pair(j, d2) for every candidate, in ascending j, that passes the limit and the same/other filter.
// tile() is called by every thread after each tile; it may hold a barrier.  The first thing a tile
// does is a barrier, so a walk may follow another, but the caller puts one between the last tile
// and its own use of `s`.
template <typename Row, typename Pair, typename Tile>
__device__ __forceinline__ void pair_walk(const PairTable& p, PairTile& s, long long c0, long long c1, bool active,
                                          const double* me, long long gi, long long self, double limit2, Row row, Pair pair,
                                          Tile tile) {
  const int tid = threadIdx.x, nd = p.ndim;
  const double nan = __builtin_nan("");
  for (long long tb = c0; tb < c1; tb += PAIR_TILE) {
    __syncthreads();                     // the tile before is read
    const long long j = tb + tid;
    if (j < c1) {
      const auto r = row(j);
#pragma unroll
      for (int d = 0; d < CTR_MAX_NDIM; ++d)
        if (d < nd) s.q[d][tid] = r.exists ? r.q[d] : nan;
      s.grp[tid] = p.group ? p.group[j] : -1;
    }
    __syncthreads();
    const int n = c1 - tb < PAIR_TILE ? (int)(c1 - tb) : PAIR_TILE;
    if (active)
      for (int jj = 0; jj < n; ++jj) {
        if (tb + jj == self) continue;
        double d2 = 0.;
#pragma unroll
        for (int d = 0; d < CTR_MAX_NDIM; ++d)
          if (d < nd) {
            const double x = s.q[d][jj] - me[d];
            const double x2 = x * x;              // the unit is compiled without contraction
            d2 = d == 0 ? x2 : d2 + x2;
          }
        if (!(d2 < limit2)) continue;             // too far, or a row that does not exist
        if (p.pairs != CTR_PCF_PAIRS_ALL) {
          const bool same = gi >= 0 && s.grp[jj] == gi;
          if (same != (p.pairs == CTR_PCF_PAIRS_SAME)) continue;
        }
        pair(tb + jj, d2);
      }
    tile();
  }
}

// ---- host -----------------------------------------------------------------------------------
// the scalars of a descriptor that both stages have; a static message, or null
template <typename Desc>
const char* pair_scalars(const Desc* c, const char* too_many) {
  if (c->ndim != 2 && c->ndim != 3) return "ndim must be 2 or 3";
  if (c->pairs != CTR_PCF_PAIRS_ALL && c->pairs != CTR_PCF_PAIRS_SAME && c->pairs != CTR_PCF_PAIRS_OTHER)
    return "pairs must be CTR_PCF_PAIRS_ALL, _SAME or _OTHER";
  if (c->n_frames < 0 || c->n_features < 0) return "negative counts";
  if (c->n_frames > 0x7ffffffdLL || c->n_features > 0x7fffffffLL) return too_many;
  for (int d = 0; d < c->ndim; ++d)
    if (!std::isfinite(c->mpp[d]) || !(c->mpp[d] > 0.)) return "mpp must be finite and positive";
  return nullptr;
}

// the columns that the rows need; a static message, or null
template <typename Desc>
const char* pair_columns(const Desc* c) {
  if (c->n_features > 0 && !c->pos) return "features without pos";
  if (c->n_features > 0 && c->pairs != CTR_PCF_PAIRS_ALL && !c->group) return "pairs by group without group";
  return nullptr;
}

// A frame of n rows has ceil(n / PAIR_TILE) work items: at most T + N / PAIR_TILE in all, whatever the
// offsets.  Returns that bound; o_start: where item_start is carved from the scratch laid out up to `at`.
template <typename Desc>
long long pair_max_items(const Desc* c, size_t& at, size_t& o_start) {
  o_start = carve(at, sizeof(long long) * (size_t)(c->n_frames + 1));
  return c->n_frames + c->n_features / PAIR_TILE;
}

// the table of a launch
template <typename Desc>
PairTable pair_table(const Desc* c, void* scratch, size_t o_start) {
  PairTable p = {};
  p.ndim = c->ndim; p.pairs = c->pairs;
  p.T = c->n_frames; p.N = c->n_features;
  for (int d = 0; d < c->ndim; ++d) p.mpp[d] = c->mpp[d];
  p.pos = c->pos;
  p.frame_offset = (const long long*)c->frame_offset;
  p.group = (const long long*)c->group;
  p.item_start = (long long*)((char*)scratch + o_start);
  p.status = c->status;
  return p;
}

#endif  // CTREFINE_PAIR_WALK_H
