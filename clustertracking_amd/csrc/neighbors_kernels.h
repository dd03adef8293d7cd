// neighbors_kernels.h -- nearest neighbours and proximity of a feature table: for every row the k
// nearest rows of the frame `lag` frames on, their number within a distance and, per particle, the
// smallest nearest-neighbour distance (ctr_neighbors_device; include/ctrefine.h has the rule,
// DESIGN.md 7b).  Included by tu_neighbors.hip inside its anonymous namespace, after stage_common.h.
// The kernel boundary is the only synchronisation between workgroups; every loop is bounded by the
// launch's arguments or by row ranges of a frame_offset that nbr_check_kernel has passed.  Every
// output element has one owner thread; the only atomics are 64-bit integer minima of the
// per-particle keys, where the order cannot matter.
#ifndef CTREFINE_NEIGHBORS_KERNELS_H
#define CTREFINE_NEIGHBORS_KERNELS_H

constexpr int NBR_THREADS = 256;                 // a workgroup of every kernel here: 4 wavefronts
constexpr int NBR_TILE = NBR_THREADS;            // rows of a frame that a work item owns, and that it stages at a time
constexpr unsigned long long NBR_NO_KEY = ~0ull; // above the key of every double: a particle without a neighbour

struct NbrArgs {
  int ndim, pairs, k;
  long long lag, T, N, P;
  double limit2;
  double mpp[CTR_MAX_NDIM];
  const double* pos;
  const long long* frame_offset;
  const long long* group;
  const long long* particle;
  // scratch
  long long* item_start;          // [T + 1] the first work item of a frame; [T]: their number
  unsigned long long* pkey;       // [P] the ordered key of the smallest dist2[i, 0] of a particle
  // out
  double* dist;
  double* dist2;
  long long* index;
  long long* count;
  double* particle_min;
  double* particle_min2;
  int* status;
};

// the caller's frame_offset, before any kernel follows it.  status[0] was zeroed in front of this kernel.
__global__ void __launch_bounds__(NBR_THREADS) nbr_check_kernel(const NbrArgs a) {
  const long long stride = (long long)gridDim.x * NBR_THREADS;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * NBR_THREADS + threadIdx.x; i <= a.T; i += stride)
    bad |= offsets_bad(a.frame_offset, i, a.T, a.N);
  if (bad) st_agent(a.status, CTR_NBR_BAD_TABLE);
}

// clauses 7 and 9 for row i: no neighbour
__device__ __forceinline__ void nbr_no_result(const NbrArgs& a, long long i) {
  const double nan = __builtin_nan("");
  for (int m = 0; m < a.k; ++m) {
    a.dist[i * a.k + m] = nan;
    a.dist2[i * a.k + m] = nan;
    a.index[i * a.k + m] = -1;
  }
  a.count[i] = 0;
}

// One thread per row that no work item owns -- every row of a refused table, else the rows outside
// [frame_offset[0], frame_offset[T]) -- and per particle: its key.
__global__ void __launch_bounds__(NBR_THREADS) nbr_defaults_kernel(const NbrArgs a) {
  const bool ok = ld_agent(a.status) == CTR_NBR_OK;
  const long long stride = (long long)gridDim.x * NBR_THREADS;
  const long long first = ok ? a.frame_offset[0] : 0, last = ok ? a.frame_offset[a.T] : 0;
  for (long long i = (long long)blockIdx.x * NBR_THREADS + threadIdx.x; i < a.N || i < a.P; i += stride) {
    if (i < a.N && (i < first || i >= last)) nbr_no_result(a, i);
    if (i < a.P) a.pkey[i] = NBR_NO_KEY;
  }
}

// One workgroup: item_start, the exclusive scan of the frames' tiles of NBR_TILE rows.  A refused
// table has no work item.
__global__ void __launch_bounds__(NBR_THREADS) nbr_items_kernel(const NbrArgs a) {
  const bool ok = ld_agent(a.status) == CTR_NBR_OK;
  const long long total = workgroup_scan_n<NBR_THREADS, long long>(
      a.T,
      [&](long long t) { return ok ? (a.frame_offset[t + 1] - a.frame_offset[t] + NBR_TILE - 1) / NBR_TILE : 0LL; },
      [&](long long t, long long before) { a.item_start[t] = before; });
  if (threadIdx.x == 0) a.item_start[a.T] = total;
}

// clauses 1 and 2 for row r: its scaled position, NaN on every axis for a row that does not exist
__device__ __forceinline__ bool nbr_row(const NbrArgs& a, long long r, double* q) {
  bool exists = true;
#pragma unroll
  for (int d = 0; d < CTR_MAX_NDIM; ++d) {
    q[d] = 0.;
    if (d < a.ndim) {
      q[d] = a.pos[r * a.ndim + d] * a.mpp[d];
      exists = exists && fabs(q[d]) < __builtin_inf();      // false for a NaN
    }
  }
  return exists;
}

// One workgroup per work item w (striding past the grid): frame t and tile of NBR_TILE of its rows,
// found in item_start; workgroups beyond the number of items leave.  A thread owns row i: it keeps
// q_i and its K best (d2, j), ascending, in registers, and walks the rows of frame t + lag, staged a
// tile at a time in LDS with their group ids (a row that does not exist is staged as NaN: its d2
// fails d2 < limit2); every lane reads the same LDS address, a broadcast.  Candidates come in
// ascending j, so a candidate that enters on a strict d2 < kept[m] behind the equal entries keeps the
// list in (d2, j) order; an empty slot holds +inf, which no qualifying d2 reaches, and j = -1.  The
// list is indexed at compile time only.  The first k <= K entries are written.
template <int K>
__global__ void __launch_bounds__(NBR_THREADS) nbr_pairs_kernel(const NbrArgs a) {
  __shared__ double s_q[CTR_MAX_NDIM][NBR_TILE];
  __shared__ long long s_grp[NBR_TILE];
  if (ld_agent(a.status) != CTR_NBR_OK) return;
  const long long total = a.item_start[a.T];
  if ((long long)blockIdx.x >= total) return;
  const int tid = threadIdx.x, nd = a.ndim;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    long long lo = 0, hi = a.T;          // the last t with item_start[t] <= w: its frame has tile w - item_start[t]
    while (hi - lo > 1) {
      const long long mid = (lo + hi) / 2;
      if (a.item_start[mid] <= w) lo = mid;
      else hi = mid;
    }
    const long long t = lo, r1 = a.frame_offset[t + 1];
    const long long i = a.frame_offset[t] + (w - a.item_start[t]) * NBR_TILE + tid;
    const long long tc = t + a.lag;      // no overflow: T and lag are below 2^31
    const long long c0 = tc < a.T ? a.frame_offset[tc] : 0, c1 = tc < a.T ? a.frame_offset[tc + 1] : 0;
    double me[CTR_MAX_NDIM] = {};
    bool exists = false;
    long long gi = -1;
    if (i < r1) {
      exists = nbr_row(a, i, me);
      if (a.group) gi = a.group[i];
    }
    double kept[K];
    int who[K];
#pragma unroll
    for (int m = 0; m < K; ++m) { kept[m] = inf; who[m] = -1; }
    int count = 0;                       // at most N < 2^31
    for (long long tb = c0; tb < c1; tb += NBR_TILE) {
      __syncthreads();                   // the tile before is read
      const long long j = tb + tid;
      if (j < c1) {
        double q[CTR_MAX_NDIM];
        const bool there = nbr_row(a, j, q);
#pragma unroll
        for (int d = 0; d < CTR_MAX_NDIM; ++d)
          if (d < nd) s_q[d][tid] = there ? q[d] : nan;
        s_grp[tid] = a.group ? a.group[j] : -1;
      }
      __syncthreads();
      const int n = c1 - tb < NBR_TILE ? (int)(c1 - tb) : NBR_TILE;
      if (exists)
        for (int jj = 0; jj < n; ++jj) {
          if (a.lag == 0 && tb + jj == i) continue;
          double d2 = 0.;
#pragma unroll
          for (int d = 0; d < CTR_MAX_NDIM; ++d)
            if (d < nd) {
              const double x = s_q[d][jj] - me[d];
              const double x2 = x * x;            // the unit is compiled without contraction
              d2 = d == 0 ? x2 : d2 + x2;
            }
          if (!(d2 < a.limit2)) continue;         // too far, or a row that does not exist
          if (a.pairs != CTR_PCF_PAIRS_ALL) {
            const bool same = gi >= 0 && s_grp[jj] == gi;
            if (same != (a.pairs == CTR_PCF_PAIRS_SAME)) continue;
          }
          ++count;
          if (!(d2 < kept[K - 1])) continue;
          const int jg = (int)(tb + jj);          // N <= 2^31 - 1
#pragma unroll
          for (int m = K - 1; m >= 1; --m) {      // downwards: kept[m - 1] is still the old one
            const bool shift = d2 < kept[m - 1], here = d2 < kept[m];
            who[m] = shift ? who[m - 1] : here ? jg : who[m];
            kept[m] = shift ? kept[m - 1] : here ? d2 : kept[m];
          }
          if (d2 < kept[0]) { kept[0] = d2; who[0] = jg; }
        }
    }
    if (i < r1) {
#pragma unroll
      for (int m = 0; m < K; ++m)
        if (m < a.k) {
          const bool any = who[m] >= 0;
          a.dist2[i * a.k + m] = any ? kept[m] : nan;
          a.dist[i * a.k + m] = any ? sqrt(kept[m]) : nan;
          a.index[i * a.k + m] = who[m];
        }
      a.count[i] = count;
      if (a.P > 0 && who[0] >= 0) {
        const long long p = a.particle[i];
        if (p >= 0 && p < a.P) atomicMin(a.pkey + p, ordered_key(kept[0]));
      }
    }
  }
}

// One thread per particle: clause 8 from its key.  A refused table left every key as it was set.
__global__ void __launch_bounds__(NBR_THREADS) nbr_particles_kernel(const NbrArgs a) {
  const long long stride = (long long)gridDim.x * NBR_THREADS;
  for (long long p = (long long)blockIdx.x * NBR_THREADS + threadIdx.x; p < a.P; p += stride) {
    const unsigned long long key = a.pkey[p];
    const double m2 = key == NBR_NO_KEY ? __builtin_nan("") : ordered_unkey(key);
    a.particle_min2[p] = m2;
    a.particle_min[p] = sqrt(m2);
  }
}

#endif  // CTREFINE_NEIGHBORS_KERNELS_H
