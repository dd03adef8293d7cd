// neighbors_kernels.h -- nearest neighbours and proximity of a feature table: for every row the k
// nearest rows of the frame `lag` frames on, their number within a distance and, per particle, the
// smallest nearest-neighbour distance (ctr_neighbors_device; include/ctrefine.h has the rule,
// DESIGN.md 7b).  Included by tu_neighbors.hip inside its anonymous namespace, after stage_common.h
// and pair_walk.h, which has the table, the work items and the walk over the candidate frame's rows;
// here are the defaults, the list a thread keeps, the outputs and the per-particle keys.  The kernel
// boundary is the only synchronisation between workgroups; every loop is bounded by the launch's
// arguments or by row ranges of a frame_offset that nbr_check_kernel has passed.  Every output
// element has one owner thread; the only atomics are 64-bit integer minima of the per-particle keys,
// where the order cannot matter.
#ifndef CTREFINE_NEIGHBORS_KERNELS_H
#define CTREFINE_NEIGHBORS_KERNELS_H

constexpr int NBR_THREADS = PAIR_THREADS;        // a workgroup of every kernel here: 4 wavefronts
constexpr int NBR_TILE = PAIR_TILE;              // rows of a frame that a work item owns
constexpr unsigned long long NBR_NO_KEY = ~0ull; // above the key of every double: a particle without a neighbour

struct NbrArgs {
  PairTable tab;
  int k;
  long long lag, P;
  double limit2;
  const long long* particle;
  // scratch
  unsigned long long* pkey;       // [P] the ordered key of the smallest dist2[i, 0] of a particle
  // out
  double* dist;
  double* dist2;
  long long* index;
  long long* count;
  double* particle_min;
  double* particle_min2;
};

__global__ void __launch_bounds__(NBR_THREADS) nbr_check_kernel(const NbrArgs a) { pair_check(a.tab, CTR_NBR_BAD_TABLE); }

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
  const bool ok = pair_ok(a.tab);
  const long long stride = (long long)gridDim.x * NBR_THREADS;
  const long long first = ok ? a.tab.frame_offset[0] : 0, last = ok ? a.tab.frame_offset[a.tab.T] : 0;
  for (long long i = (long long)blockIdx.x * NBR_THREADS + threadIdx.x; i < a.tab.N || i < a.P; i += stride) {
    if (i < a.tab.N && (i < first || i >= last)) nbr_no_result(a, i);
    if (i < a.P) a.pkey[i] = NBR_NO_KEY;
  }
}

__global__ void __launch_bounds__(NBR_THREADS) nbr_items_kernel(const NbrArgs a) { pair_items(a.tab); }

// One workgroup per work item w (striding past the grid): frame t and tile of NBR_TILE of its rows,
// found in item_start; workgroups beyond the number of items leave.  A thread owns row i: it keeps
// q_i and its K best (d2, j), ascending, in registers, and walks the rows of frame t + lag
// (pair_walk: a candidate exists when it is finite, clauses 1 and 2).  Candidates come in ascending
// j, so a candidate that enters on a strict d2 < kept[m] behind the equal entries keeps the list in
// (d2, j) order; an empty slot holds +inf, which no qualifying d2 reaches, and j = -1.  The list is
// indexed at compile time only.  The first k <= K entries are written.
template <int K>
__global__ void __launch_bounds__(NBR_THREADS) nbr_pairs_kernel(const NbrArgs a) {
  __shared__ PairTile s_tile;
  if (!pair_ok(a.tab)) return;
  const long long total = a.tab.item_start[a.tab.T];
  if ((long long)blockIdx.x >= total) return;
  const int tid = threadIdx.x;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long t = pair_item_frame(a.tab, w), r1 = a.tab.frame_offset[t + 1];
    const long long i = a.tab.frame_offset[t] + (w - a.tab.item_start[t]) * NBR_TILE + tid;
    const long long tc = t + a.lag;      // no overflow: T and lag are below 2^31
    const long long c0 = tc < a.tab.T ? a.tab.frame_offset[tc] : 0, c1 = tc < a.tab.T ? a.tab.frame_offset[tc + 1] : 0;
    PairRow me = {};
    long long gi = -1;
    if (i < r1) {
      me = pair_row(a.tab, i);
      if (a.tab.group) gi = a.tab.group[i];
    }
    double kept[K];
    int who[K];
#pragma unroll
    for (int m = 0; m < K; ++m) { kept[m] = inf; who[m] = -1; }
    int count = 0;                       // at most N < 2^31
    pair_walk(
        a.tab, s_tile, c0, c1, me.exists, me.q, gi, a.lag == 0 ? i : -1, a.limit2,
        [&](long long j) { return pair_row(a.tab, j); },
        [&](long long j, double d2) {
          ++count;
          if (!(d2 < kept[K - 1])) return;
          const int jg = (int)j;                  // N <= 2^31 - 1
#pragma unroll
          for (int m = K - 1; m >= 1; --m) {      // downwards: kept[m - 1] is still the old one
            const bool shift = d2 < kept[m - 1], here = d2 < kept[m];
            who[m] = shift ? who[m - 1] : here ? jg : who[m];
            kept[m] = shift ? kept[m - 1] : here ? d2 : kept[m];
          }
          if (d2 < kept[0]) { kept[0] = d2; who[0] = jg; }
        },
        []() {});
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
