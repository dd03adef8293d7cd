// pair_corr_kernels.h -- pair correlation function g(r) of a feature table: an all-pairs distance
// histogram per frame and an edge correction per reference row (ctr_pair_correlation_device;
// include/ctrefine.h has the rule).  Included by tu_pair_corr.hip inside its anonymous
// namespace, after stage_common.h and pair_walk.h, which has the table, the work items and the walk
// over a frame's rows; here are the box, the reference rows, the binning of a pair, the flush of a
// workgroup's histogram, the arc weight, finish and pool.  The kernel boundary is the only
// synchronisation between workgroups; every loop is bounded by the launch's arguments or by row
// ranges of a frame_offset that pcf_check_kernel has passed.  Integer atomics only (LDS and the int64
// counts, where the order cannot matter); every sum of doubles is taken in an order that the input
// alone decides.
#ifndef CTREFINE_PAIR_CORR_KERNELS_H
#define CTREFINE_PAIR_CORR_KERNELS_H

constexpr int PCF_THREADS = PAIR_THREADS;        // a workgroup of every kernel here: 4 wavefronts
constexpr int PCF_TILE = PAIR_TILE;              // reference rows of a work item
constexpr int PCF_MAX_BINS = CTR_PCF_MAX_BINS;   // edge2 and the histogram of a workgroup are in LDS
constexpr int PCF_FLUSH_TILES = 16384;           // 256 * 256 * 16384 = 2^30 pairs at most between two flushes of the 32-bit counters
constexpr double PCF_HALF_PI = 1.5707963267948966, PCF_TWO_PI = 6.283185307179586;

struct PcfArgs {
  PairTable tab;
  int edge;
  long long B;
  double dr;
  const double* box;          // [2, ndim]: lo, hi in scaled units
  const double* edge2;        // [B + 1]
  const double* shell;        // [B]
  // scratch
  double* wpart;              // [max_items, B] 'arc': the weight of a work item's reference rows
  // out
  double* g;
  double* g_frame;
  long long* count;
  double* weight;
  long long* n_ref;
  long long* n_rows;
};

__global__ void __launch_bounds__(PCF_THREADS) pcf_check_kernel(const PcfArgs a) { pair_check(a.tab, CTR_PCF_BAD_TABLE); }

struct PcfBox {
  double lo[CTR_MAX_NDIM], hi[CTR_MAX_NDIM];
};

__device__ __forceinline__ PcfBox pcf_box(const PcfArgs& a) {
  PcfBox o;
#pragma unroll
  for (int d = 0; d < CTR_MAX_NDIM; ++d) {
    o.lo[d] = d < a.tab.ndim ? a.box[d] : 0.;
    o.hi[d] = d < a.tab.ndim ? a.box[a.tab.ndim + d] : 0.;
  }
  return o;
}

// clause 3: the product over the axes, in axis order, of hi - lo
__device__ __forceinline__ double pcf_volume(const PcfBox& box, int nd) {
  double v = box.hi[0] - box.lo[0];
#pragma unroll
  for (int d = 1; d < CTR_MAX_NDIM; ++d)
    if (d < nd) v = v * (box.hi[d] - box.lo[d]);
  return v;
}

// clauses 2, 4 and 5 for row r: its scaled position, whether it exists (finite and within the box),
// whether it is a reference row
struct PcfRow : PairRow {
  bool ref;
};

__device__ __forceinline__ PcfRow pcf_row(const PcfArgs& a, const PcfBox& box, double r_max, long long r) {
  bool inner = true;      // asked of a row that exists only: the box's test runs while the axes before passed
  PcfRow o = {pair_row(a.tab, r, [&](int d, double q) {
                inner = inner && q - box.lo[d] >= r_max && box.hi[d] - q >= r_max;
                return q >= box.lo[d] && q <= box.hi[d];
              }),
              false};
  o.ref = o.exists && (a.edge != CTR_PCF_EDGE_INTERIOR || inner);
  return o;
}

// One workgroup per frame (striding past the grid): n_rows, n_ref, and the frame's counts zeroed.
// A refused table: zeros.
__global__ void __launch_bounds__(PCF_THREADS) pcf_frames_kernel(const PcfArgs a) {
  __shared__ int s_rows, s_ref;
  const bool ok = pair_ok(a.tab);
  const int tid = threadIdx.x;
  const PcfBox box = pcf_box(a);
  const double r_max = (double)a.B * a.dr;
  for (long long t = blockIdx.x; t < a.tab.T; t += gridDim.x) {
    __syncthreads();
    if (tid == 0) { s_rows = 0; s_ref = 0; }
    __syncthreads();
    int rows = 0, ref = 0;
    if (ok)
      for (long long r = a.tab.frame_offset[t] + tid; r < a.tab.frame_offset[t + 1]; r += PCF_THREADS) {
        const PcfRow row = pcf_row(a, box, r_max, r);
        rows += row.exists ? 1 : 0;
        ref += row.ref ? 1 : 0;
      }
    if (rows) atomicAdd(&s_rows, rows);      // at most N < 2^31
    if (ref) atomicAdd(&s_ref, ref);
    __syncthreads();
    if (tid == 0) { a.n_rows[t] = s_rows; a.n_ref[t] = s_ref; }
    for (long long b = tid; b < a.B; b += PCF_THREADS) a.count[t * a.B + b] = 0;
  }
}

__global__ void __launch_bounds__(PCF_THREADS) pcf_items_kernel(const PcfArgs a) { pair_items(a.tab); }

// the angle of the circle of radius R that a quadrant with its walls at a (along axis 0) and b
// (along axis 1) holds: clause 8
__device__ __forceinline__ double pcf_quadrant(double wall_a, double wall_b, double R) {
  if (wall_a >= R && wall_b >= R) return PCF_HALF_PI;
  const double v = asin(fmin(wall_b / R, 1.)) - acos(fmin(wall_a / R, 1.));
  return v > 0. ? v : 0.;
}

// the fraction of the circle of radius R around (q0, q1) inside the box; exactly 1 without
// trigonometry for a row further than R from every wall
__device__ __forceinline__ double pcf_arc_fraction(double q0, double q1, const PcfBox& box, double R) {
  const double a0 = box.hi[0] - q0, a1 = q0 - box.lo[0], b0 = box.hi[1] - q1, b1 = q1 - box.lo[1];
  if (a0 >= R && a1 >= R && b0 >= R && b1 >= R) return 1.;
  return (((pcf_quadrant(a0, b0, R) + pcf_quadrant(a0, b1, R)) + pcf_quadrant(a1, b0, R)) + pcf_quadrant(a1, b1, R)) / PCF_TWO_PI;
}

// the histogram of the workgroup added to the frame's counts, and zeroed by the thread that read it
__device__ __forceinline__ void pcf_flush(const PcfArgs& a, unsigned* s_hist, long long t) {
  for (int b = threadIdx.x; b < a.B; b += PCF_THREADS) {
    const unsigned c = s_hist[b];
    if (c) atomicAdd((unsigned long long*)(a.count + t * a.B + b), (unsigned long long)c);
    s_hist[b] = 0;
  }
}

// clause 7 for a pair at d2 < edge2[B]: a guess from the square root, corrected against the edges that
// the rule compares with, and one LDS atomic
__device__ __forceinline__ void pcf_bin(double d2, double inv_dr, int B, const double* s_edge2, unsigned* s_hist) {
  int b = (int)fmin(sqrt(d2) * inv_dr, (double)(B - 1));
  while (b > 0 && d2 < s_edge2[b]) --b;
  while (d2 >= s_edge2[b + 1]) ++b;               // ends below B: d2 < edge2[B]
  atomicAdd(&s_hist[b], 1u);
}

// One workgroup per work item w (striding past the grid): frame t and tile k of PCF_TILE of its
// rows, found in item_start; workgroups beyond the number of items leave.  A thread keeps its
// reference row in registers and walks the frame's rows (pair_walk: a candidate exists when it is
// finite and within the box); it bins with LDS atomics; the workgroup adds its histogram to
// count[t, :] with 64-bit atomics.  'arc': one thread per bin then walks the tile's reference rows in
// row order.
__global__ void __launch_bounds__(PCF_THREADS) pcf_pairs_kernel(const PcfArgs a) {
  __shared__ double s_edge2[PCF_MAX_BINS + 1];
  __shared__ unsigned s_hist[PCF_MAX_BINS];
  __shared__ PairTile s_tile;
  if (!pair_ok(a.tab)) return;
  const long long total = a.tab.item_start[a.tab.T];
  if ((long long)blockIdx.x >= total) return;
  const int tid = threadIdx.x, B = (int)a.B;
  const PcfBox box = pcf_box(a);
  const double r_max = (double)a.B * a.dr, inv_dr = 1. / a.dr, nan = __builtin_nan("");
  for (int b = tid; b <= B; b += PCF_THREADS) s_edge2[b] = a.edge2[b];
  for (int b = tid; b < B; b += PCF_THREADS) s_hist[b] = 0;
  const double e2_max = a.edge2[B];
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long t = pair_item_frame(a.tab, w), r0 = a.tab.frame_offset[t], r1 = a.tab.frame_offset[t + 1];
    const long long i = r0 + (w - a.tab.item_start[t]) * PCF_TILE + tid;
    PcfRow me = {};
    long long gi = -1;
    if (i < r1) {
      me = pcf_row(a, box, r_max, i);
      if (a.tab.group) gi = a.tab.group[i];
    }
    long long tiles = 0;
    pair_walk(                           // its first barrier: the histogram is zero
        a.tab, s_tile, r0, r1, me.ref, me.q, gi, i, e2_max,
        [&](long long j) { return pcf_row(a, box, r_max, j); },
        [&](long long, double d2) { pcf_bin(d2, inv_dr, B, s_edge2, s_hist); },
        [&]() {
          if (++tiles % PCF_FLUSH_TILES == 0) {
            __syncthreads();
            pcf_flush(a, s_hist, t);
          }
        });
    __syncthreads();
    pcf_flush(a, s_hist, t);
    if (a.edge == CTR_PCF_EDGE_ARC) {
      s_tile.q[0][tid] = me.ref ? me.q[0] : nan;   // the neighbour tiles are read: the barrier above
      s_tile.q[1][tid] = me.ref ? me.q[1] : nan;
      __syncthreads();
      for (int b = tid; b < B; b += PCF_THREADS) {
        const double R = (double)b * a.dr + a.dr / 2;
        double sum = 0.;
        for (int k = 0; k < PCF_TILE; ++k) {
          const double q0 = s_tile.q[0][k];
          if (q0 == q0) sum += pcf_arc_fraction(q0, s_tile.q[1][k], box, R);
        }
        a.wpart[w * a.B + b] = sum;
      }
    }
  }
}

// One thread per (frame, bin): the weight (the partials of the frame's work items added in item
// order, or n_ref) and g_frame, clauses 8 and 9.  A refused table: NaN.
__global__ void __launch_bounds__(PCF_THREADS) pcf_finish_kernel(const PcfArgs a) {
  const bool ok = pair_ok(a.tab);
  const long long stride = (long long)gridDim.x * PCF_THREADS;
  const double volume = pcf_volume(pcf_box(a), a.tab.ndim), nan = __builtin_nan("");
  for (long long e = (long long)blockIdx.x * PCF_THREADS + threadIdx.x; e < a.tab.T * a.B; e += stride) {
    const long long t = e / a.B, b = e % a.B;
    double w = nan, gf = nan;
    if (ok) {
      if (a.edge == CTR_PCF_EDGE_ARC) {
        w = 0.;
        for (long long k = a.tab.item_start[t]; k < a.tab.item_start[t + 1]; ++k) w += a.wpart[k * a.B + b];
      } else {
        w = (double)a.n_ref[t];
      }
      const double rho = (double)(a.n_rows[t] - 1) / volume;
      const double den = (rho * a.shell[b]) * w;
      if (den > 0. && den < __builtin_inf()) gf = (double)a.count[e] / den;
    }
    a.weight[e] = w;
    a.g_frame[e] = gf;
  }
}

// One thread per bin walks the frames in order: clause 10.  A refused table: NaN.
__global__ void __launch_bounds__(PCF_THREADS) pcf_pool_kernel(const PcfArgs a) {
  const bool ok = pair_ok(a.tab);
  const long long stride = (long long)gridDim.x * PCF_THREADS;
  const double volume = pcf_volume(pcf_box(a), a.tab.ndim);
  for (long long b = (long long)blockIdx.x * PCF_THREADS + threadIdx.x; b < a.B; b += stride) {
    long long c = 0;
    double den = 0.;
    bool any = false;
    const double shell = a.shell[b];
#pragma unroll 8
    for (long long t = 0; ok && t < a.tab.T; ++t) {
      const double rho = (double)(a.n_rows[t] - 1) / volume;
      const double d = (rho * shell) * a.weight[t * a.B + b];
      c += a.count[t * a.B + b];
      if (d > 0. && d < __builtin_inf()) { den += d; any = true; }
    }
    a.g[b] = any ? (double)c / den : __builtin_nan("");
  }
}

#endif  // CTREFINE_PAIR_CORR_KERNELS_H
