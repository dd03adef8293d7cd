// pair_corr_kernels.h -- pair correlation function g(r) of a feature table: an all-pairs distance
// histogram per frame and an edge correction per reference row (ctr_pair_correlation_device;
// include/ctrefine.h has the rule).  Included by tu_pair_corr.hip inside its anonymous
// namespace, after stage_common.h.  The kernel boundary is the only synchronisation between
// workgroups; every loop is bounded by the launch's arguments or by row ranges of a frame_offset that
// pcf_check_kernel has passed.  Integer atomics only (LDS and the int64 counts, where the order cannot
// matter); every sum of doubles is taken in an order that the input alone decides.
#ifndef CTREFINE_PAIR_CORR_KERNELS_H
#define CTREFINE_PAIR_CORR_KERNELS_H

constexpr int PCF_THREADS = 256;                 // a workgroup of every kernel here: 4 wavefronts
constexpr int PCF_TILE = PCF_THREADS;            // rows of a frame that a work item refers to, and that it stages at a time
constexpr int PCF_MAX_BINS = CTR_PCF_MAX_BINS;   // edge2 and the histogram of a workgroup are in LDS
constexpr int PCF_FLUSH_TILES = 16384;           // 256 * 256 * 16384 = 2^30 pairs at most between two flushes of the 32-bit counters
constexpr double PCF_HALF_PI = 1.5707963267948966, PCF_TWO_PI = 6.283185307179586;

struct PcfArgs {
  int ndim, edge, pairs;
  long long B, T, N;
  double dr;
  double mpp[CTR_MAX_NDIM];
  const double* pos;
  const long long* frame_offset;
  const long long* group;
  const double* box;          // [2, ndim]: lo, hi in scaled units
  const double* edge2;        // [B + 1]
  const double* shell;        // [B]
  // scratch
  long long* item_start;      // [T + 1] the first work item of a frame; [T]: their number
  double* wpart;              // [max_items, B] 'arc': the weight of a work item's reference rows
  // out
  double* g;
  double* g_frame;
  long long* count;
  double* weight;
  long long* n_ref;
  long long* n_rows;
  int* status;
};

// the caller's frame_offset, before any kernel follows it.  status[0] was zeroed in front of this kernel.
__global__ void __launch_bounds__(PCF_THREADS) pcf_check_kernel(const PcfArgs a) {
  const long long stride = (long long)gridDim.x * PCF_THREADS;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * PCF_THREADS + threadIdx.x; i <= a.T; i += stride)
    bad |= offsets_bad(a.frame_offset, i, a.T, a.N);
  if (bad) st_agent(a.status, CTR_PCF_BAD_TABLE);
}

struct PcfBox {
  double lo[CTR_MAX_NDIM], hi[CTR_MAX_NDIM];
};

__device__ __forceinline__ PcfBox pcf_box(const PcfArgs& a) {
  PcfBox o;
#pragma unroll
  for (int d = 0; d < CTR_MAX_NDIM; ++d) {
    o.lo[d] = d < a.ndim ? a.box[d] : 0.;
    o.hi[d] = d < a.ndim ? a.box[a.ndim + d] : 0.;
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

// clauses 2, 4 and 5 for row r: its scaled position, whether it exists, whether it is a reference row
struct PcfRow {
  double q[CTR_MAX_NDIM];
  bool exists, ref;
};

__device__ __forceinline__ PcfRow pcf_row(const PcfArgs& a, const PcfBox& box, double r_max, long long r) {
  PcfRow o;
  bool exists = true, inner = true;
#pragma unroll
  for (int d = 0; d < CTR_MAX_NDIM; ++d) {
    o.q[d] = 0.;
    if (d < a.ndim) {
      const double q = a.pos[r * a.ndim + d] * a.mpp[d];
      o.q[d] = q;
      exists = exists && fabs(q) < __builtin_inf() && q >= box.lo[d] && q <= box.hi[d];     // false for a NaN
      inner = inner && q - box.lo[d] >= r_max && box.hi[d] - q >= r_max;
    }
  }
  o.exists = exists;
  o.ref = exists && (a.edge != CTR_PCF_EDGE_INTERIOR || inner);
  return o;
}

// One workgroup per frame (striding past the grid): n_rows, n_ref, and the frame's counts zeroed.
// A refused table: zeros.
__global__ void __launch_bounds__(PCF_THREADS) pcf_frames_kernel(const PcfArgs a) {
  __shared__ int s_rows, s_ref;
  const bool ok = ld_agent(a.status) == CTR_PCF_OK;
  const int tid = threadIdx.x;
  const PcfBox box = pcf_box(a);
  const double r_max = (double)a.B * a.dr;
  for (long long t = blockIdx.x; t < a.T; t += gridDim.x) {
    __syncthreads();
    if (tid == 0) { s_rows = 0; s_ref = 0; }
    __syncthreads();
    int rows = 0, ref = 0;
    if (ok)
      for (long long r = a.frame_offset[t] + tid; r < a.frame_offset[t + 1]; r += PCF_THREADS) {
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

// One workgroup: item_start, the exclusive scan of the frames' tiles of PCF_TILE rows.  A refused
// table has no work item.
__global__ void __launch_bounds__(PCF_THREADS) pcf_items_kernel(const PcfArgs a) {
  const bool ok = ld_agent(a.status) == CTR_PCF_OK;
  const long long total = workgroup_scan_n<PCF_THREADS, long long>(
      a.T,
      [&](long long t) { return ok ? (a.frame_offset[t + 1] - a.frame_offset[t] + PCF_TILE - 1) / PCF_TILE : 0LL; },
      [&](long long t, long long before) { a.item_start[t] = before; });
  if (threadIdx.x == 0) a.item_start[a.T] = total;
}

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

// One workgroup per work item w (striding past the grid): frame t and tile k of PCF_TILE of its
// rows, found in item_start; workgroups beyond the number of items leave.  A thread keeps its
// reference row in registers and walks the frame's rows, staged a tile at a time in LDS with
// their group ids (a row that does not exist is staged as NaN: its distance fails every
// comparison); it bins with LDS atomics; the workgroup adds its histogram to count[t, :] with 64-bit
// atomics.  'arc': one thread per bin then walks the tile's reference rows in row order.
__global__ void __launch_bounds__(PCF_THREADS) pcf_pairs_kernel(const PcfArgs a) {
  __shared__ double s_edge2[PCF_MAX_BINS + 1];
  __shared__ unsigned s_hist[PCF_MAX_BINS];
  __shared__ double s_q[CTR_MAX_NDIM][PCF_TILE];
  __shared__ long long s_grp[PCF_TILE];
  if (ld_agent(a.status) != CTR_PCF_OK) return;
  const long long total = a.item_start[a.T];
  if ((long long)blockIdx.x >= total) return;
  const int tid = threadIdx.x, nd = a.ndim, B = (int)a.B;
  const PcfBox box = pcf_box(a);
  const double r_max = (double)a.B * a.dr, inv_dr = 1. / a.dr, nan = __builtin_nan("");
  for (int b = tid; b <= B; b += PCF_THREADS) s_edge2[b] = a.edge2[b];
  for (int b = tid; b < B; b += PCF_THREADS) s_hist[b] = 0;
  const double e2_max = a.edge2[B];
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    long long lo = 0, hi = a.T;          // the last t with item_start[t] <= w: its frame has tile w - item_start[t]
    while (hi - lo > 1) {
      const long long mid = (lo + hi) / 2;
      if (a.item_start[mid] <= w) lo = mid;
      else hi = mid;
    }
    const long long t = lo, r0 = a.frame_offset[t], r1 = a.frame_offset[t + 1];
    const long long i = r0 + (w - a.item_start[t]) * PCF_TILE + tid;
    PcfRow me = {};
    long long gi = -1;
    if (i < r1) {
      me = pcf_row(a, box, r_max, i);
      if (a.group) gi = a.group[i];
    }
    long long tiles = 0;
    for (long long tb = r0; tb < r1; tb += PCF_TILE) {
      __syncthreads();                   // the tile before is read, the histogram is zero
      const long long j = tb + tid;
      if (j < r1) {
        const PcfRow row = pcf_row(a, box, r_max, j);
#pragma unroll
        for (int d = 0; d < CTR_MAX_NDIM; ++d)
          if (d < nd) s_q[d][tid] = row.exists ? row.q[d] : nan;
        s_grp[tid] = a.group ? a.group[j] : -1;
      }
      __syncthreads();
      const int n = r1 - tb < PCF_TILE ? (int)(r1 - tb) : PCF_TILE;
      if (me.ref)
        for (int jj = 0; jj < n; ++jj) {
          if (tb + jj == i) continue;
          double d2 = 0.;
#pragma unroll
          for (int d = 0; d < CTR_MAX_NDIM; ++d)
            if (d < nd) {
              const double x = s_q[d][jj] - me.q[d];
              const double x2 = x * x;            // the unit is compiled without contraction
              d2 = d == 0 ? x2 : d2 + x2;
            }
          if (!(d2 < e2_max)) continue;           // beyond the last edge, or a row that does not exist
          if (a.pairs != CTR_PCF_PAIRS_ALL) {
            const bool same = gi >= 0 && s_grp[jj] == gi;
            if (same != (a.pairs == CTR_PCF_PAIRS_SAME)) continue;
          }
          // a guess from the square root, corrected against the edges that the rule compares with
          int b = (int)fmin(sqrt(d2) * inv_dr, (double)(B - 1));
          while (b > 0 && d2 < s_edge2[b]) --b;
          while (d2 >= s_edge2[b + 1]) ++b;       // ends below B: d2 < edge2[B]
          atomicAdd(&s_hist[b], 1u);
        }
      if (++tiles % PCF_FLUSH_TILES == 0) {
        __syncthreads();
        pcf_flush(a, s_hist, t);
      }
    }
    __syncthreads();
    pcf_flush(a, s_hist, t);
    if (a.edge == CTR_PCF_EDGE_ARC) {
      s_q[0][tid] = me.ref ? me.q[0] : nan;        // the neighbour tiles are read: the barrier above
      s_q[1][tid] = me.ref ? me.q[1] : nan;
      __syncthreads();
      for (int b = tid; b < B; b += PCF_THREADS) {
        const double R = (double)b * a.dr + a.dr / 2;
        double sum = 0.;
        for (int k = 0; k < PCF_TILE; ++k) {
          const double q0 = s_q[0][k];
          if (q0 == q0) sum += pcf_arc_fraction(q0, s_q[1][k], box, R);
        }
        a.wpart[w * a.B + b] = sum;
      }
    }
  }
}

// One thread per (frame, bin): the weight (the partials of the frame's work items added in item
// order, or n_ref) and g_frame, clauses 8 and 9.  A refused table: NaN.
__global__ void __launch_bounds__(PCF_THREADS) pcf_finish_kernel(const PcfArgs a) {
  const bool ok = ld_agent(a.status) == CTR_PCF_OK;
  const long long stride = (long long)gridDim.x * PCF_THREADS;
  const double volume = pcf_volume(pcf_box(a), a.ndim), nan = __builtin_nan("");
  for (long long e = (long long)blockIdx.x * PCF_THREADS + threadIdx.x; e < a.T * a.B; e += stride) {
    const long long t = e / a.B, b = e % a.B;
    double w = nan, gf = nan;
    if (ok) {
      if (a.edge == CTR_PCF_EDGE_ARC) {
        w = 0.;
        for (long long k = a.item_start[t]; k < a.item_start[t + 1]; ++k) w += a.wpart[k * a.B + b];
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
  const bool ok = ld_agent(a.status) == CTR_PCF_OK;
  const long long stride = (long long)gridDim.x * PCF_THREADS;
  const double volume = pcf_volume(pcf_box(a), a.ndim);
  for (long long b = (long long)blockIdx.x * PCF_THREADS + threadIdx.x; b < a.B; b += stride) {
    long long c = 0;
    double den = 0.;
    bool any = false;
    const double shell = a.shell[b];
#pragma unroll 8
    for (long long t = 0; ok && t < a.T; ++t) {
      const double rho = (double)(a.n_rows[t] - 1) / volume;
      const double d = (rho * shell) * a.weight[t * a.B + b];
      c += a.count[t * a.B + b];
      if (d > 0. && d < __builtin_inf()) { den += d; any = true; }
    }
    a.g[b] = any ? (double)c / den : __builtin_nan("");
  }
}

#endif  // CTREFINE_PAIR_CORR_KERNELS_H
