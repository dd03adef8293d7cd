// vanhove_kernels.h -- van Hove displacement distributions of linked particles: the histogram of
// the displacements at a list of lags, per coordinate and radial, with counted tails, the first,
// second and fourth moment and the non-Gaussian parameter (ctr_vanhove_device; include/ctrefine.h
// has the rule).  Included by tu_msd.hip inside its anonymous namespace, after
// msd_kernels.h: the table check, the sorted rows, msd_partner and the order of the ensemble's sums
// are the MSD stage's.  The kernel boundary is the only synchronisation between workgroups; every
// loop is bounded by the launch's arguments or by row ranges that msd_rows_kernel wrote from a table
// msd_check_kernel has passed; integer atomics only, in LDS and on the int64 tables: every float sum
// is taken in an order that the input alone decides.
#ifndef CTREFINE_VANHOVE_KERNELS_H
#define CTREFINE_VANHOVE_KERNELS_H

static_assert(CTR_VANHOVE_OK == CTR_MSD_OK && CTR_VANHOVE_BAD_TABLE == CTR_MSD_BAD_TABLE,
              "msd_check_kernel writes the status of this stage");

constexpr int VH_MAX_LAGS = CTR_VANHOVE_MAX_LAGS;
constexpr int VH_MAX_H = CTR_VANHOVE_MAX_HALF_BINS;
constexpr int VH_VALUES = 3 * CTR_MAX_NDIM;      // sums of a lag: d, d^2 and d^4 per coordinate
// counters of a workgroup: per coordinate 2 H bins, below, above; then H radial bins and above_r
constexpr int VH_COUNTERS = CTR_MAX_NDIM * (2 * VH_MAX_H + 2) + VH_MAX_H + 1;

struct VanhoveArgs {
  MsdArgs t;                 // the table and its sorted rows; t.L, t.M, t.part and the outputs of the MSD are not used
  int K, H;                  // lags; half the bins of a coordinate
  long long lag[VH_MAX_LAGS];
  double bin_width, inv_width;
  const double* edges;       // [2 H + 1]
  const double* edge2;       // [H + 1]
  // scratch
  double* part;              // [chunks, K, 3 ndim] sums of the chunks (t.n_chunks of them): d, d^2, d^4
  long long* part_n;         // [chunks, K]
  // out
  unsigned long long* count;      // [K, ndim, 2 H]
  unsigned long long* below;      // [K, ndim]
  unsigned long long* above;      // [K, ndim]
  unsigned long long* count_r;    // [K, H]
  unsigned long long* above_r;    // [K]
  long long* n;                   // [K]
  double* density;                // [K, ndim, 2 H]
  double* density_r;              // [K, H]
  double* mean_d;                 // [K, ndim]
  double* mean_d2;
  double* mean_d4;
  double* alpha2;
};

// the int64 tables zeroed in front of vanhove_bin_kernel, whatever the status
__global__ void __launch_bounds__(MSD_THREADS) vanhove_clear_kernel(const VanhoveArgs v) {
  const long long stride = (long long)gridDim.x * MSD_THREADS;
  const long long nd = v.t.ndim, B = 2LL * v.H;
  const long long cells = (long long)v.K * nd * B, tails = (long long)v.K * nd, radial = (long long)v.K * v.H;
  for (long long i = (long long)blockIdx.x * MSD_THREADS + threadIdx.x; i < cells; i += stride) {
    v.count[i] = 0;
    if (i < tails) v.below[i] = v.above[i] = 0;
    if (i < radial) v.count_r[i] = 0;          // radial < cells
    if (i < v.K) v.above_r[i] = 0;
  }
}

// what a thread has added for one lag
struct VhSums {
  double v[VH_VALUES];       // d per coordinate, then d^2, then d^4
  long long n;
};

// the workgroup's sum of every thread's sums, in every thread: msd_reduce's tree with a third moment
struct VhRed {
  double v[MSD_WAVES][VH_VALUES];
  long long n[MSD_WAVES];
};

__device__ __forceinline__ void vanhove_reduce(VhSums& s, VhRed& red, int nd) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
#pragma unroll
    for (int d = 0; d < CTR_MAX_NDIM; ++d)
      if (d < nd) {
        s.v[d] += __shfl_down(s.v[d], w);
        s.v[CTR_MAX_NDIM + d] += __shfl_down(s.v[CTR_MAX_NDIM + d], w);
        s.v[2 * CTR_MAX_NDIM + d] += __shfl_down(s.v[2 * CTR_MAX_NDIM + d], w);
      }
    s.n += __shfl_down(s.n, w);
  }
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < VH_VALUES; ++d) red.v[wave][d] = s.v[d];
    red.n[wave] = s.n;
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < VH_VALUES; ++d) s.v[d] = (red.v[0][d] + red.v[1][d]) + (red.v[2][d] + red.v[3][d]);
  s.n = (red.n[0] + red.n[1]) + (red.n[2] + red.n[3]);
}

// The counter of x among the 2 H bins of a coordinate (clause 5): 2 H for below, 2 H + 1 for above, -1
// for a NaN.  The division guesses, the handed-over edges decide; lo = edges[0], hi = edges[2 H].
__device__ __forceinline__ int vanhove_bin(const double* edges, double x, double lo, double hi, double inv_width, int H) {
#pragma clang fp contract(off)
  const int B = 2 * H;
  if (x < lo) return B;
  if (x >= hi) return B + 1;
  if (!(x >= lo)) return -1;
  int b = (int)floor(x * inv_width) + H;       // |x * inv_width| <= H (1 + 2^-51): no overflow
  b = b < 0 ? 0 : b > B - 1 ? B - 1 : b;
  while (b > 0 && x < edges[b]) --b;           // edges[0] <= x < edges[B]: both loops end inside
  while (b < B - 1 && x >= edges[b + 1]) ++b;
  return b;
}

// The counter of d2 among the H radial bins (clause 6): H for above_r, -1 for a NaN.
__device__ __forceinline__ int vanhove_bin_r(const double* edge2, double d2, double hi2, double inv_width, int H) {
#pragma clang fp contract(off)
  if (d2 >= hi2) return H;
  if (!(d2 >= 0.)) return -1;
  int b = (int)(sqrt(d2) * inv_width);         // 0 <= d2 < edge2[H]
  b = b > H - 1 ? H - 1 : b;
  while (b > 0 && d2 < edge2[b]) --b;
  while (b < H - 1 && d2 >= edge2[b + 1]) ++b;
  return b;
}

// One workgroup per chunk c of MSD_CHUNK consecutive ids and lag index q (striding past the grid):
// the pairs of lag[q] of the chunk's ids, whose rows are the sorted rows [r0, r1), visited as
// msd_chunk_kernel visits them.  The moments are added in registers and reduced in its tree, one
// partial per (chunk, lag); the counters are uint32 in LDS (a chunk has fewer than 2^31 rows and a row
// opens at most one pair of a lag) and the non-zero ones are added to the int64 tables, which
// vanhove_clear_kernel zeroed: integer sums, the same bytes in any order.
__global__ void __launch_bounds__(MSD_THREADS) vanhove_bin_kernel(const VanhoveArgs v) {
#pragma clang fp contract(off)
  __shared__ unsigned s_count[VH_COUNTERS];
  __shared__ VhRed s_red;
  __shared__ int s_lo, s_hi, s_span;
  const MsdArgs& a = v.t;
  if (ld_agent(a.status) != CTR_VANHOVE_OK) return;
  const int tid = threadIdx.x, nd = a.ndim, H = v.H, B = 2 * H;
  const int per_axis = B + 2, used = nd * per_axis + H + 1;       // <= VH_COUNTERS: the launch checked nd and H
  const double lo = v.edges[0], hi = v.edges[B], hi2 = v.edge2[H];
  for (long long w = blockIdx.x; w < a.n_chunks * v.K; w += gridDim.x) {
    const long long c = w / v.K;
    const int q = (int)(w % v.K);
    const long long k = v.lag[q];
    __syncthreads();                           // the item before is done with LDS
    if (tid == 0) { s_lo = 0x7fffffff; s_hi = 0; s_span = 0; }
    for (int j = tid; j < used; j += MSD_THREADS) s_count[j] = 0;
    __syncthreads();
    const long long p_end = (c + 1) * MSD_CHUNK < a.P ? (c + 1) * MSD_CHUNK : a.P;
    for (long long p = c * MSD_CHUNK + tid; p < p_end; p += MSD_THREADS) {
      const int b = a.first[p], e = a.last[p];
      if (e > b) {
        atomicMin(&s_lo, b);
        atomicMax(&s_hi, e);
        atomicMax(&s_span, msd_raw(a.code[e - 1]) - msd_raw(a.code[b]));
      }
    }
    __syncthreads();
    const long long r0 = s_lo < s_hi ? s_lo : 0, r1 = s_lo < s_hi ? s_hi : 0;
    VhSums s = {};
    if (k <= s_span)                           // else no id of the chunk spans the lag
      for (long long i = r0 + tid; i < r1; i += MSD_THREADS) {
        const int f = a.code[i];
        if (f < 0) continue;
        const long long j = msd_partner(a.code, i, (long long)a.last[a.key[i]], f, k, a.T);
        if (j < 0) continue;
        double d2 = 0.;
#pragma unroll
        for (int d = 0; d < CTR_MAX_NDIM; ++d)
          if (d < nd) {
            const double diff = a.spos[j * nd + d] - a.spos[i * nd + d];
            const double x = diff * a.mpp[d];      // nothing here is contracted: x, x2 and d2 are NumPy's doubles
            const double x2 = x * x;
            // the running sums of d and d^2 as the MSD unit takes them, the product and the addition in
            // one fused operation (msd_add as that unit is compiled): the bytes of the ensemble's MSD
            s.v[d] = fma(a.mpp[d], diff, s.v[d]);
            s.v[CTR_MAX_NDIM + d] = fma(x, x, s.v[CTR_MAX_NDIM + d]);
            s.v[2 * CTR_MAX_NDIM + d] += x2 * x2;
            d2 = d == 0 ? x2 : d2 + x2;
            const int b = vanhove_bin(v.edges, x, lo, hi, v.inv_width, H);
            if (b >= 0) atomicAdd(&s_count[d * per_axis + b], 1u);
          }
        ++s.n;
        const int b = vanhove_bin_r(v.edge2, d2, hi2, v.inv_width, H);
        if (b >= 0) atomicAdd(&s_count[nd * per_axis + b], 1u);
      }
    vanhove_reduce(s, s_red, nd);              // its barrier: the counters are complete too
    if (tid == 0) {
      const long long at = c * v.K + q;
#pragma unroll
      for (int d = 0; d < CTR_MAX_NDIM; ++d)
        if (d < nd) {
          v.part[at * 3 * nd + d] = s.v[d];
          v.part[at * 3 * nd + nd + d] = s.v[CTR_MAX_NDIM + d];
          v.part[at * 3 * nd + 2 * nd + d] = s.v[2 * CTR_MAX_NDIM + d];
        }
      v.part_n[at] = s.n;
    }
    if (s.n == 0) continue;                    // the same in every thread: nothing was counted
    for (int j = tid; j < used; j += MSD_THREADS) {
      const unsigned cnt = s_count[j];
      if (cnt == 0) continue;
      unsigned long long* to;
      if (j < nd * per_axis) {
        const int d = j / per_axis, b = j % per_axis;
        to = b < B ? v.count + ((long long)q * nd + d) * B + b : (b == B ? v.below : v.above) + (long long)q * nd + d;
      } else {
        const int b = j - nd * per_axis;
        to = b < H ? v.count_r + (long long)q * H + b : v.above_r + q;
      }
      atomicAdd(to, (unsigned long long)cnt);
    }
  }
}

// One workgroup per lag index q: the partials of the chunks added in chunk order, each sum by one
// thread, as msd_pool_kernel adds them; the means and clause 9; then the densities of clause 10 from
// the finished counts, the threads side by side.  A refused table: NaN and n = 0 (the counts are 0).
__global__ void __launch_bounds__(MSD_THREADS) vanhove_finish_kernel(const VanhoveArgs v) {
#pragma clang fp contract(off)
  __shared__ double s_sum[VH_VALUES];
  __shared__ long long s_n;
  const MsdArgs& a = v.t;
  const bool ok = ld_agent(a.status) == CTR_VANHOVE_OK;
  const int tid = threadIdx.x, nd = a.ndim, H = v.H, B = 2 * H;
  const double nan = __builtin_nan("");
  for (int q = blockIdx.x; q < v.K; q += gridDim.x) {
    __syncthreads();                           // the lag before is done with LDS
    if (tid < 3 * nd) {
      double sum = 0.;
      for (long long c = 0; ok && c < a.n_chunks; ++c) sum += v.part[(c * v.K + q) * 3 * nd + tid];
      s_sum[tid] = sum;
    } else if (tid == 64) {
      long long n = 0;
      for (long long c = 0; ok && c < a.n_chunks; ++c) n += v.part_n[c * v.K + q];
      s_n = n;
    }
    __syncthreads();
    const long long n = s_n;
    if (tid < nd) {
      const double m1 = n > 0 ? s_sum[tid] / (double)n : nan;
      const double m2 = n > 0 ? s_sum[nd + tid] / (double)n : nan;
      const double m4 = n > 0 ? s_sum[2 * nd + tid] / (double)n : nan;
      v.mean_d[q * nd + tid] = m1;
      v.mean_d2[q * nd + tid] = m2;
      v.mean_d4[q * nd + tid] = m4;
      v.alpha2[q * nd + tid] = m4 / (3. * (m2 * m2)) - 1.;      // NaN from NaN
    }
    if (tid == 0) v.n[q] = n;
    const double per = (double)n * v.bin_width;
    for (int j = tid; j < nd * B; j += MSD_THREADS) {
      const long long at = (long long)q * nd * B + j;
      v.density[at] = n > 0 ? (double)v.count[at] / per : nan;
    }
    for (int j = tid; j < H; j += MSD_THREADS) {
      const long long at = (long long)q * H + j;
      v.density_r[at] = n > 0 ? (double)v.count_r[at] / per : nan;
    }
  }
}

#endif  // CTREFINE_VANHOVE_KERNELS_H
