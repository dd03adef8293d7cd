// msd_kernels.h -- mean squared displacement of linked particles: the sorted rows of a table, the
// moments of every particle and of the ensemble against lag (ctr_msd_device, ctr_emsd_device;
// include/ctrefine.h has the rule).  Included by tu_msd.hip inside its anonymous
// namespace, after stage_common.h.  The kernel boundary is the only synchronisation between
// workgroups; every loop is bounded by the launch's arguments or by row ranges that msd_rows_kernel
// wrote from a table msd_check_kernel has passed; integer atomics in LDS only: every float sum is
// taken in an order that the input alone decides.
#ifndef CTREFINE_MSD_KERNELS_H
#define CTREFINE_MSD_KERNELS_H

constexpr int MSD_THREADS = 256;            // a workgroup of every kernel here: 4 wavefronts
constexpr int MSD_WAVES = MSD_THREADS / 64;
constexpr int MSD_TILE = CTR_MSD_TILE;      // frames of a span dense in LDS
constexpr int MSD_CHUNK = CTR_MSD_CHUNK;    // ids per partial of the ensemble
constexpr int MSD_VALUES = 2 * CTR_MAX_NDIM;   // sums of a lag: d and d^2 per coordinate
constexpr long long MSD_FILL = 2048;        // workgroups of msd_chunk_kernel that fill the device: 256 CUs, 8 of them on each

struct MsdArgs {
  int ndim;
  long long L, T, N, P, M;
  double mpp[CTR_MAX_NDIM];
  const long long* frame_offset;
  const long long* particle;
  const long long* order;
  const long long* select;
  const double* pos;
  // scratch, in sorted row order
  int* code;                 // [N] the frame of the row, or -(g + 2) < 0 for a row that does not exist (g: its frame, -1 or T for none)
  int* key;                  // [N] the id, -1 for an unlinked row
  double* spos;              // [N, ndim]
  int* first;                // [P] the sorted rows [first, last) of an id; 0, 0 without rows
  int* last;                 // [P]
  double* part;              // [chunks, L, 2 ndim] sums of the ensemble's chunks
  long long* part_n;         // [chunks, L]
  long long n_chunks;
  long long lag_groups;       // G: the workgroups that share the lags of a chunk (a launch decision: the bytes do not depend on it)
  // out
  double* msd;
  double* mean_d;
  double* mean_d2;
  int* n;                    // per particle
  long long* n_pool;         // ensemble
  int* status;
};

__device__ __forceinline__ long long msd_key(long long p) { return p < 0 ? -1 : p; }
// the frame a code stands for, whether its row exists or not: it never falls along the rows of an id
__device__ __forceinline__ int msd_raw(int code) { return code >= 0 ? code : -code - 2; }

// The caller's tables, before any kernel follows an index: offsets monotone within [0, N], particle
// < P, order a stable ascending sort by particle.  status[0] was zeroed in front of this kernel.
__global__ void __launch_bounds__(MSD_THREADS) msd_check_kernel(const MsdArgs a) {
  const long long stride = (long long)gridDim.x * MSD_THREADS;
  const long long n = a.T + 1 > a.N ? a.T + 1 : a.N;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * MSD_THREADS + threadIdx.x; i < n; i += stride) {
    if (i <= a.T) bad |= offsets_bad(a.frame_offset, i, a.T, a.N);
    if (i < a.N) {
      bad |= a.particle[i] >= a.P;
      const long long r = a.order[i];
      if (r < 0 || r >= a.N) { bad = true; continue; }
      if (i + 1 < a.N) {
        const long long r1 = a.order[i + 1];
        if (r1 < 0 || r1 >= a.N) { bad = true; continue; }
        const long long k = msd_key(a.particle[r]), k1 = msd_key(a.particle[r1]);
        bad |= k1 < k || (k1 == k && k >= 0 && r1 <= r);
      }
    }
  }
  if (bad) st_agent(a.status, CTR_MSD_BAD_TABLE);
}

// the frame of row r (the last t with frame_offset[t] <= r), -1 before the first frame, T from
// frame_offset[T] on
__device__ __forceinline__ long long msd_frame_of(const MsdArgs& a, long long r) {
  if (a.T <= 0 || r < a.frame_offset[0]) return -1;
  if (r >= a.frame_offset[a.T]) return a.T;
  long long lo = 0, hi = a.T;
  while (hi - lo > 1) {
    const long long mid = (lo + hi) / 2;
    if (a.frame_offset[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One thread per sorted row i: code, key, spos, and first / last of an id where the id changes
// (both were zeroed in front of this kernel).  A row exists when its id is >= 0, it lies in a frame
// and the sorted row before it is not of the same id and frame (clause 1: the lowest row).
__global__ void __launch_bounds__(MSD_THREADS) msd_rows_kernel(const MsdArgs a) {
  if (ld_agent(a.status) != CTR_MSD_OK) return;
  const long long stride = (long long)gridDim.x * MSD_THREADS;
  const int nd = a.ndim;
  for (long long i = (long long)blockIdx.x * MSD_THREADS + threadIdx.x; i < a.N; i += stride) {
    const long long r = a.order[i];
    const long long p = msd_key(a.particle[r]);
    const long long g = msd_frame_of(a, r);
    bool exists = p >= 0 && g >= 0 && g < a.T;
    const long long p_before = i > 0 ? msd_key(a.particle[a.order[i - 1]]) : -2;
    const long long p_after = i + 1 < a.N ? msd_key(a.particle[a.order[i + 1]]) : -2;
    if (exists && p_before == p && msd_frame_of(a, a.order[i - 1]) == g) exists = false;
    a.code[i] = exists ? (int)g : (int)(-(g + 2));       // g <= T <= 2^31 - 3
    a.key[i] = (int)p;
    for (int d = 0; d < nd; ++d) a.spos[i * nd + d] = a.pos[r * nd + d];
    if (p >= 0) {
      if (p_before != p) a.first[p] = (int)i;
      if (p_after != p) a.last[p] = (int)(i + 1);
    }
  }
}

// The sorted row of the same id as row i (an existing row of frame f) in frame f + k, among the
// rows (i, e) of that id, or -1.  Without a gap or a repeated row in between it is row i + k; else
// the first row whose frame is not below f + k, by bisection: the lowest row of a frame exists.
__device__ __forceinline__ long long msd_partner(const int* code, long long i, long long e, int f, long long k, long long T) {
  const long long target = (long long)f + k;
  if (target >= T || i + 1 >= e || msd_raw(code[e - 1]) < target) return -1;
  if (i + k < e && code[i + k] == target) return i + k;
  long long lo = i + 1, hi = e;          // the first row in [lo, hi) with raw >= target; raw(code[e - 1]) >= target
  while (lo < hi) {
    const long long mid = (lo + hi) / 2;
    if (msd_raw(code[mid]) < target) lo = mid + 1;
    else hi = mid;
  }
  return code[lo] == target ? lo : -1;
}

// what a thread has added for one lag
struct MsdSums {
  double v[MSD_VALUES];      // d per coordinate, then d^2 per coordinate
  long long n;
};

__device__ __forceinline__ void msd_add(MsdSums& s, const double* from, const double* to, const double* mpp, int nd) {
#pragma unroll
  for (int d = 0; d < CTR_MAX_NDIM; ++d)
    if (d < nd) {
      const double x = (to[d] - from[d]) * mpp[d];
      s.v[d] += x;
      s.v[CTR_MAX_NDIM + d] += __dmul_rn(x, x);      // the square rounded, then added: no contraction
    }
  ++s.n;
}

// The terms of lag k of the sorted rows [r0, r1), thread t taking rows r0 + t, r0 + t + 256, ...
// in that order; `e` of a row is the end of its id's rows: `last[key]`, or r1 where the rows are of one id.
__device__ __forceinline__ void msd_lag_of_rows(const MsdArgs& a, long long r0, long long r1, bool one_id, long long k, MsdSums& s) {
  const int nd = a.ndim;
  for (long long i = r0 + threadIdx.x; i < r1; i += MSD_THREADS) {
    const int f = a.code[i];
    if (f < 0) continue;
    const long long e = one_id ? r1 : (long long)a.last[a.key[i]];
    const long long j = msd_partner(a.code, i, e, f, k, a.T);
    if (j >= 0) msd_add(s, a.spos + i * nd, a.spos + j * nd, a.mpp, nd);
  }
}

// The workgroup's sum of every thread's sums, in every thread: a tree of shuffles in the wavefront,
// lane l taking lane l + 32, + 16, ..., + 1, then the wavefronts' sums ((0 + 1) + (2 + 3)) through
// s_red[parity]: one barrier, and the calls of consecutive lags alternate the parity.
struct MsdRed {
  double v[2][MSD_WAVES][MSD_VALUES];
  long long n[2][MSD_WAVES];
};

__device__ __forceinline__ void msd_reduce(MsdSums& s, MsdRed& red, int parity, int nd) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
#pragma unroll
    for (int d = 0; d < CTR_MAX_NDIM; ++d)
      if (d < nd) {
        s.v[d] += __shfl_down(s.v[d], w);
        s.v[CTR_MAX_NDIM + d] += __shfl_down(s.v[CTR_MAX_NDIM + d], w);
      }
    s.n += __shfl_down(s.n, w);
  }
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < MSD_VALUES; ++d) red.v[parity][wave][d] = s.v[d];
    red.n[parity][wave] = s.n;
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < MSD_VALUES; ++d)
    s.v[d] = (red.v[parity][0][d] + red.v[parity][1][d]) + (red.v[parity][2][d] + red.v[parity][3][d]);
  s.n = (red.n[parity][0] + red.n[parity][1]) + (red.n[parity][2] + red.n[parity][3]);
}

// clauses 5 to 7 and 9 from the sums of a lag, written by one thread
__device__ __forceinline__ void msd_write(const MsdSums& s, int nd, double* msd, double* mean_d, double* mean_d2) {
  const double nan = __builtin_nan("");
  double total = 0.;
#pragma unroll
  for (int d = 0; d < CTR_MAX_NDIM; ++d)       // constant indices: the sums stay in registers
    if (d < nd) {
      const double m1 = s.n > 0 ? s.v[d] / (double)s.n : nan;
      const double m2 = s.n > 0 ? s.v[CTR_MAX_NDIM + d] / (double)s.n : nan;
      mean_d[d] = m1;
      mean_d2[d] = m2;
      total = d == 0 ? m2 : total + m2;
    }
  *msd = total;
}

// One workgroup per reported id m (striding past the grid): the moments of its track at the lags
// 1 .. L.  A span of at most MSD_TILE frames is dense in LDS by frame; a longer one is read from the
// sorted rows.  Lags beyond the span, an id without rows and a refused table: NaN and 0.
__global__ void __launch_bounds__(MSD_THREADS) msd_particle_kernel(const MsdArgs a) {
  __shared__ double s_x[CTR_MAX_NDIM][MSD_TILE];
  __shared__ unsigned char s_has[MSD_TILE];
  __shared__ MsdRed s_red;
  __shared__ int s_lo, s_hi;
  const bool ok = ld_agent(a.status) == CTR_MSD_OK;
  const int tid = threadIdx.x, nd = a.ndim;
  for (long long m = blockIdx.x; m < a.M; m += gridDim.x) {
    const long long p = a.select ? a.select[m] : m;
    const bool known = ok && p >= 0 && p < a.P;
    const long long r0 = known ? a.first[p] : 0, r1 = known ? a.last[p] : 0;
    __syncthreads();                           // the id before is done with LDS
    if (tid == 0) { s_lo = 0x7fffffff; s_hi = -1; }
    __syncthreads();
    int lo = 0x7fffffff, hi = -1;
    for (long long i = r0 + tid; i < r1; i += MSD_THREADS) {
      const int f = a.code[i];
      if (f >= 0) { lo = f < lo ? f : lo; hi = f > hi ? f : hi; }
    }
    if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __syncthreads();
    const long long f0 = s_lo, span = s_hi >= 0 ? (long long)s_hi - f0 + 1 : 0;
    const long long kmax = span - 1 < a.L ? (span > 0 ? span - 1 : 0) : a.L;     // lags with a chance of a pair
    const bool dense = span <= MSD_TILE;
    if (dense && kmax > 0) {
      for (int f = tid; f < span; f += MSD_THREADS) s_has[f] = 0;
      __syncthreads();
      for (long long i = r0 + tid; i < r1; i += MSD_THREADS) {
        const int f = a.code[i];
        if (f < 0) continue;
        const int at = (int)(f - f0);          // < span <= MSD_TILE; an existing row is alone in its frame
        s_has[at] = 1;
        for (int d = 0; d < nd; ++d) s_x[d][at] = a.spos[i * nd + d];
      }
      __syncthreads();
    }
    for (long long k = 1; k <= kmax; ++k) {
      MsdSums s = {};
      if (dense) {
        for (long long f = tid; f + k < span; f += MSD_THREADS)
          if (s_has[f] && s_has[f + k]) {
            double from[CTR_MAX_NDIM], to[CTR_MAX_NDIM];
#pragma unroll
            for (int d = 0; d < CTR_MAX_NDIM; ++d)
              if (d < nd) { from[d] = s_x[d][f]; to[d] = s_x[d][f + k]; }
            msd_add(s, from, to, a.mpp, nd);
          }
      } else {
        msd_lag_of_rows(a, r0, r1, true, k, s);
      }
      msd_reduce(s, s_red, (int)(k & 1), nd);
      if (tid == 0) {
        const long long at = m * a.L + (k - 1);
        msd_write(s, nd, a.msd + at, a.mean_d + at * nd, a.mean_d2 + at * nd);
        a.n[at] = (int)s.n;                    // at most the rows of the track < 2^31
      }
    }
    for (long long k = kmax + 1 + tid; k <= a.L; k += MSD_THREADS) {
      const long long at = m * a.L + (k - 1);
      a.msd[at] = __builtin_nan("");
      for (int d = 0; d < nd; ++d) a.mean_d[at * nd + d] = a.mean_d2[at * nd + d] = __builtin_nan("");
      a.n[at] = 0;
    }
  }
}

// One workgroup per chunk c of MSD_CHUNK consecutive ids and group g of lags (striding past the
// grid): the sums and the count of the lags g + 1, g + 1 + G, ... over the pairs of the chunk's ids,
// whose rows are the sorted rows [r0, r1).  The G = lag_groups workgroups of a chunk share its lags
// so that a table of few ids still fills the device; a lag is summed by one workgroup whatever G
// is, so the bytes do not depend on it.  Lags beyond the longest span in the chunk get zeros without
// a reduction.
__global__ void __launch_bounds__(MSD_THREADS) msd_chunk_kernel(const MsdArgs a) {
  __shared__ MsdRed s_red;
  __shared__ int s_lo, s_hi, s_span;
  if (ld_agent(a.status) != CTR_MSD_OK) return;
  const int tid = threadIdx.x, nd = a.ndim;
  const long long G = a.lag_groups;
  int parity = 0;
  for (long long w = blockIdx.x; w < a.n_chunks * G; w += gridDim.x) {
    const long long c = w / G, g = w % G;
    __syncthreads();
    if (tid == 0) { s_lo = 0x7fffffff; s_hi = 0; s_span = 0; }
    __syncthreads();
    const long long p_end = (c + 1) * MSD_CHUNK < a.P ? (c + 1) * MSD_CHUNK : a.P;
    for (long long p = c * MSD_CHUNK + tid; p < p_end; p += MSD_THREADS) {
      const int b = a.first[p], e = a.last[p];
      if (e > b) {
        atomicMin(&s_lo, b);
        atomicMax(&s_hi, e);
        atomicMax(&s_span, msd_raw(a.code[e - 1]) - msd_raw(a.code[b]));      // no less than the span - 1 of its existing rows
      }
    }
    __syncthreads();
    const long long r0 = s_lo < s_hi ? s_lo : 0, r1 = s_lo < s_hi ? s_hi : 0;
    const long long kmax = s_span < a.L ? s_span : a.L;
    for (long long k = g + 1; k <= kmax; k += G) {
      MsdSums s = {};
      msd_lag_of_rows(a, r0, r1, false, k, s);
      msd_reduce(s, s_red, parity, nd);
      parity ^= 1;
      if (tid == 0) {
        const long long at = c * a.L + (k - 1);
#pragma unroll
        for (int d = 0; d < CTR_MAX_NDIM; ++d)
          if (d < nd) {
            a.part[at * 2 * nd + d] = s.v[d];
            a.part[at * 2 * nd + nd + d] = s.v[CTR_MAX_NDIM + d];
          }
        a.part_n[at] = s.n;
      }
    }
    // this group's lags beyond kmax: the first is the smallest k > kmax with k - 1 = g (mod G)
    const long long k_first = kmax < g + 1 ? g + 1 : g + 1 + (kmax - g - 1 + G) / G * G;
    for (long long k = k_first + (long long)tid * G; k <= a.L; k += (long long)MSD_THREADS * G) {
      const long long at = c * a.L + (k - 1);
      for (int d = 0; d < 2 * nd; ++d) a.part[at * 2 * nd + d] = 0.;
      a.part_n[at] = 0;
    }
  }
}

// One thread per lag: the partials of the chunks added in chunk order, then clauses 5 to 7 and 9.
// A refused table: NaN and 0.
__global__ void __launch_bounds__(MSD_THREADS) msd_pool_kernel(const MsdArgs a) {
  const bool ok = ld_agent(a.status) == CTR_MSD_OK;
  const long long stride = (long long)gridDim.x * MSD_THREADS;
  const int nd = a.ndim;
  for (long long l = (long long)blockIdx.x * MSD_THREADS + threadIdx.x; l < a.L; l += stride) {
    MsdSums s = {};
    for (long long c = 0; ok && c < a.n_chunks; ++c) {
      const long long at = c * a.L + l;
#pragma unroll
      for (int d = 0; d < CTR_MAX_NDIM; ++d)
        if (d < nd) {
          s.v[d] += a.part[at * 2 * nd + d];
          s.v[CTR_MAX_NDIM + d] += a.part[at * 2 * nd + nd + d];
        }
      s.n += a.part_n[at];
    }
    msd_write(s, nd, a.msd + l, a.mean_d + l * nd, a.mean_d2 + l * nd);
    a.n_pool[l] = s.n;
  }
}

#endif  // CTREFINE_MSD_KERNELS_H
