// motion_ci_kernels.h -- bootstrap confidence interval of the diffusion tensor (ctr_diffusion_ci_device;
// DESIGN.md 7b).  Included by tu_motion_ci.hip inside its anonymous namespace, behind motion_kernels.h
// (mot_displ, MOT_TILE).
//
// The rule (include/ctrefine.h has it in full): per pair = (track, lag), or lag alone with pooled
// tracks, the rows x[n, D] of the diffusion tensor in the order (track,) permutation, frame;
// stat(x) = mean(x x^T) 0.5 fps / lag; B resamples with the counter-based indices ci_index; every
// entry sorted over the resamples; z0, the acceleration and the ranks of the BCa (or percentile)
// interval from them.
//
// Layout of the work, per chunk of pairs (the host's decision, tu_motion_ci.hip):
//   ci_rows_kernel: one workgroup per pair walks (track,) permutation, tile of MOT_TILE frames in the
//     order of the rule; lane = frame.  The valid rows of a tile are ranked by ballot and popcount
//     and written behind those of the tiles before: a stable compaction, rows[pair][k][D], and n.
//   ci_resample_kernel<D, LDS>: one workgroup per (pair, CI_THREADS resamples), lane = resample b.
//     LDS: the workgroup stages the n rows once and every lane gathers from them; otherwise the
//     lanes gather from the scratch in global memory (L2).  A lane adds the D(D+1)/2 products of
//     its rows k = 0 .. n-1 in that order into registers: no reduction across lanes, no atomics.
//     A row is D consecutive doubles (24 or 48 bytes): one or two cache lines per gather from L2;
//     in LDS the D reads of a lane start at the random bank 6k or 12k mod 64, so a wavefront's reads
//     conflict as 32 random addresses over 32 8-byte slots do (about 3.5 deep), whatever the layout.
//   ci_order_kernel: one workgroup per (pair, entry i <= j).  Sum of the products p_k = x_ki x_kj
//     (thread-strided, then a tree over the threads: a fixed order), ostat from it, then the sums of
//     (p_k - mean)^2 and ^3 the same way: the acceleration.  The B statistics of the entry are
//     sorted in LDS (bitonic, padded with +inf to a power of two); #{s_b < ostat} is the lower bound
//     of ostat in the sorted values.  z0, avals, ranks and the interval follow, written to (i, j) and
//     (j, i).
// Nothing depends on which other pairs a chunk or a call holds: a pair gives the same bytes alone,
// in a batch, in a sweep and in any chunking.
#ifndef CTREFINE_MOTION_CI_KERNELS_H
#define CTREFINE_MOTION_CI_KERNELS_H

constexpr int CI_THREADS = 512;        // resamples per workgroup, and threads of the order kernel
constexpr int CI_MAX_ALPHA = 8;

struct CiArgs {
  int ndim, n_perm, n_alpha, method, pool;
  long long T, F, n_lags;
  long long n_max;            // rows a pair can have: P F, or T P F pooled (the stride of `rows`)
  long long B, B2;            // resamples, and the next power of two (the sort)
  long long pair0;            // first pair of this chunk
  unsigned long long seed_mix;      // mix64(seed)
  double fps;
  double z_alpha[CI_MAX_ALPHA], alphas[CI_MAX_ALPHA];
  const long long* lags;
  const double* positions;
  const double* bases;
  // scratch of the chunk
  double* rows;               // [pair][n_max][D]
  double* stats;              // [pair][D (D + 1) / 2][B]
  long long* n;               // [pair]
  // outputs, indexed by the pair of the call; all but interval may be null
  double* interval;           // [pair][n_alpha][D][D]
  double* tensor;             // [pair][D][D]
  long long* n_rows;          // [pair]
  double* z0;                 // [pair][D][D]
  double* accel;              // [pair][D][D]
  long long* ranks;           // [pair][n_alpha][D][D]
};

// index k of resample b among n rows: depends on (seed, b, k, n) alone
__device__ __forceinline__ long long ci_index(unsigned long long seed_mix, unsigned long long b, unsigned long long k,
                                              unsigned long long n) {
  const unsigned long long r = mix64(seed_mix + ((b << 32) + k + 1ull) * 0x9E3779B97F4A7C15ull);
  return (long long)__umul64hi(r, n);
}

// mean and scale of a sum of n products, the expression of diffusion_final_kernel
__device__ __forceinline__ double ci_scale(double s, double n, double dt) { return s / n * 0.5 / dt; }

__device__ __forceinline__ void ci_pair(const CiArgs& a, long long pair, long long& t0, long long& t1, long long& li) {
  if (a.pool) { t0 = 0; t1 = a.T; li = pair; }
  else { t0 = pair / a.n_lags; t1 = t0 + 1; li = pair - t0 * a.n_lags; }
}

__global__ __launch_bounds__(MOT_THREADS) void ci_rows_kernel(CiArgs a) {
  __shared__ int wave_n[MOT_THREADS / WAVE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const long long local = blockIdx.x;
  long long t0, t1, li;
  ci_pair(a, a.pair0 + local, t0, t1, li);
  const long long lag = a.lags[li];
  const int D = a.ndim == 2 ? 3 : 6;
  double* dst = a.rows + local * a.n_max * D;
  long long base = 0;                                  // rows written by the tiles before
  if (lag >= 1 && lag < a.F) {
    const long long last = a.F - lag;                  // frames b < last have a later frame
    for (long long t = t0; t < t1; ++t)
      for (long long p = 0; p < a.n_perm; ++p) {
        const double* gb = a.bases + (t * a.n_perm + p) * a.F * 9;
        const double* gp = a.positions + t * a.F * 3;
        for (long long b0 = 0; b0 < last; b0 += MOT_TILE) {
          const long long b = b0 + tid;
          bool ok = b < last;
          double x[6] = {0., 0., 0., 0., 0., 0.};
          if (ok) {
            double Bm[9], q[3], C[9], r[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) { Bm[k] = gb[b * 9 + k]; C[k] = gb[(b + lag) * 9 + k]; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { q[k] = gp[b * 3 + k]; r[k] = gp[(b + lag) * 3 + k]; }
            mot_displ(Bm, q, C, r, x);
#pragma unroll
            for (int k = 0; k < 6; ++k) ok = ok && isfinite(x[k]);
          }
          const unsigned long long m = __ballot(ok);
          if (lane == 0) wave_n[wave] = __popcll(m);
          __syncthreads();
          long long at = base;
          int total = 0;
#pragma unroll
          for (int w = 0; w < MOT_THREADS / WAVE; ++w) {
            if (w < wave) at += wave_n[w];
            total += wave_n[w];
          }
          if (ok) {
            at += __popcll(m & ((1ull << lane) - 1ull));
            double* o = dst + at * D;
            if (a.ndim == 2) { o[0] = x[0]; o[1] = x[1]; o[2] = x[5]; }      // x, y translation and z rotation
            else {
#pragma unroll
              for (int k = 0; k < 6; ++k) o[k] = x[k];
            }
          }
          base += total;
          __syncthreads();
        }
      }
  }
  if (tid == 0) a.n[local] = base;
}

template <int D, bool LDS>
__global__ __launch_bounds__(CI_THREADS) void ci_resample_kernel(CiArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ci_lds[];
  constexpr int NE = D * (D + 1) / 2;
  const int tid = threadIdx.x;
  const long long per_pair = (a.B + CI_THREADS - 1) / CI_THREADS;
  const long long local = blockIdx.x / per_pair, blk = blockIdx.x - local * per_pair;
  const long long n = a.n[local];
  if (n == 0) return;                                  // the whole workgroup: the order kernel writes NaN
  const double* rows = a.rows + local * a.n_max * D;
  if (LDS) {
    for (long long e = tid; e < n * D; e += CI_THREADS) ci_lds[e] = rows[e];
    __syncthreads();
    rows = ci_lds;
  }
  const long long b = blk * CI_THREADS + tid;
  if (b >= a.B) return;
  double acc[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) acc[e] = 0.;
#pragma unroll 4
  for (long long k = 0; k < n; ++k) {
    const double* xr = rows + ci_index(a.seed_mix, (unsigned long long)b, (unsigned long long)k, (unsigned long long)n) * D;
    double x[D];
    if constexpr (D == 6) {                            // 48-byte rows on a 16-byte boundary
      const double2* x2 = (const double2*)xr;
      const double2 u = x2[0], v = x2[1], w = x2[2];
      x[0] = u.x; x[1] = u.y; x[2] = v.x; x[3] = v.y; x[4] = w.x; x[5] = w.y;
    } else {
#pragma unroll
      for (int c = 0; c < D; ++c) x[c] = xr[c];
    }
    int e = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j) { acc[e] = acc[e] + x[i] * x[j]; ++e; }
  }
  long long t0, t1, li;
  ci_pair(a, a.pair0 + local, t0, t1, li);
  const double dt = (double)a.lags[li] / a.fps, nn = (double)n;
  double* out = a.stats + local * NE * a.B + b;
#pragma unroll
  for (int e = 0; e < NE; ++e) out[e * a.B] = ci_scale(acc[e], nn, dt);
}

// sum over the workgroup in a fixed order: the threads' values by a tree in LDS; every thread gets it
__device__ __forceinline__ double ci_block_sum(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  for (int s = CI_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(CI_THREADS) void ci_order_kernel(CiArgs a) {
  extern __shared__ __attribute__((aligned(16))) double ci_lds[];                   // [B2]: the statistics of the entry
  __shared__ double red[CI_THREADS];
  const int tid = threadIdx.x;
  const int D = a.ndim == 2 ? 3 : 6, NE = D * (D + 1) / 2;
  const long long local = blockIdx.x / NE;
  const int e = (int)(blockIdx.x - local * NE);
  int i = 0, rest = e;
  while (rest >= D - i) { rest -= D - i; ++i; }        // e = i D - i (i - 1) / 2 + (j - i)
  const int j = i + rest;
  const long long pair = a.pair0 + local;
  const long long n = a.n[local];
  const int K = a.n_alpha;
  const int ij = i * D + j, ji = j * D + i;
  if (n == 0) {
    if (tid == 0) {
      for (int q = 0; q < K; ++q) {
        a.interval[(pair * K + q) * D * D + ij] = NAN;
        a.interval[(pair * K + q) * D * D + ji] = NAN;
        if (a.ranks) { a.ranks[(pair * K + q) * D * D + ij] = 0; a.ranks[(pair * K + q) * D * D + ji] = 0; }
      }
      if (a.tensor) { a.tensor[pair * D * D + ij] = NAN; a.tensor[pair * D * D + ji] = NAN; }
      if (a.z0) { a.z0[pair * D * D + ij] = NAN; a.z0[pair * D * D + ji] = NAN; }
      if (a.accel) { a.accel[pair * D * D + ij] = NAN; a.accel[pair * D * D + ji] = NAN; }
      if (a.n_rows && e == 0) a.n_rows[pair] = 0;
    }
    return;
  }
  const double* rows = a.rows + local * a.n_max * D;
  double s1 = 0.;
  for (long long k = tid; k < n; k += CI_THREADS) s1 = s1 + rows[k * D + i] * rows[k * D + j];
  s1 = ci_block_sum(s1, red, tid);
  const double nn = (double)n;
  const double mean = s1 / nn;
  double s2 = 0., s3 = 0.;
  for (long long k = tid; k < n; k += CI_THREADS) {
    const double d = rows[k * D + i] * rows[k * D + j] - mean;
    const double dd = d * d;
    s2 = s2 + dd;
    s3 = s3 + dd * d;
  }
  s2 = ci_block_sum(s2, red, tid);
  s3 = ci_block_sum(s3, red, tid);
  // the sort
  const double* st = a.stats + (local * NE + e) * a.B;
  for (long long m = tid; m < a.B2; m += CI_THREADS) ci_lds[m] = m < a.B ? st[m] : INFINITY;
  __syncthreads();
  for (long long size = 2; size <= a.B2; size <<= 1)
    for (long long stride = size >> 1; stride > 0; stride >>= 1) {
      for (long long m = tid; m < (a.B2 >> 1); m += CI_THREADS) {
        const long long lo = 2 * m - (m & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const double u = ci_lds[lo], v = ci_lds[hi];
        if ((u > v) == up) { ci_lds[lo] = v; ci_lds[hi] = u; }
      }
      __syncthreads();
    }
  if (tid != 0) return;
  long long t0, t1, li;
  ci_pair(a, pair, t0, t1, li);
  const double dt = (double)a.lags[li] / a.fps;
  const double ostat = ci_scale(s1, nn, dt);
  long long lo = 0, hi = a.B;                          // #{s_b < ostat}
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (ci_lds[mid] < ostat) lo = mid + 1; else hi = mid;
  }
  const double z0 = lo == 0 ? -INFINITY : lo == a.B ? INFINITY : normcdfinv((double)lo / (double)a.B);
  const double acc = s3 / (6. * pow(s2, 1.5));
  for (int q = 0; q < K; ++q) {
    double av = a.alphas[q];
    if (a.method == CTR_CI_BCA) {
      const double zs = z0 + a.z_alpha[q];
      av = normcdf(z0 + zs / (1. - acc * zs));
    }
    const double rk = rint((double)(a.B - 1) * av);
    long long rank = rk == rk ? (long long)rk : 0;     // nan_to_num
    rank = rank < 0 ? 0 : rank > a.B - 1 ? a.B - 1 : rank;
    const double v = ci_lds[rank];
    a.interval[(pair * K + q) * D * D + ij] = v;
    a.interval[(pair * K + q) * D * D + ji] = v;
    if (a.ranks) { a.ranks[(pair * K + q) * D * D + ij] = rank; a.ranks[(pair * K + q) * D * D + ji] = rank; }
  }
  if (a.tensor) { a.tensor[pair * D * D + ij] = ostat; a.tensor[pair * D * D + ji] = ostat; }
  if (a.z0) { a.z0[pair * D * D + ij] = z0; a.z0[pair * D * D + ji] = z0; }
  if (a.accel) { a.accel[pair * D * D + ij] = acc; a.accel[pair * D * D + ji] = acc; }
  if (a.n_rows && e == 0) a.n_rows[pair] = n;
}

#endif  // CTREFINE_MOTION_CI_KERNELS_H
