// residual_kernels.h -- model and residual frames of a fitted table, and the goodness-of-fit sums per
// feature and per cluster (ctr_residual_device; the rule is in include/ctrefine.h).
// Included inside the anonymous namespace of tu_residual.hip, after device_common.h and
// stage_common.h.  The unit is compiled without floating-point contraction.
//   resid_check_kernel    the caller's frame_offset, before an index is followed
//   resid_frame_kernel    a workgroup per tile of pixels of one frame: the rows of the frame in chunks
//                         through LDS, compacted to those whose box meets the tile
//   resid_feature_kernel  a wavefront per row: the sums over its clipped box
//   resid_cluster_kernel  a thread per row: the sums of its cluster, in ascending row order
// Every kernel strides over its items and leaves at once where status is not CTR_RESID_OK.
#ifndef CTREFINE_RESIDUAL_KERNELS_H
#define CTREFINE_RESIDUAL_KERNELS_H

constexpr int RESID_THREADS = 256;
constexpr int RESID_CHUNK = CTR_RESID_CHUNK;   // rows staged at once: one per thread
// a staged row: the mask centre [3], background, signal, position [3], 1 / size^2 [3], profile parameters [INV_NX]
constexpr int RESID_CEN = 0, RESID_BG = 3, RESID_SIG = 4, RESID_POS = 5, RESID_INV = 8, RESID_EX = 11;
constexpr int RESID_ROWD = RESID_EX + INV_NX;
static_assert(RESID_CHUNK == RESID_THREADS, "a thread stages one row of a chunk");

struct ResidArgs {
  int shape[3], radius[3];      // axis a of ndim at index a; 1 and 0 beyond
  int tile[3], ntile[3];        // pixels of a tile and tiles of a frame per axis
  int nx, n_params, outside, dtype;
  long long T, N, E;            // frames, rows, pixels of a frame
  long long tiles_per_frame, n_items;
  const void* frames;
  const long long* frame_offset;
  const double* params;
  const double* mask_pos;       // null: the positions in params
  const long long* cluster;
  const double* fmax;           // [T] the frame maxima (cluster pass)
  double* residual;             // never null: the caller's block or scratch
  double* model;                // may be null
  int* coverage;                // may be null
  int* owner;                   // never null
  long long *n_pix, *n_own, *n_nan;
  double *sum, *sum_sq, *own_sum_sq, *max_abs, *rms;
  long long* cluster_n_pix;
  double *cluster_sum_sq, *cost;
  int* status;
};

__global__ void __launch_bounds__(RESID_THREADS) resid_check_kernel(const ResidArgs a) {
  const long long stride = (long long)gridDim.x * RESID_THREADS;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * RESID_THREADS + threadIdx.x; i <= a.T; i += stride)
    bad |= offsets_bad(a.frame_offset, i, a.T, a.N) || (i == 0 && a.frame_offset[0] != 0) ||
           (i == a.T && a.frame_offset[i] != a.N);
  if (bad) st_agent(a.status, CTR_RESID_BAD_TABLE);
}

// the centre of the mask of row i
template <int ND>
__device__ __forceinline__ void resid_centre(const ResidArgs& a, long long i, double (&c)[ND]) {
#pragma unroll
  for (int d = 0; d < ND; ++d) c[d] = a.mask_pos ? a.mask_pos[i * ND + d] : a.params[i * a.n_params + 2 + d];
}

// The clipped box of a mask along one axis, one pixel wider on either side than centre -/+ radius so
// that no rounding of the covering test can fall outside it: [lo, hi] in doubles, empty (lo > hi or
// a NaN) for a centre that is not finite or too far outside.
__device__ __forceinline__ void resid_box(double c, int radius, int extent, double& lo, double& hi) {
  lo = fmax(c - (double)radius - 1., 0.);
  hi = fmin(c + (double)radius + 1., (double)(extent - 1));
  if (!(c - c == 0.)) { lo = 1.; hi = 0.; }
}

template <int FIT, int ND, bool ISO>
__global__ void __launch_bounds__(RESID_THREADS) resid_frame_kernel(const ResidArgs a) {
  __shared__ double s_row[RESID_CHUNK * RESID_ROWD];
  __shared__ int s_idx[RESID_CHUNK];
  if (ld_agent(a.status) != CTR_RESID_OK) return;
  const int tid = threadIdx.x;
  int radius[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) radius[d] = a.radius[d];
  for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
    const long long t = item / a.tiles_per_frame;
    long long rem = item - t * a.tiles_per_frame;
    int t0[ND], t1[ND], idx[ND];
    int l = tid;
    bool inside = true;
    long long pix = 0;
#pragma unroll
    for (int d = ND - 1; d >= 0; --d) {
      t0[d] = (int)(rem % a.ntile[d]) * a.tile[d];
      rem /= a.ntile[d];
      t1[d] = t0[d] + a.tile[d] < a.shape[d] ? t0[d] + a.tile[d] - 1 : a.shape[d] - 1;
      idx[d] = t0[d] + l % a.tile[d];
      l /= a.tile[d];
      inside = inside && idx[d] < a.shape[d];
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) pix = pix * a.shape[d] + idx[d];
    pix += t * a.E;
    const double image = inside ? load_pixel(a.frames, a.dtype, (size_t)pix) : 0.;
    const long long r0 = a.frame_offset[t], r1 = a.frame_offset[t + 1];
    int cov = 0, own = -1;
    double res = 0., s = 0., bg = 0.;
    for (long long c0 = r0; c0 < r1; c0 += RESID_CHUNK) {
      const long long i = c0 + tid;
      bool meets = i < r1;
      double cen[ND];
      if (meets) {
        resid_centre<ND>(a, i, cen);
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          double lo, hi;
          resid_box(cen[d], radius[d], a.shape[d], lo, hi);
          meets = meets && lo <= hi && lo <= (double)t1[d] && hi >= (double)t0[d];
        }
      }
      int total;
      const int at = workgroup_scan<RESID_THREADS, int>(meets ? 1 : 0, total);   // (its barriers: the chunk before is read)
      if (meets) {
        double* R = s_row + at * RESID_ROWD;
        const double* p = a.params + i * a.n_params;
        R[RESID_BG] = p[0];
        R[RESID_SIG] = p[1];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          R[RESID_CEN + d] = cen[d];
          R[RESID_POS + d] = p[2 + d];
          const double sz = p[2 + ND + (ISO ? 0 : d)];
          R[RESID_INV + d] = 1. / (sz * sz);
        }
        if (FIT != CTR_FIT_GAUSS)
          for (int k = 0; k < INV_NX; ++k) R[RESID_EX + k] = k < a.nx ? p[2 + ND + (ISO ? 1 : ND) + k] : 0.;
        s_idx[at] = (int)i;
      }
      __syncthreads();
      if (inside) {
        for (int k = 0; k < total; ++k) {
          const double* R = s_row + k * RESID_ROWD;
          double cen_k[ND];
#pragma unroll
          for (int d = 0; d < ND; ++d) cen_k[d] = R[RESID_CEN + d];
          if (!in_mask_exact<ND>(idx, cen_k, radius)) continue;
          if (cov == 0) {
            own = s_idx[k];
            bg = R[RESID_BG];
            res = image - bg;
          }
          ++cov;
          double r2 = 0., dd[ND];
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            dd[d] = (double)idx[d] - R[RESID_POS + d];
            r2 = r2 + (dd[d] * dd[d]) * R[RESID_INV + d];
          }
          double g, dg;
          if constexpr (FIT == CTR_FIT_GAUSS) {
            g = exp(-0.5 * ND * r2);
          } else if constexpr (FIT == CTR_FIT_INV_SERIES) {
            double ex[INV_NX], dge[INV_NX];
#pragma unroll
            for (int e = 0; e < INV_NX; ++e) ex[e] = R[RESID_EX + e];
            profile_inv_dev(a.nx, r2, ex, g, dg, dge);
          } else {
            double dge, q = 0.;
            const double e = R[RESID_EX];
#pragma unroll
            for (int d = ND - 1; d >= 0; --d) q = q + dd[d] * dd[d];
            profile_dev<FIT, ND>(r2, e, g, dg, dge);
            if (q < 1.) g = (FIT == CTR_FIT_DISC && e > 0.) ? 1. : NAN;   // r2_*_safe
          }
          const double term = R[RESID_SIG] * g;
          res = res - term;
          s = s + term;
        }
      }
    }
    if (inside) {
      double mdl = bg + s;
      if (cov == 0) {
        res = a.outside == CTR_RESID_ZERO ? 0. : a.outside == CTR_RESID_NAN ? NAN : image;
        mdl = a.outside == CTR_RESID_NAN ? NAN : 0.;
      }
      a.residual[pix] = res;
      a.owner[pix] = own;
      if (a.model) a.model[pix] = mdl;
      if (a.coverage) a.coverage[pix] = cov;
    }
  }
}

__device__ __forceinline__ long long resid_wave_sum_ll(long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

template <int ND>
__global__ void __launch_bounds__(RESID_THREADS) resid_feature_kernel(const ResidArgs a) {
  if (ld_agent(a.status) != CTR_RESID_OK) return;
  constexpr int WAVES = RESID_THREADS / WAVE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int radius[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) radius[d] = a.radius[d];
  for (long long i = (long long)blockIdx.x * WAVES + wave; i < a.N; i += (long long)gridDim.x * WAVES) {
    // the frame of row i: the last t with frame_offset[t] <= i
    long long lo_t = 0, hi_t = a.T - 1;
    while (lo_t < hi_t) {
      const long long mid = (lo_t + hi_t + 1) >> 1;
      if (a.frame_offset[mid] <= i) lo_t = mid; else hi_t = mid - 1;
    }
    double cen[ND];
    resid_centre<ND>(a, i, cen);
    int b0[ND], bn[ND];
    long long vol = 1;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      double lo, hi;
      resid_box(cen[d], radius[d], a.shape[d], lo, hi);
      if (lo <= hi) {
        b0[d] = (int)floor(lo);
        bn[d] = (int)ceil(hi) - b0[d] + 1;
      } else {
        b0[d] = 0;
        bn[d] = 0;
      }
      vol *= bn[d];
    }
    long long n_pix = 0, n_own = 0, n_nan = 0;
    double sum = 0., sum_sq = 0., own_sq = 0., max_abs = 0.;
    for (long long p = lane; p < vol; p += WAVE) {
      int idx[ND];
      long long q = p;
#pragma unroll
      for (int d = ND - 1; d >= 0; --d) {
        idx[d] = b0[d] + (int)(q % bn[d]);
        q /= bn[d];
      }
      if (!in_mask_exact<ND>(idx, cen, radius)) continue;
      long long pix = 0;
#pragma unroll
      for (int d = 0; d < ND; ++d) pix = pix * a.shape[d] + idx[d];
      pix += lo_t * a.E;
      const double r = a.residual[pix];
      const bool mine = a.owner[pix] == (int)i;
      ++n_pix;
      n_own += mine ? 1 : 0;
      if (r != r) { ++n_nan; continue; }
      const double rr = r * r;
      sum = sum + r;
      sum_sq = sum_sq + rr;
      if (mine) own_sq = own_sq + rr;
      max_abs = fmax(max_abs, fabs(r));
    }
    n_pix = resid_wave_sum_ll(n_pix);
    n_own = resid_wave_sum_ll(n_own);
    n_nan = resid_wave_sum_ll(n_nan);
    sum = wave_sum(sum);
    sum_sq = wave_sum(sum_sq);
    own_sq = wave_sum(own_sq);
    max_abs = wave_max(max_abs);
    if (lane == 0) {
      a.n_pix[i] = n_pix;
      a.n_own[i] = n_own;
      a.n_nan[i] = n_nan;
      a.sum[i] = sum;
      a.sum_sq[i] = sum_sq;
      a.own_sum_sq[i] = own_sq;
      a.max_abs[i] = max_abs;
      a.rms[i] = sqrt(sum_sq / (double)n_pix);
    }
  }
}

// A workgroup per frame; a thread per row adds the rows of its cluster itself, from the cluster's
// first row to the end of the frame in ascending row order: every row of a cluster gets the same bytes.
__global__ void __launch_bounds__(RESID_THREADS) resid_cluster_kernel(const ResidArgs a) {
  if (ld_agent(a.status) == CTR_RESID_BAD_TABLE) return;
  bool bad = false;
  for (long long t = blockIdx.x; t < a.T; t += gridDim.x) {
    const long long r0 = a.frame_offset[t], r1 = a.frame_offset[t + 1];
    const double fm = a.fmax[t];
    for (long long i = r0 + threadIdx.x; i < r1; i += RESID_THREADS) {
      const long long c = a.cluster[i];
      long long n = 0;
      double sq = 0., cost = NAN;
      if (c < r0 || c > i || a.cluster[c] != c) {
        bad = true;
      } else {
        for (long long j = c; j < r1; ++j)
          if (a.cluster[j] == c) {
            n += a.n_own[j];
            sq = sq + a.own_sum_sq[j];
          }
        cost = sqrt(sq / (double)n) / fm;
      }
      a.cluster_n_pix[i] = n;
      a.cluster_sum_sq[i] = sq;
      a.cost[i] = cost;
    }
  }
  if (bad) st_agent(a.status, CTR_RESID_BAD_CLUSTER);
}

#endif  // CTREFINE_RESIDUAL_KERNELS_H
