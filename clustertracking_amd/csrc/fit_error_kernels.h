// fit_error_kernels.h -- standard errors and covariance of a fitted table: the exact Hessian of the
// reference's objective per cluster, its Cholesky factor and its inverse (ctr_fit_error_device; the rule
// is in include/ctrefine.h).  Included inside the anonymous namespace of
// tu_fit_error.hip, after device_common.h and stage_common.h.  The unit is compiled without
// floating-point contraction.
//   fiterr_check_kernel   the caller's frame_offset, order, cluster_offset and the offsets of the
//                         covariance, before an index is followed
//   fiterr_refuse_kernel  a refused table: CTR_FITERR_BAD_TABLE on every row
//   fit_error_kernel      a workgroup per cluster, launched once per size class: A = J^T J + Q as a
//                         packed triangle in LDS, Cholesky, the inverse of the factor in place
// Every kernel strides over its items.
#ifndef CTREFINE_FIT_ERROR_KERNELS_H
#define CTREFINE_FIT_ERROR_KERNELS_H

constexpr int FE_THREADS = 256;
constexpr int FE_WAVES = FE_THREADS / WAVE;
constexpr int FE_MAXF = CTR_FITERR_MAX_ROWS;
// size classes: the most variables of a class and the pixel rows it stages at once.  The last
// class's request (triangle 65024 B + features 7168 B + rows 8192 B + 96 B) lets two workgroups
// share the 160 KiB of a CU.
constexpr int FE_CLASS_VARS[CTR_FITERR_CLASSES] = {16, 48, CTR_MAX_VARS};
constexpr int FE_CLASS_CHUNK[CTR_FITERR_CLASSES] = {256, 32, 8};
constexpr int FE_FD_MAX = 14;       // doubles of a staged feature: centre, position, sizes, signal, profile
constexpr int FE_SHARED = CTR_MAX_PARAMS;   // the values of the cluster variables, per column

__host__ __device__ constexpr int fe_nxm(int fit, int nd, bool iso) {
  return fit == CTR_FIT_GAUSS ? 0
         : fit != CTR_FIT_INV_SERIES ? 1
         : (CTR_MAX_PARAMS - 2 - nd - (iso ? 1 : nd) < INV_NX ? CTR_MAX_PARAMS - 2 - nd - (iso ? 1 : nd) : INV_NX);
}
__host__ __device__ constexpr int fe_tri(int i) { return (i * (i + 1)) / 2; }
// pixel rows of a class are `ld` doubles apart: the variables, odd so that rows fall on different banks
__host__ __device__ constexpr int fe_ld(int nv) { return nv | 1; }
// doubles of LDS of a class: triangle, features, pixel rows, cluster values
__host__ __device__ constexpr size_t fe_lds_doubles(int cls) {
  return (size_t)fe_tri(FE_CLASS_VARS[cls]) + (size_t)FE_MAXF * FE_FD_MAX + (size_t)FE_CLASS_CHUNK[cls] * fe_ld(FE_CLASS_VARS[cls]) + FE_SHARED;
}

struct FitErrArgs {
  int shape[3], radius[3];      // axis a of ndim at index a; 1 and 0 beyond
  int nx, n_params, dtype, want_cov;
  int modes[CTR_MAX_PARAMS];
  int n_var_cols, n_cl_cols;    // columns of CTR_MODE_VAR and of CTR_MODE_CLUSTER
  int cls, cls_lo, cls_hi;      // this launch takes the clusters with cls_lo < n_vars <= cls_hi (class 0: from 0, and the too large ones)
  int chunk;
  long long T, N, C, E, n_vars_total, n_cov_total;
  double residual_factor;
  const void* frames;
  const long long* frame_offset;
  const double* params;
  const double* mask_pos;       // null: the positions in params
  const long long* order;
  const long long* cluster_offset;
  const long long* var_offset;
  const long long* cov_offset;
  const double* fmax;           // [T] the frame maxima
  double* params_std;
  int* status;
  int* n_vars;
  long long* n_pix;
  double* cov;
  long long* var_row;
  int* var_col;
  int* table;                   // [1] scratch: 0 while the tables are taken
};

// variables of a cluster of n rows, and whether it is beyond the stage
__device__ __forceinline__ long long fe_cluster_vars(const FitErrArgs& a, long long n, bool& too_large) {
  const long long nv = (long long)a.n_var_cols * n + a.n_cl_cols;
  too_large = n > FE_MAXF || nv > CTR_MAX_VARS;
  return nv;
}

__global__ void __launch_bounds__(FE_THREADS) fiterr_check_kernel(const FitErrArgs a) {
  const long long stride = (long long)gridDim.x * FE_THREADS;
  long long n = a.T + 1 > a.N ? a.T + 1 : a.N;
  n = a.C + 1 > n ? a.C + 1 : n;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += stride) {
    if (i <= a.T)
      bad |= offsets_bad(a.frame_offset, i, a.T, a.N) || (i == 0 && a.frame_offset[0] != 0) || (i == a.T && a.frame_offset[i] != a.N);
    if (i < a.N) bad |= a.order[i] < 0 || a.order[i] >= a.N;
    if (i <= a.C) {
      bad |= offsets_bad(a.cluster_offset, i, a.C, a.N) || (i == 0 && a.cluster_offset[0] != 0) || (i == a.C && a.cluster_offset[i] != a.N);
      if (a.want_cov) {
        bad |= offsets_bad(a.var_offset, i, a.C, a.n_vars_total) || offsets_bad(a.cov_offset, i, a.C, a.n_cov_total);
        if (i < a.C) {
          bool too_large;
          long long nv = fe_cluster_vars(a, a.cluster_offset[i + 1] - a.cluster_offset[i], too_large);
          if (too_large) nv = 0;
          bad |= a.var_offset[i + 1] - a.var_offset[i] != nv || a.cov_offset[i + 1] - a.cov_offset[i] != nv * nv;
        }
      }
    }
  }
  if (bad) st_agent(a.table, 1);
}

__global__ void __launch_bounds__(FE_THREADS) fiterr_refuse_kernel(const FitErrArgs a) {
  if (ld_agent(a.table) == 0) return;
  const long long stride = (long long)gridDim.x * FE_THREADS;
  for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < a.N; i += stride) {
    a.status[i] = CTR_FITERR_BAD_TABLE;
    a.n_vars[i] = 0;
    a.n_pix[i] = 0;
    for (int k = 0; k < a.n_params; ++k) a.params_std[i * a.n_params + k] = NAN;
  }
  if (a.want_cov) {
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < a.n_cov_total; i += stride) a.cov[i] = NAN;
    for (long long i = (long long)blockIdx.x * FE_THREADS + threadIdx.x; i < a.n_vars_total; i += stride) {
      a.var_row[i] = -1;
      a.var_col[i] = -1;
    }
  }
}

// (row, column) of entry e of a packed lower triangle, column <= row
__device__ __forceinline__ void fe_untri(int e, int& r, int& c) {
  r = (int)((sqrt(8. * (double)e + 1.) - 1.) * 0.5);
  while (fe_tri(r + 1) <= e) ++r;
  while (fe_tri(r) > e) --r;
  c = e - fe_tri(r);
}

// What the rule calls g and its derivatives: in r2 (g1, g2), in the profile parameters (ge, gee as a
// packed triangle) and mixed (g1e).  q: the sum of d_a d_a, last axis first (the safe forms).
template <int FIT, int ND, int NXM>
__device__ __forceinline__ void fe_profile(double r2, double q, const double* ex, int nx, double& g, double& g1, double& g2,
                                           double (&ge)[NXM > 0 ? NXM : 1], double (&g1e)[NXM > 0 ? NXM : 1],
                                           double (&gee)[NXM > 0 ? fe_tri(NXM) : 1]) {
  const double k = 0.5 * ND;
  if constexpr (FIT == CTR_FIT_GAUSS) {
    g = exp(-0.5 * ND * r2);
    g1 = -k * g;
    g2 = k * k * g;
  } else if constexpr (FIT == CTR_FIT_INV_SERIES) {
    // y = r2^N + e1 r2^(N-1) + ... + eN, N = nx - 1; pw[t] = r2^(N - t), dpw[t] = (N - t) r2^(N - t - 1)
    double y = 1., dy = 0., ddy = 0.;
#pragma unroll
    for (int t = 1; t < NXM; ++t)
      if (t < nx) { ddy = ddy * r2 + 2. * dy; dy = dy * r2 + y; y = y * r2 + ex[t]; }
    const double e0 = ex[0], inv = 1. / y, inv2 = inv * inv, inv3 = inv2 * inv;
    g = e0 / y;
    g1 = -e0 * dy * inv2;
    g2 = e0 * (2. * dy * dy * inv3 - ddy * inv2);
    double pw[NXM], dpw[NXM];
    pw[0] = 0.; dpw[0] = 0.;
    double p = 1., dp = 0.;
#pragma unroll
    for (int t = NXM - 1; t >= 1; --t) {
      pw[t] = 0.; dpw[t] = 0.;
      if (t < nx) { pw[t] = p; dpw[t] = dp; dp = dp * r2 + p; p = p * r2; }
    }
    ge[0] = inv;
    g1e[0] = -dy * inv2;
    gee[0] = 0.;
#pragma unroll
    for (int t = 1; t < NXM; ++t) {
      ge[t] = -e0 * pw[t] * inv2;
      g1e[t] = -e0 * (dpw[t] * inv2 - 2. * dy * pw[t] * inv3);
      gee[fe_tri(t)] = -pw[t] * inv2;
#pragma unroll
      for (int u = 1; u <= t; ++u) gee[fe_tri(t) + u] = 2. * e0 * pw[t] * pw[u] * inv3;
    }
  } else {
    const double e = ex[0];
    ge[0] = 0.; g1e[0] = 0.; gee[0] = 0.;
    if (FIT == CTR_FIT_DISC && !(e > 0.)) {          // the Gaussian
      g = q < 1. ? NAN : exp(-0.5 * ND * r2);
      g1 = -k * g;
      g2 = k * k * g;
      return;
    }
    // phi(r, e) and its derivatives; g = exp(phi)
    double phi, p_r, p_rr, p_e, p_ee, p_re;
    const double r = sqrt(r2);
    bool flat = false, clamped = false;
    if constexpr (FIT == CTR_FIT_RING) {
      const double num = r - 1. + e, w = num / e;
      const double w_e = (1. - r) / (e * e), w_ee = -2. * (1. - r) / (e * e * e);
      phi = -0.5 * ND * (w * w);
      p_r = -2. * k * w / e;
      p_rr = -2. * k / (e * e);
      p_e = -2. * k * w * w_e;
      p_ee = -2. * k * (w_e * w_e + w * w_ee);
      p_re = -2. * k * (w_e * e - w) / (e * e);
      if (q < 1.) phi = NAN;
    } else {
      clamped = e >= 1.;
      const double ds = clamped ? 0.999 : e;
      const double W = 1. - ds, u = (r - ds) / W;
      const double u_d = (r - 1.) / (W * W), u_dd = 2. * (r - 1.) / (W * W * W);
      flat = !(r2 > ds * ds) || q < 1.;
      phi = u * u * ND / -2.;
      p_r = -2. * k * u / W;
      p_rr = -2. * k / (W * W);
      p_e = -2. * k * u * u_d;
      p_ee = -2. * k * (u_d * u_d + u * u_dd);
      p_re = -2. * k * (u_d / W + u / (W * W));
    }
    if (flat) {
      g = r2 == r2 || q < 1. ? 1. : NAN;
      g1 = 0.; g2 = 0.;
      return;
    }
    g = exp(phi);
    const double g_r = g * p_r, g_rr = g * (p_r * p_r + p_rr);
    g1 = g_r / (2. * r);
    g2 = g_rr / (4. * r2) - g_r / (4. * r2 * r);
    if (!clamped) {
      ge[0] = g * p_e;
      gee[0] = g * (p_e * p_e + p_ee);
      g1e[0] = g * (p_r * p_e + p_re) / (2. * r);
    }
  }
}

// a staged feature: the mask centre [ND], position [ND], size [1 or ND], signal, profile parameters [NXM]
template <int ND, bool ISO, int NXM>
struct FeLayout {
  static constexpr int NSZ = ISO ? 1 : ND, CEN = 0, POS = ND, SIZE = 2 * ND, SIG = 2 * ND + NSZ, EX = SIG + 1, FD = EX + NXM;
};

// d_a, r2 and q of a pixel for a staged feature, as the residual stage evaluates them
template <int ND, bool ISO, int NXM>
__device__ __forceinline__ void fe_r2(const double* R, const int (&idx)[ND], double (&dd)[ND], double (&i2)[ND], double& r2, double& q) {
  using L = FeLayout<ND, ISO, NXM>;
  r2 = 0.;
  q = 0.;
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    const double sz = R[L::SIZE + (ISO ? 0 : d)];
    dd[d] = (double)idx[d] - R[L::POS + d];
    i2[d] = 1. / (sz * sz);
    r2 = r2 + (dd[d] * dd[d]) * i2[d];
  }
#pragma unroll
  for (int d = ND - 1; d >= 0; --d) q = q + dd[d] * dd[d];
}

// The residual of pixel idx: ((image - background) - term_1) - term_2 ... over the covering rows of
// the cluster in row order; *covered: whether any row covers it.
template <int ND, bool ISO, int FIT>
__device__ __forceinline__ double fe_residual(const double* F, int n, const int (&idx)[ND], const int (&radius)[ND], int nx,
                                              double image, double bg, bool* covered) {
  constexpr int NXM = fe_nxm(FIT, ND, ISO);
  using L = FeLayout<ND, ISO, NXM>;
  double res = image - bg;
  bool any = false;
  for (int j = 0; j < n; ++j) {
    const double* R = F + j * L::FD;
    double cen[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) cen[d] = R[L::CEN + d];
    if (!in_mask_exact<ND>(idx, cen, radius)) continue;
    any = true;
    double dd[ND], i2[ND], r2, q, g, dg;
    fe_r2<ND, ISO, NXM>(R, idx, dd, i2, r2, q);
    if constexpr (FIT == CTR_FIT_GAUSS) {
      g = exp(-0.5 * ND * r2);
    } else if constexpr (FIT == CTR_FIT_INV_SERIES) {
      double ex[INV_NX], dge[INV_NX];
#pragma unroll
      for (int e = 0; e < INV_NX; ++e) ex[e] = e < NXM ? R[L::EX + (e < NXM ? e : 0)] : 0.;
      profile_inv_dev(nx, r2, ex, g, dg, dge);
    } else {
      double dge;
      const double e = R[L::EX];
      profile_dev<FIT, ND>(r2, e, g, dg, dge);
      if (q < 1.) g = (FIT == CTR_FIT_DISC && e > 0.) ? 1. : NAN;   // r2_*_safe
    }
    res = res - R[L::SIG] * g;
  }
  *covered = any;
  return res;
}

// the clipped box of a mask (residual_kernels.h: resid_box): first pixel and extent per axis
template <int ND>
__device__ __forceinline__ long long fe_box(const double* cen, const int (&radius)[ND], const int* shape, int (&b0)[ND], int (&bn)[ND]) {
  long long vol = 1;
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    const double c = cen[d];
    double lo = fmax(c - (double)radius[d] - 1., 0.);
    double hi = fmin(c + (double)radius[d] + 1., (double)(shape[d] - 1));
    if (!(c - c == 0.)) { lo = 1.; hi = 0.; }
    if (lo <= hi) {
      b0[d] = (int)floor(lo);
      bn[d] = (int)ceil(hi) - b0[d] + 1;
    } else {
      b0[d] = 0;
      bn[d] = 0;
    }
    vol *= bn[d];
  }
  return vol;
}

template <int ND>
__device__ __forceinline__ long long fe_pixel(long long p, const int (&b0)[ND], const int (&bn)[ND], const int* shape, int (&idx)[ND]) {
#pragma unroll
  for (int d = ND - 1; d >= 0; --d) {
    idx[d] = b0[d] + (int)(p % bn[d]);
    p /= bn[d];
  }
  long long pix = 0;
#pragma unroll
  for (int d = 0; d < ND; ++d) pix = pix * shape[d] + idx[d];
  return pix;
}

// first derivatives of r2 in the geometric parameters p = 0 .. ND + NSZ - 1 (centres, then sizes)
template <int ND, bool ISO>
__device__ __forceinline__ void fe_r2_first(const double (&dd)[ND], const double (&i2)[ND], const double* size, double r2,
                                            double (&r2p)[ND + (ISO ? 1 : ND)]) {
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    r2p[d] = -2. * dd[d] * i2[d];
    if (!ISO) r2p[ND + d] = -2. * dd[d] * dd[d] * i2[d] / size[d];
  }
  if (ISO) r2p[ND] = -2. * r2 / size[0];
}

// second derivative of r2 in the geometric parameters p >= q
template <int ND, bool ISO>
__device__ __forceinline__ double fe_r2_second(int p, int q, const double (&dd)[ND], const double (&i2)[ND], const double* size, double r2) {
  if (p < ND) return p == q ? 2. * i2[p] : 0.;
  if (ISO) return q < ND ? 4. * dd[q] * i2[q] / size[0] : 6. * r2 * i2[0];
  const int ax = p - ND;
  if (q < ND) return q == ax ? 4. * dd[ax] * i2[ax] / size[ax] : 0.;
  return q == p ? 6. * dd[ax] * dd[ax] * i2[ax] * i2[ax] : 0.;
}

template <int ND, bool ISO, int FIT>
__global__ void __launch_bounds__(FE_THREADS) fit_error_kernel(const FitErrArgs a) {
  extern __shared__ double fe_lds[];
  constexpr int NSZ = ISO ? 1 : ND, NG = ND + NSZ;
  constexpr int NXM = fe_nxm(FIT, ND, ISO), NXA = NXM > 0 ? NXM : 1;
  constexpr int PW = 1 + NG + NXM, PWT = fe_tri(PW);     // a feature's block: signal, centres, sizes, profile
  using L = FeLayout<ND, ISO, NXM>;
  static_assert(L::FD <= FE_FD_MAX, "a staged feature fits its slot");
  static_assert(FE_WAVES * PWT <= FE_CLASS_CHUNK[CTR_FITERR_CLASSES - 1] * fe_ld(FE_CLASS_VARS[CTR_FITERR_CLASSES - 1]), "the blocks of a round fit the pixel rows");
  __shared__ long long s_row[FE_MAXF];
  __shared__ int s_base[CTR_MAX_PARAMS];
  __shared__ int s_mode[CTR_MAX_PARAMS];
  __shared__ int s_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int np = a.n_params, nx = a.nx;
  double* const T = fe_lds;                                     // the packed triangle
  double* const F = T + fe_tri(a.cls_hi);                       // the staged features
  double* const J = F + FE_MAXF * FE_FD_MAX;                    // the pixel rows; later the blocks of a round, a column, the std
  double* const S = J + a.chunk * fe_ld(a.cls_hi);              // the values of the cluster variables
  int radius[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) radius[d] = a.radius[d];
  int shape[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) shape[d] = a.shape[d];
  if (ld_agent(a.table) != 0) return;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < CTR_MAX_PARAMS; ++k) s_mode[k] = a.modes[k];
  }
  __syncthreads();

  for (long long c = blockIdx.x; c < a.C; c += gridDim.x) {
    const long long c0 = a.cluster_offset[c], c1 = a.cluster_offset[c + 1];
    if (c1 == c0) continue;
    bool too_large;
    const long long nv_ll = fe_cluster_vars(a, c1 - c0, too_large);
    if (too_large ? a.cls != 0 : !(nv_ll > a.cls_lo || a.cls == 0) || nv_ll > a.cls_hi) continue;
    __syncthreads();     // the cluster before is done with the LDS
    if (too_large) {
      for (long long k = c0 + tid; k < c1; k += FE_THREADS) {
        const long long row = a.order[k];
        a.status[row] = CTR_FITERR_TOO_LARGE;
        a.n_vars[row] = nv_ll > 0x7fffffffLL ? 0x7fffffff : (int)nv_ll;
        a.n_pix[row] = 0;
        for (int col = 0; col < np; ++col) a.params_std[row * np + col] = NAN;
      }
      continue;
    }
    const int n = (int)(c1 - c0), nv = (int)nv_ll, ld = fe_ld(a.cls_hi);
    // the frame of the cluster: that of its first row; every row must lie in it
    const long long first = a.order[c0];
    long long t = 0, hi_t = a.T - 1;
    while (t < hi_t) {
      const long long mid = (t + hi_t + 1) >> 1;
      if (a.frame_offset[mid] <= first) t = mid; else hi_t = mid - 1;
    }
    const long long r0 = a.frame_offset[t], r1 = a.frame_offset[t + 1];
    bool bad = false;
    if (tid < n) {
      const long long row = a.order[c0 + tid];
      s_row[tid] = row;
      bad = row < r0 || row >= r1 || (tid > 0 && a.order[c0 + tid - 1] >= row);
    }
    if (tid == 0) {
      int base = 0;
      for (int col = 0; col < CTR_MAX_PARAMS; ++col) {
        const int mode = col < np ? s_mode[col] : CTR_MODE_CONST;
        s_base[col] = mode == CTR_MODE_CONST ? -1 : base;
        base += mode == CTR_MODE_VAR ? n : mode == CTR_MODE_CLUSTER ? 1 : 0;
      }
    }
    const int table_bad = __syncthreads_or(bad ? 1 : 0);
    // the value of a cluster variable: the first row's where all rows are equal, else the mean in row order
    if (tid < FE_SHARED) {
      double v = NAN;
      if (tid < np && !table_bad && (s_mode[tid] == CTR_MODE_CLUSTER || tid == 0)) {
        const double v0 = a.params[s_row[0] * np + tid];
        v = v0;
        if (s_mode[tid] == CTR_MODE_CLUSTER) {
          bool same = true;
          double sum = 0.;
          for (int k = 0; k < n; ++k) {
            const double x = a.params[s_row[k] * np + tid];
            same = same && x == v0;
            sum = sum + x;
          }
          if (!same) v = sum / (double)n;
        }
      }
      S[tid] = v;
    }
    __syncthreads();
    bool nonfinite = false;
    if (tid < n && !table_bad) {
      const long long row = s_row[tid];
      double* R = F + tid * L::FD;
      auto par = [&](int col) { return s_mode[col] == CTR_MODE_CLUSTER ? S[col] : a.params[row * np + col]; };
      double v = par(1);
      R[L::SIG] = v;
      nonfinite = !(v - v == 0.);
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const double pos = par(2 + d), sz = par(2 + ND + (ISO ? 0 : d));
        const double cen = a.mask_pos ? a.mask_pos[row * ND + d] : a.params[row * np + 2 + d];
        R[L::CEN + d] = cen;
        R[L::POS + d] = pos;
        R[L::SIZE + (ISO ? 0 : d)] = sz;
        nonfinite = nonfinite || !(pos - pos == 0.) || !(sz - sz == 0.) || !(cen - cen == 0.);
      }
#pragma unroll
      for (int e = 0; e < NXM; ++e) {
        v = e < nx ? par(2 + ND + NSZ + (e < nx ? e : 0)) : 0.;
        R[L::EX + e] = v;
        nonfinite = nonfinite || !(v - v == 0.);
      }
      if (tid == 0) { v = S[0]; nonfinite = nonfinite || !(v - v == 0.); }
    }
    const int any_nonfinite = __syncthreads_or(nonfinite ? 1 : 0);
    const double bg = S[0];
    const int ntri = fe_tri(nv);
    for (int e = tid; e < ntri; e += FE_THREADS) T[e] = 0.;

    int status = table_bad ? CTR_FITERR_BAD_TABLE : any_nonfinite ? CTR_FITERR_NONFINITE : CTR_FITERR_OK;
    long long P = 0;
    if (status == CTR_FITERR_OK) {
      // ---- J^T J: the covered pixels by owner, staged as rows of J, every entry of the triangle adds them in order
      int fill = 0;
      auto flush = [&]() {
        __syncthreads();
        for (int e = tid; e < ntri; e += FE_THREADS) {
          int r, cc;
          fe_untri(e, r, cc);
          double acc = T[e];
          for (int k = 0; k < fill; ++k) acc = acc + J[k * ld + r] * J[k * ld + cc];
          T[e] = acc;
        }
        __syncthreads();
        fill = 0;
      };
      for (int i = 0; i < n; ++i) {
        const double* Ri = F + i * L::FD;
        double cen[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) cen[d] = Ri[L::CEN + d];
        int b0[ND], bn[ND];
        const long long vol = fe_box<ND>(cen, radius, shape, b0, bn);
        for (long long p0 = 0; p0 < vol; p0 += a.chunk) {
          const long long p = p0 + tid;
          bool cand = tid < a.chunk && p < vol, ok = false;
          int idx[ND];
          long long pix = 0;
          if (cand) {
            pix = fe_pixel<ND>(p, b0, bn, shape, idx);
            cand = in_mask_exact<ND>(idx, cen, radius);
            for (int j = 0; cand && j < i; ++j) {
              double cj[ND];
#pragma unroll
              for (int d = 0; d < ND; ++d) cj[d] = F[j * L::FD + L::CEN + d];
              if (in_mask_exact<ND>(idx, cj, radius)) cand = false;     // an earlier row owns it
            }
          }
          if (cand) {
            bool covered;
            const double image = load_pixel(a.frames, a.dtype, (size_t)(t * a.E + pix));
            const double res = fe_residual<ND, ISO, FIT>(F, n, idx, radius, nx, image, bg, &covered);
            ok = res == res;
          }
          int total;
          const int at = workgroup_scan<FE_THREADS, int>((cand ? 0x10000 : 0) | (ok ? 1 : 0), total);
          P += total >> 16;
          const int n_ok = total & 0xffff;
          if (fill + n_ok > a.chunk) flush();
          if (ok) {
            double* row = J + (fill + (at & 0xffff)) * ld;
            for (int v = 0; v < nv; ++v) row[v] = 0.;
            if (s_base[0] >= 0) row[s_base[0]] = -1.;
            for (int j = 0; j < n; ++j) {
              const double* R = F + j * L::FD;
              double cj[ND];
#pragma unroll
              for (int d = 0; d < ND; ++d) cj[d] = R[L::CEN + d];
              if (!in_mask_exact<ND>(idx, cj, radius)) continue;
              double dd[ND], i2[ND], r2, q, g, g1, g2, ge[NXA], g1e[NXA], gee[NXM > 0 ? fe_tri(NXM) : 1], r2p[NG];
              fe_r2<ND, ISO, NXM>(R, idx, dd, i2, r2, q);
              fe_profile<FIT, ND, NXM>(r2, q, R + L::EX, nx, g, g1, g2, ge, g1e, gee);
              fe_r2_first<ND, ISO>(dd, i2, R + L::SIZE, r2, r2p);
              const double sig = R[L::SIG];
#pragma unroll
              for (int tt = 0; tt < PW; ++tt) {
                const int col = 1 + tt;
                if (col >= np) continue;
                const int base = s_base[col];
                if (base < 0) continue;
                const double dm = tt == 0 ? g : tt <= NG ? sig * g1 * r2p[tt <= NG ? (tt > 0 ? tt - 1 : 0) : 0] : sig * ge[tt > NG ? tt - 1 - NG : 0];
                if (s_mode[col] == CTR_MODE_VAR) row[base + j] = -dm;
                else row[base] = row[base] - dm;
              }
            }
          }
          fill += n_ok;
        }
      }
      flush();

      // ---- Q: the block of every feature over its own box, a wavefront per feature, four to a round
      double* const blocks = J;
      for (int i0 = 0; i0 < n; i0 += FE_WAVES) {
        const int i = i0 + wave;
        if (i < n) {
          const double* R = F + i * L::FD;
          double cen[ND], acc[PWT];
#pragma unroll
          for (int e = 0; e < PWT; ++e) acc[e] = 0.;
#pragma unroll
          for (int d = 0; d < ND; ++d) cen[d] = R[L::CEN + d];
          int b0[ND], bn[ND];
          const long long vol = fe_box<ND>(cen, radius, shape, b0, bn);
          const double sig = R[L::SIG];
          for (long long p = lane; p < vol; p += WAVE) {
            int idx[ND];
            const long long pix = fe_pixel<ND>(p, b0, bn, shape, idx);
            if (!in_mask_exact<ND>(idx, cen, radius)) continue;
            bool covered;
            const double image = load_pixel(a.frames, a.dtype, (size_t)(t * a.E + pix));
            const double res = fe_residual<ND, ISO, FIT>(F, n, idx, radius, nx, image, bg, &covered);
            if (res != res) continue;
            double dd[ND], i2[ND], r2, q, g, g1, g2, ge[NXA], g1e[NXA], gee[NXM > 0 ? fe_tri(NXM) : 1], r2p[NG];
            fe_r2<ND, ISO, NXM>(R, idx, dd, i2, r2, q);
            fe_profile<FIT, ND, NXM>(r2, q, R + L::EX, nx, g, g1, g2, ge, g1e, gee);
            fe_r2_first<ND, ISO>(dd, i2, R + L::SIZE, r2, r2p);
            // d2res = -d2m
#pragma unroll
            for (int tt = 1; tt < PW; ++tt) {
#pragma unroll
              for (int uu = 0; uu <= tt; ++uu) {
                double h;
                if (tt <= NG) {
                  const int p_ = tt - 1;
                  if (uu == 0) h = g1 * r2p[p_];
                  else h = sig * (g2 * r2p[p_] * r2p[uu > 0 ? uu - 1 : 0] + g1 * fe_r2_second<ND, ISO>(p_, uu > 0 ? uu - 1 : 0, dd, i2, R + L::SIZE, r2));
                } else {
                  const int k_ = tt - 1 - NG;
                  if (uu == 0) h = ge[k_ < NXA ? k_ : 0];
                  else if (uu <= NG) h = sig * g1e[k_ < NXA ? k_ : 0] * r2p[uu > 0 ? uu - 1 : 0];
                  else h = sig * gee[NXM > 0 ? fe_tri(k_) + (uu - 1 - NG) : 0];
                }
                acc[fe_tri(tt) + uu] = acc[fe_tri(tt) + uu] - res * h;
              }
            }
          }
#pragma unroll
          for (int e = 0; e < PWT; ++e) {
            const double s = wave_sum(acc[e]);
            if (lane == 0) blocks[wave * PWT + e] = s;
          }
        }
        __syncthreads();
        if (tid < PWT) {
          int tt, uu;
          fe_untri(tid, tt, uu);
          const int ct = 1 + tt, cu = 1 + uu;
          if (ct < np && s_base[ct] >= 0 && s_base[cu] >= 0) {
            for (int w = 0; w < FE_WAVES && i0 + w < n; ++w) {
              const int vt = s_base[ct] + (s_mode[ct] == CTR_MODE_VAR ? i0 + w : 0);
              const int vu = s_base[cu] + (s_mode[cu] == CTR_MODE_VAR ? i0 + w : 0);
              const int e = vt >= vu ? fe_tri(vt) + vu : fe_tri(vu) + vt;
              T[e] = T[e] + blocks[w * PWT + tid];
            }
          }
        }
        __syncthreads();
      }

      if (P == 0) status = CTR_FITERR_EMPTY;
    }

    if (status == CTR_FITERR_OK) {
      // ---- Cholesky of the packed triangle, in place
      for (int j = 0; j < nv; ++j) {
        if (tid == 0) {
          const double d = T[fe_tri(j) + j];
          const bool ok = d > 0. && d < INFINITY;
          s_flag = ok ? 1 : 0;
          if (ok) T[fe_tri(j) + j] = sqrt(d);
        }
        __syncthreads();
        if (!s_flag) { status = CTR_FITERR_NOT_POSITIVE_DEFINITE; break; }
        const double piv = T[fe_tri(j) + j];
        for (int i = j + 1 + tid; i < nv; i += FE_THREADS) T[fe_tri(i) + j] = T[fe_tri(i) + j] / piv;
        __syncthreads();
        const int m = fe_tri(nv - j - 1);
        for (int e = tid; e < m; e += FE_THREADS) {
          int ri, rk;
          fe_untri(e, ri, rk);
          const int i = j + 1 + ri, k = j + 1 + rk;
          T[fe_tri(i) + k] = T[fe_tri(i) + k] - T[fe_tri(i) + j] * T[fe_tri(k) + j];
        }
        __syncthreads();
      }
    }
    __syncthreads();

    double* const col = J;            // a column of the factor
    double* const stdv = J + 128;     // the std of every variable
    if (status == CTR_FITERR_OK) {
      // ---- the inverse of the factor in place, last column first
      for (int j = nv - 1; j >= 0; --j) {
        const double ajj = 1. / T[fe_tri(j) + j];
        for (int i = j + 1 + tid; i < nv; i += FE_THREADS) col[i] = T[fe_tri(i) + j];
        __syncthreads();
        if (tid == 0) T[fe_tri(j) + j] = ajj;
        for (int i = j + 1 + tid; i < nv; i += FE_THREADS) {
          double v = 0.;
          for (int k = j + 1; k <= i; ++k) v = v + T[fe_tri(i) + k] * col[k];
          T[fe_tri(i) + j] = -v * ajj;
        }
        __syncthreads();
      }
    }
    const double fm = a.fmax[t];
    const double pn = (double)P * (fm * fm / a.residual_factor);
    for (int v = tid; v < nv; v += FE_THREADS) {
      double s = NAN;
      if (status == CTR_FITERR_OK) {
        s = 0.;
        for (int k = v; k < nv; ++k) s = s + T[fe_tri(k) + v] * T[fe_tri(k) + v];
        s = sqrt(pn * s);
      }
      stdv[v] = s;
    }
    __syncthreads();
    for (int e = tid; e < n * np; e += FE_THREADS) {
      const int k = e / np, cc = e - k * np;
      const int base = s_base[cc];
      a.params_std[s_row[k] * np + cc] = base < 0 ? NAN : stdv[base + (s_mode[cc] == CTR_MODE_VAR ? k : 0)];
    }
    if (tid < n) {
      const long long row = s_row[tid];
      a.status[row] = status;
      a.n_vars[row] = nv;
      a.n_pix[row] = P;
    }
    if (a.want_cov) {
      const long long v0 = a.var_offset[c], q0 = a.cov_offset[c];
      for (int v = tid; v < nv; v += FE_THREADS) {
        int cc = 0;
        for (int k = 0; k < np; ++k)
          if (s_base[k] >= 0 && s_base[k] <= v) cc = k;
        a.var_col[v0 + v] = cc;
        a.var_row[v0 + v] = s_mode[cc] == CTR_MODE_VAR ? s_row[v - s_base[cc]] : -1;
      }
      for (int e = tid; e < nv * nv; e += FE_THREADS) {
        const int r = e / nv, cc = e - r * nv;
        const int lo = r < cc ? r : cc, hi = r < cc ? cc : r;
        double s = NAN;
        if (status == CTR_FITERR_OK) {
          s = 0.;
          for (int k = hi; k < nv; ++k) s = s + T[fe_tri(k) + hi] * T[fe_tri(k) + lo];
          s = pn * s;
        }
        a.cov[q0 + e] = s;
      }
    }
  }
}

#endif  // CTREFINE_FIT_ERROR_KERNELS_H
