// motion_kernels.h -- orientation and diffusion tensor of tracked clusters (ctr_orientation_device,
// ctr_diffusion_device).  Included by tu_motion.hip inside its anonymous namespace.
//
// The rule (reference motion.py:40-198, as include/ctrefine.h restates it):
//   orientation: per (track, frame) the cluster's coordinates in x, y(, z) order times mpp; per
//     permutation of the features (the reference's tables) the centre of mass with UNPERMUTED weights
//     and a right-handed basis of rows x, y, z from it; a frame with a missing coordinate, and a basis
//     with a non-finite entry, are NaN;
//   diffusion: per (track, lag, permutation, frame b) the 6-vector (bases[b] (pos[b + lag] - pos[b]),
//     0.5 sum_i e_i x (bases[b] bases[b + lag, i])); rows with a non-finite component are dropped, the
//     rest pooled over the permutations: tensor = mean(x x^T) 0.5 fps / lag.
//
// Layout of the work:
//   orientation_kernel<ND, CS>: one lane per (track, frame) loops over the permutations (they read
//     the same <= 12 coordinates); lanes of a wavefront are consecutive frames, so the stores of a
//     permutation cover one contiguous block of bases[t, p].
//   diffusion_partial_kernel: one workgroup per (track, permutation, tile of MOT_TILE frames).  It
//     stages the tile and the `halo` frames behind it (bases and positions, one LDS row per
//     component) once, then loops over the lags of the call: lane = frame b of the tile, the later
//     frame from LDS, or from global memory where it lies beyond the staged halo.  Per lag the 21
//     distinct products and the count are reduced over the wavefront (wave_sum4), then over the four
//     wavefronts in their order, and written as one partial per (track, lag, permutation, tile).
//     The tiles do not depend on the lags, and no sum depends on which other tracks or lags a call
//     holds: a (track, lag) gives the same bytes alone and inside a batch or a sweep.
//   diffusion_final_kernel: one workgroup per (track, lag) adds its partials in the order
//     permutation, tile, scales and writes tensor and n_samples.
#ifndef CTREFINE_MOTION_KERNELS_H
#define CTREFINE_MOTION_KERNELS_H

constexpr int MOT_THREADS = 256;
constexpr int MOT_TILE = 256;      // frames of a (track, permutation) per workgroup: one per lane
constexpr int MOT_ROW = 12;        // staged doubles per frame: 9 of the basis, 3 of the position
constexpr int MOT_NSUM = 22;       // 21 products x_i x_j (i <= j) and the count of rows
constexpr int MOT_NPAD = 24;       // ... padded to six groups of four (wave_sum4)
constexpr int MOT_RED = (MOT_THREADS / WAVE) * MOT_NPAD;   // doubles in front of the tile: one row per wavefront

struct OriArgs {
  long long T, F;
  double mpp;
  double w[4];
  const double* pos;
  const double* angles;
  double* com;
  double* bases;
};

struct DifArgs {
  int ndim, n_perm;
  int halo;                 // frames staged behind the tile (the host's decision, tu_motion.hip)
  long long T, F, n_lags, n_tiles;
  double fps;
  const long long* lags;
  const double* positions;
  const double* bases;
  double* partial;          // [T, n_lags, P, n_tiles, MOT_NSUM]
  double* tensor;
  long long* n_samples;
};

// motion.py:137-145
__host__ __device__ constexpr int mot_n_perm(int cs) { return cs == 2 ? 2 : cs == 3 ? 6 : 12; }
__host__ __device__ constexpr int mot_perm(int cs, int p, int k) {
  constexpr int P2[2][2] = {{0, 1}, {1, 0}};
  constexpr int P3[6][3] = {{0, 1, 2}, {2, 0, 1}, {1, 2, 0}, {2, 1, 0}, {0, 2, 1}, {1, 0, 2}};
  constexpr int P4[12][4] = {{0, 1, 2, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {1, 0, 2, 3}, {1, 2, 3, 0}, {1, 3, 0, 2},
                             {2, 0, 1, 3}, {2, 1, 3, 0}, {2, 3, 0, 1}, {3, 0, 1, 2}, {3, 1, 2, 0}, {3, 2, 0, 1}};
  return cs == 2 ? P2[p][k] : cs == 3 ? P3[p][k] : P4[p][k];
}

__device__ __forceinline__ void mot_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void mot_unit(double* v) {      // v / np.linalg.norm(v); 0 / 0 = NaN
  const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  v[0] /= n; v[1] /= n; v[2] /= n;
}

template <int ND, int CS>
__global__ __launch_bounds__(MOT_THREADS) void orientation_kernel(OriArgs a) {
  constexpr int P = mot_n_perm(CS);
  const long long i = (long long)blockIdx.x * MOT_THREADS + threadIdx.x;
  if (i >= a.T * a.F) return;
  const long long t = i / a.F, f = i - t * a.F;
  const double* src = a.pos + i * (CS * ND);
  double c[CS][3];
  bool present = true;
#pragma unroll
  for (int k = 0; k < CS; ++k)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      c[k][d] = d < ND ? src[k * ND + (ND - 1 - d)] * a.mpp : 0.;
      present = present && isfinite(c[k][d]);
    }
  double wsum = 0.;
#pragma unroll
  for (int k = 0; k < CS; ++k) wsum += a.w[k];
  double com[3] = {NAN, NAN, NAN};
#pragma unroll
  for (int p = 0; p < P; ++p) {
    double B[9] = {NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN, NAN};
    if (present) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        double s = 0.;
#pragma unroll
        for (int k = 0; k < CS; ++k) s += c[mot_perm(CS, p, k)][d] * a.w[k];
        com[d] = s / wsum;
      }
      double *x = B, *y = B + 3, *z = B + 6;
      const double* c0 = c[mot_perm(CS, p, 0)];
      if (ND == 2) {
        x[0] = c0[0] - com[0]; x[1] = c0[1] - com[1]; x[2] = 0.;
        mot_unit(x);
        z[0] = 0.; z[1] = 0.; z[2] = 1.;
      } else {
        z[0] = c0[0] - com[0]; z[1] = c0[1] - com[1]; z[2] = c0[2] - com[2];
        mot_unit(z);
        if (CS == 2) {
          // motion.py:3-16 (rotation_matrix about z by the caller's angle) applied to [1, 0, 0] x z
          const double th = a.angles[(t * P + p) * a.F + f];
          const double an = sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
          const double ca = cos(th / 2.), sa = sin(th / 2.);
          const double qb = -(z[0] / an) * sa, qc = -(z[1] / an) * sa, qd = -(z[2] / an) * sa;
          const double aa = ca * ca, bb = qb * qb, cc = qc * qc, dd = qd * qd;
          const double bc = qb * qc, ad = ca * qd, ac = ca * qc, ab = ca * qb, bd = qb * qd, cd = qc * qd;
          const double v[3] = {0., -z[2], z[1]};
          x[0] = (aa + bb - cc - dd) * v[0] + 2. * (bc + ad) * v[1] + 2. * (bd - ac) * v[2];
          x[1] = 2. * (bc - ad) * v[0] + (aa + cc - bb - dd) * v[1] + 2. * (cd + ab) * v[2];
          x[2] = 2. * (bd + ac) * v[0] + 2. * (cd - ab) * v[1] + (aa + dd - bb - cc) * v[2];
        } else {
          const double* c1 = c[mot_perm(CS, p, 1)];
          double u[3];
          if (CS == 3) {
            u[0] = c1[0] - com[0]; u[1] = c1[1] - com[1]; u[2] = c1[2] - com[2];
          } else {
            const double* c2 = c[mot_perm(CS, p, CS == 4 ? 2 : 1)];
            u[0] = c2[0] - c1[0]; u[1] = c2[1] - c1[1]; u[2] = c2[2] - c1[2];
          }
          mot_cross(z, u, x);
        }
        mot_unit(x);
      }
      mot_cross(z, x, y);
      mot_unit(y);
    }
    bool fin = present;
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && isfinite(B[k]);
    double* dst = a.bases + ((t * P + p) * a.F + f) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) dst[k] = fin ? B[k] : NAN;
  }
  double* cd = a.com + i * 3;
  cd[0] = com[0]; cd[1] = com[1]; cd[2] = com[2];      // 2D: the third coordinate is 0
}

// the 6-vector of one row: basis B and position q of frame b, basis C and position r of frame b + lag
__device__ __forceinline__ void mot_displ(const double* B, const double* q, const double* C, const double* r, double* x) {
  const double d0 = r[0] - q[0], d1 = r[1] - q[1], d2 = r[2] - q[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) x[i] = B[3 * i] * d0 + B[3 * i + 1] * d1 + B[3 * i + 2] * d2;
  // M(k, i) = (B C[i])_k = sum_j B[k][j] C[i][j]
  auto M = [&](int k, int i) { return B[3 * k] * C[3 * i] + B[3 * k + 1] * C[3 * i + 1] + B[3 * k + 2] * C[3 * i + 2]; };
  x[3] = 0.5 * (M(2, 1) - M(1, 2));
  x[4] = 0.5 * (M(0, 2) - M(2, 0));
  x[5] = 0.5 * (M(1, 0) - M(0, 1));
}

__global__ __launch_bounds__(MOT_THREADS) void diffusion_partial_kernel(DifArgs a) {
  extern __shared__ double mot_lds[];
  double* red = mot_lds;              // [MOT_THREADS / WAVE][MOT_NPAD]
  double* st = mot_lds + MOT_RED;     // [MOT_ROW][L]
  const int L = MOT_TILE + a.halo;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  long long blk = blockIdx.x;
  const long long tile = blk % a.n_tiles;
  blk /= a.n_tiles;
  const long long p = blk % a.n_perm, t = blk / a.n_perm;
  const long long b0 = tile * MOT_TILE;
  const long long left = a.F - b0;                              // >= 1
  const int n_st = (int)(left < (long long)L ? left : (long long)L);    // frames staged
  const double* gb = a.bases + ((t * a.n_perm + p) * a.F + b0) * 9;
  const double* gp = a.positions + (t * a.F + b0) * 3;
  for (int e = tid; e < n_st * 9; e += MOT_THREADS) {
    const int fr = e / 9, k = e - fr * 9;
    st[k * L + fr] = gb[e];
  }
  for (int e = tid; e < n_st * 3; e += MOT_THREADS) {
    const int fr = e / 3, k = e - fr * 3;
    st[(9 + k) * L + fr] = gp[e];
  }
  __syncthreads();
  const bool have = tid < n_st && tid < MOT_TILE;
  double B[9], q[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) B[k] = have ? st[k * L + tid] : NAN;
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = have ? st[(9 + k) * L + tid] : NAN;
  const long long b = b0 + tid;
  for (long long li = 0; li < a.n_lags; ++li) {
    const long long lag = a.lags[li];
    bool ok = have && lag >= 1 && lag < a.F && b < a.F - lag;
    double x[6] = {0., 0., 0., 0., 0., 0.};
    if (ok) {
      double C[9], r[3];
      const long long j = tid + lag;          // frame b + lag, counted from b0
      if (j < n_st) {
#pragma unroll
        for (int k = 0; k < 9; ++k) C[k] = st[k * L + (int)j];
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = st[(9 + k) * L + (int)j];
      } else {                                // beyond the staged halo
#pragma unroll
        for (int k = 0; k < 9; ++k) C[k] = gb[j * 9 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = gp[j * 3 + k];
      }
      mot_displ(B, q, C, r, x);
#pragma unroll
      for (int k = 0; k < 6; ++k) ok = ok && isfinite(x[k]);
    }
    double v[MOT_NPAD];
    {
      int n = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) v[n++] = ok ? x[i] * x[j] : 0.;
      v[21] = ok ? 1. : 0.;
      v[22] = 0.;
      v[23] = 0.;
    }
#pragma unroll
    for (int g = 0; g < MOT_NPAD / 4; ++g) {
      const double s = wave_sum4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3], lane);
      if ((lane & 15) == 0) red[wave * MOT_NPAD + 4 * g + (lane >> 4)] = s;
    }
    __syncthreads();
    if (tid < MOT_NSUM) {
      double s = red[tid];
#pragma unroll
      for (int w = 1; w < MOT_THREADS / WAVE; ++w) s += red[w * MOT_NPAD + tid];
      a.partial[((((t * a.n_lags + li) * a.n_perm + p) * a.n_tiles + tile)) * MOT_NSUM + tid] = s;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(WAVE) void diffusion_final_kernel(DifArgs a) {
  __shared__ double S[MOT_NPAD];
  const int tid = threadIdx.x;
  const long long blk = blockIdx.x;            // t * n_lags + li
  const long long li = blk % a.n_lags;
  const long long m_end = (long long)a.n_perm * a.n_tiles;
  if (tid < MOT_NSUM) {
    const double* src = a.partial + blk * m_end * MOT_NSUM + tid;
    double s = 0.;
    for (long long m = 0; m < m_end; ++m) s += src[m * MOT_NSUM];     // permutation, then tile
    S[tid] = s;
  }
  __syncthreads();
  const double n = S[21];
  const int D = a.ndim == 2 ? 3 : 6;
  if (tid < D * D) {
    int i = tid / D, j = tid - i * D;
    if (a.ndim == 2) { i = i == 2 ? 5 : i; j = j == 2 ? 5 : j; }      // x, y translation and z rotation
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const double s = S[lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)];
    const double dt = (double)a.lags[li] / a.fps;
    a.tensor[blk * (D * D) + tid] = n > 0. ? s / n * 0.5 / dt : NAN;
  }
  if (tid == 0) a.n_samples[blk] = (long long)n;
}

#endif  // CTREFINE_MOTION_KERNELS_H
