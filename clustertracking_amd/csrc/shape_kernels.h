// shape_kernels.h -- shape coordinates of tracked clusters: bonds, angles and the radius of gyration
// of every (track, frame), their displacement statistics over a sweep of lags, their static moments
// and their histograms (ctr_shape_device, ctr_shape_dynamics_device, ctr_shape_histogram_device;
// include/ctrefine.h has the rule).  Included by tu_shape.hip inside its anonymous
// namespace.
//
// Layout of the work:
//   shape_coords_kernel<ND, CS>: one lane per (track, frame), lanes along the frames.  It writes
//     coordinate c of frame i at out[c * cstride + i * fstride]: the public block [T, F, C] (cstride
//     1, fstride C), or the scratch of the other two calls, coordinate-major [C][T F] (cstride T F,
//     fstride 1), where the stores of a coordinate are contiguous and so is every later read.
//   shape_partial_kernel: one workgroup per (track, tile of SHP_TILE frames).  It stages the tile and
//     the `halo` frames behind it, one LDS row per coordinate, then loops over the lags of the call:
//     lane = frame b of the tile, the later frame from LDS, or from global memory where it lies
//     beyond the staged halo.  Per (lag, coordinate) the count and the sums of d, d^2, d^4 are reduced
//     over the wavefront (wave_sum4), then over the four wavefronts in their order, and written as
//     one partial per (track, tile, lag, coordinate).  The tiles do not depend on the lags, and no
//     sum depends on which other tracks or lags a call holds.
//   shape_final_kernel: one thread per (track, coordinate, lag) adds its tiles in tile order, and
//     leaves the four sums of the track in scratch.
//   shape_pool_kernel: one thread per (coordinate, lag) adds those sums of the tracks in track order.
//   shape_moments_kernel: one workgroup per (track, coordinate): count, sum, min, max of the finite
//     values, then the squared deviations from the mean in a second pass; fixed trees.
//   shape_hist_kernel: one workgroup per (group, coordinate, chunk of SHP_HIST_CHUNK frames), group =
//     a track (per_track) or all frames: uint32 counters in LDS, integer atomics, the non-zero ones
//     added to the int64 tables; shape_density_kernel divides.
// Every grid is exact (the launch checks that it fits): no kernel strides past its grid.
#ifndef CTREFINE_SHAPE_KERNELS_H
#define CTREFINE_SHAPE_KERNELS_H

constexpr int SHP_THREADS = 256;
constexpr int SHP_WAVES = SHP_THREADS / WAVE;
constexpr int SHP_TILE = CTR_SHAPE_TILE;      // frames of a track per workgroup: one per lane
constexpr int SHP_MAXC = CTR_SHAPE_MAX_COORDS;
constexpr int SHP_NSUM = 4;                   // count and the sums of d, d^2, d^4 of a (coordinate, lag)
constexpr int SHP_RED_ROW = 80;               // >= SHP_NSUM * SHP_MAXC = 76: the sums of one wavefront
constexpr int SHP_RED = SHP_WAVES * SHP_RED_ROW;       // doubles in front of the staged rows
constexpr int SHP_HALO_CAP = CTR_SHAPE_HALO_CAP;
constexpr int SHP_HIST_CHUNK = 4096;          // frames of a workgroup of the histogram
constexpr int SHP_MAX_BINS = CTR_SHAPE_MAX_BOND_BINS;  // >= CTR_SHAPE_MAX_ANGLE_BINS

static_assert(SHP_TILE == SHP_THREADS, "one lane per frame of the tile");
static_assert(SHP_RED_ROW >= SHP_NSUM * SHP_MAXC && CTR_SHAPE_MAX_ANGLE_BINS <= SHP_MAX_BINS, "room of the reductions and counters");

__host__ __device__ constexpr int shp_nb(int cs) { return cs * (cs - 1) / 2; }
__host__ __device__ constexpr int shp_na(int cs) { return cs * (cs - 1) * (cs - 2) / 2; }
__host__ __device__ constexpr int shp_nc(int cs) { return shp_nb(cs) + shp_na(cs) + 1; }

struct ShpCoordArgs {
  long long n;               // T F
  double mpp[3];
  const double* pos;
  double* out;
  long long cstride, fstride;
};

struct ShpDynArgs {
  int C, halo;               // halo: frames staged behind the tile (the host's decision, tu_shape.hip)
  long long T, F, n_lags, n_tiles;
  double fps;
  const long long* lags;
  const double* q;           // [C][T F]
  double* partial;           // [T, n_tiles, n_lags, C, SHP_NSUM]
  double* track_sums;        // [T, C, n_lags, SHP_NSUM]: the sums of a track, its tiles added
  long long* n;              // [T, C, L]
  double *mean_d, *mean_d2, *mean_d4, *flex;
  long long* pooled_n;       // [C, L]
  double *pooled_mean_d, *pooled_mean_d2, *pooled_mean_d4, *pooled_flex;
  long long* count;          // [T, C]
  double *mean, *var, *min, *max;
};

struct ShpHistArgs {
  int C, NB, NA;
  long long TF, G, FG, chunks;     // groups (T or 1), frames of a group, chunks of a group
  int B, A;
  double inv_dr, inv_da, bond_dr, angle_width;
  const double* q;           // [C][T F]
  const double* bond_edges;  // [B + 1]
  const double* angle_edges; // [A + 1]
  unsigned long long* count_bond;    // [G, NB + 1, B]
  unsigned long long* above;         // [G, NB + 1]
  unsigned long long* count_angle;   // [G, NA, A]
  unsigned long long* n;             // [G]
  double* density_bond;
  double* density_angle;
};

// Rule 1: the C coordinates of one frame from its CS * ND positions.  Every product, sum and square
// root is rounded on its own (the unit is compiled without contraction).
template <int ND, int CS>
__device__ __forceinline__ void shp_coords(const double* __restrict__ src, const double* mpp, double* q) {
#pragma clang fp contract(off)
  constexpr int C = shp_nc(CS);
  double x[CS][ND];
  bool present = true;
#pragma unroll
  for (int i = 0; i < CS; ++i)
#pragma unroll
    for (int k = 0; k < ND; ++k) {
      x[i][k] = src[i * ND + k] * mpp[k];
      present = present && isfinite(x[i][k]);
    }
  int c = 0;
#pragma unroll
  for (int a = 0; a < CS; ++a)
#pragma unroll
    for (int b = a + 1; b < CS; ++b) {
      double d2 = 0.;
#pragma unroll
      for (int k = 0; k < ND; ++k) {
        const double d = x[b][k] - x[a][k];
        const double dd = d * d;
        d2 = k == 0 ? dd : d2 + dd;
      }
      q[c++] = __dsqrt_rn(d2);
    }
#pragma unroll
  for (int a = 0; a < CS; ++a)
#pragma unroll
    for (int b = 0; b < CS; ++b)
#pragma unroll
      for (int e = b + 1; e < CS; ++e) {
        if (b == a || e == a) continue;
        double u[ND], v[ND];
        double dot = 0.;
#pragma unroll
        for (int k = 0; k < ND; ++k) {
          u[k] = x[b][k] - x[a][k];
          v[k] = x[e][k] - x[a][k];
          const double uv = u[k] * v[k];
          dot = dot + uv;                     // from +0: coincident features give dot = +0 and the angle 0, never -0 and pi
        }
        double cr;
        if (ND == 2) {
          const double p0 = u[0] * v[1], p1 = u[1] * v[0];
          cr = fabs(p0 - p1);
        } else {
          const double a0 = u[1] * v[ND - 1], a1 = u[ND - 1] * v[1];
          const double b0 = u[ND - 1] * v[0], b1 = u[0] * v[ND - 1];
          const double e0 = u[0] * v[1], e1 = u[1] * v[0];
          const double c0 = a0 - a1, c1 = b0 - b1, c2 = e0 - e1;
          const double s0 = c0 * c0, s1 = c1 * c1, s2 = c2 * c2;
          const double s01 = s0 + s1;
          cr = __dsqrt_rn(s01 + s2);
        }
        q[c++] = atan2(cr, dot);
      }
  double cen[ND];
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    double s = x[0][k];
#pragma unroll
    for (int i = 1; i < CS; ++i) s = s + x[i][k];
    cen[k] = s / (double)CS;
  }
  double s = 0.;
#pragma unroll
  for (int i = 0; i < CS; ++i)
#pragma unroll
    for (int k = 0; k < ND; ++k) {
      const double e = x[i][k] - cen[k];
      const double ee = e * e;
      s = (i == 0 && k == 0) ? ee : s + ee;
    }
  q[c++] = __dsqrt_rn(s / (double)CS);
  if (!present) {
#pragma unroll
    for (int j = 0; j < C; ++j) q[j] = NAN;
  }
}

template <int ND, int CS>
__global__ __launch_bounds__(SHP_THREADS) void shape_coords_kernel(ShpCoordArgs a) {
  constexpr int C = shp_nc(CS);
  const long long i = (long long)blockIdx.x * SHP_THREADS + threadIdx.x;
  if (i >= a.n) return;
  double q[C];
  shp_coords<ND, CS>(a.pos + i * (CS * ND), a.mpp, q);
  double* dst = a.out + i * a.fstride;
#pragma unroll
  for (int c = 0; c < C; ++c) dst[c * a.cstride] = q[c];
}

__global__ __launch_bounds__(SHP_THREADS) void shape_partial_kernel(ShpDynArgs a) {
  extern __shared__ double shp_lds[];
  double* red = shp_lds;              // [SHP_WAVES][SHP_RED_ROW]
  double* st = shp_lds + SHP_RED;     // [C][L]
  const int L = SHP_TILE + a.halo, C = a.C;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const long long blk = blockIdx.x;
  const long long tile = blk % a.n_tiles, t = blk / a.n_tiles;
  const long long b0 = tile * SHP_TILE;
  const long long left = a.F - b0;                              // >= 1
  const int n_st = (int)(left < (long long)L ? left : (long long)L);    // frames staged
  const long long TF = a.T * a.F;
  const double* g = a.q + t * a.F + b0;                         // coordinate c of frame b0 + j: g[c TF + j]
  for (int c = 0; c < C; ++c)
    for (int e = tid; e < n_st; e += SHP_THREADS) st[c * L + e] = g[c * TF + e];
  __syncthreads();
  const bool have = tid < n_st;
  const long long b = b0 + tid;
  for (long long li = 0; li < a.n_lags; ++li) {
    const long long lag = a.lags[li];
    const bool ok = have && lag >= 1 && lag < a.F && b < a.F - lag;
    const long long j = tid + lag;            // frame b + lag, counted from b0
    for (int c = 0; c < C; ++c) {
      double v0 = 0., v1 = 0., v2 = 0., v3 = 0.;
      if (ok) {
        const double q0 = st[c * L + tid];
        const double q1 = j < n_st ? st[c * L + (int)j] : g[c * TF + j];      // beyond the staged halo
        if (isfinite(q0) && isfinite(q1)) {
          const double d = q1 - q0;
          const double d2 = d * d;
          v0 = 1.; v1 = d; v2 = d2; v3 = d2 * d2;
        }
      }
      const double s = wave_sum4(v0, v1, v2, v3, lane);
      if ((lane & 15) == 0) red[wave * SHP_RED_ROW + SHP_NSUM * c + (lane >> 4)] = s;
    }
    __syncthreads();
    if (tid < SHP_NSUM * C) {
      double s = red[tid];
#pragma unroll
      for (int w = 1; w < SHP_WAVES; ++w) s += red[w * SHP_RED_ROW + tid];
      a.partial[(((t * a.n_tiles + tile) * a.n_lags + li) * C) * SHP_NSUM + tid] = s;
    }
    __syncthreads();
  }
}

// the means of rule 2 from a count and three sums
__device__ __forceinline__ void shp_means(double n, double s1, double s2, double s4, double fps, long long lag,
                                          double* mean_d, double* mean_d2, double* mean_d4, double* flex) {
  const bool any = n > 0.;
  const double m2 = any ? s2 / n : NAN;
  *mean_d = any ? s1 / n : NAN;
  *mean_d2 = m2;
  *mean_d4 = any ? s4 / n : NAN;
  *flex = any ? ((m2 * 0.5) * fps) / (double)lag : NAN;
}

__global__ __launch_bounds__(SHP_THREADS) void shape_final_kernel(ShpDynArgs a) {
  const long long i = (long long)blockIdx.x * SHP_THREADS + threadIdx.x;      // (t C + c) L + li
  if (i >= a.T * a.C * a.n_lags) return;
  const long long li = i % a.n_lags, tc = i / a.n_lags;
  const long long c = tc % a.C, t = tc / a.C;
  double n = 0., s1 = 0., s2 = 0., s4 = 0.;
  for (long long tile = 0; tile < a.n_tiles; ++tile) {
    const double* p = a.partial + ((((t * a.n_tiles + tile) * a.n_lags + li) * a.C) + c) * SHP_NSUM;
    n += p[0]; s1 += p[1]; s2 += p[2]; s4 += p[3];
  }
  a.n[i] = (long long)n;
  shp_means(n, s1, s2, s4, a.fps, a.lags[li], a.mean_d + i, a.mean_d2 + i, a.mean_d4 + i, a.flex + i);
  double* sums = a.track_sums + i * SHP_NSUM;       // for shape_pool_kernel
  sums[0] = n; sums[1] = s1; sums[2] = s2; sums[3] = s4;
}

__global__ __launch_bounds__(SHP_THREADS) void shape_pool_kernel(ShpDynArgs a) {
  const long long i = (long long)blockIdx.x * SHP_THREADS + threadIdx.x;      // c L + li
  if (i >= a.C * a.n_lags) return;
  const long long li = i % a.n_lags, c = i / a.n_lags;
  double N = 0., S1 = 0., S2 = 0., S4 = 0.;
  for (long long t = 0; t < a.T; ++t) {
    const double* p = a.track_sums + (((t * a.C + c) * a.n_lags) + li) * SHP_NSUM;
    N += p[0]; S1 += p[1]; S2 += p[2]; S4 += p[3];
  }
  a.pooled_n[i] = (long long)N;
  shp_means(N, S1, S2, S4, a.fps, a.lags[li], a.pooled_mean_d + i, a.pooled_mean_d2 + i, a.pooled_mean_d4 + i,
            a.pooled_flex + i);
}

__global__ __launch_bounds__(SHP_THREADS) void shape_moments_kernel(ShpDynArgs a) {
  __shared__ double s_red[SHP_WAVES][4];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const long long blk = blockIdx.x;           // t C + c
  const long long c = blk % a.C, t = blk / a.C;
  const double* g = a.q + c * (a.T * a.F) + t * a.F;
  double s = 0., n = 0., lo = INFINITY, hi = -INFINITY;
  for (long long f = tid; f < a.F; f += SHP_THREADS) {
    const double v = g[f];
    if (isfinite(v)) { s += v; n += 1.; lo = fmin(lo, v); hi = fmax(hi, v); }
  }
  const double sn = wave_sum4(s, n, 0., 0., lane);      // rows 0 and 1 of the wavefront: the sum, the count
  lo = -wave_max(-lo);
  hi = wave_max(hi);
  if (lane == 0) { s_red[wave][0] = sn; s_red[wave][2] = lo; s_red[wave][3] = hi; }
  if (lane == 16) s_red[wave][1] = sn;
  __syncthreads();
  double S = s_red[0][0], N = s_red[0][1];
  lo = s_red[0][2];
  hi = s_red[0][3];
#pragma unroll
  for (int w = 1; w < SHP_WAVES; ++w) {
    S += s_red[w][0]; N += s_red[w][1];
    lo = fmin(lo, s_red[w][2]); hi = fmax(hi, s_red[w][3]);
  }
  const double mean = S / N;                  // N == 0: not used
  double ss = 0.;
  for (long long f = tid; f < a.F; f += SHP_THREADS) {
    const double v = g[f];
    if (isfinite(v)) { const double e = v - mean; ss += e * e; }
  }
  ss = wave_sum(ss);
  __syncthreads();                            // every thread has read the first pass
  if (lane == 0) s_red[wave][0] = ss;
  __syncthreads();
  if (tid == 0) {
    double SS = s_red[0][0];
#pragma unroll
    for (int w = 1; w < SHP_WAVES; ++w) SS += s_red[w][0];
    const bool any = N > 0.;
    a.count[blk] = (long long)N;
    a.mean[blk] = any ? mean : NAN;
    a.var[blk] = any ? SS / N : NAN;
    a.min[blk] = any ? lo : NAN;
    a.max[blk] = any ? hi : NAN;
  }
}

// The bin of v among `bins` bins with the edges e[0 .. bins] (rule 3): the product guesses, the
// handed-over edges decide.  e[0] <= v and (v < e[bins] or closed): both loops end inside.
__device__ __forceinline__ int shp_bin(const double* __restrict__ e, double v, double inv_width, int bins) {
  int b = (int)(v * inv_width);
  b = b < 0 ? 0 : b > bins - 1 ? bins - 1 : b;
  while (b > 0 && v < e[b]) --b;
  while (b < bins - 1 && v >= e[b + 1]) ++b;
  return b;
}

__global__ __launch_bounds__(SHP_THREADS) void shape_hist_kernel(ShpHistArgs a) {
  __shared__ unsigned s_count[SHP_MAX_BINS + 1];
  __shared__ unsigned s_n;
  const int tid = threadIdx.x;
  long long blk = blockIdx.x;
  const long long chunk = blk % a.chunks;
  blk /= a.chunks;
  const int r = (int)(blk % a.C);
  const long long grp = blk / a.C;
  const bool angle = r >= a.NB && r < a.C - 1;
  const int bins = angle ? a.A : a.B;
  const double* e = angle ? a.angle_edges : a.bond_edges;
  const double inv = angle ? a.inv_da : a.inv_dr;
  const double top = e[bins];
  for (int j = tid; j <= bins; j += SHP_THREADS) s_count[j] = 0;
  if (tid == 0) s_n = 0;
  __syncthreads();
  const long long f0 = chunk * SHP_HIST_CHUNK;
  const long long f1 = f0 + SHP_HIST_CHUNK < a.FG ? f0 + SHP_HIST_CHUNK : a.FG;
  const double* src = a.q + r * a.TF + grp * a.FG;
  unsigned mine = 0;
  for (long long f = f0 + tid; f < f1; f += SHP_THREADS) {
    const double v = src[f];
    if (v != v) continue;                     // a NaN is nowhere
    ++mine;
    if (!(v >= e[0])) continue;
    if (angle) {
      if (v > top) continue;                  // the last bin is closed at pi; atan2 gives nothing above
    } else if (v >= top) {
      atomicAdd(&s_count[bins], 1u);          // above
      continue;
    }
    atomicAdd(&s_count[shp_bin(e, v, inv, bins)], 1u);
  }
  if (r == 0 && mine) atomicAdd(&s_n, mine);
  __syncthreads();
  const int row = angle ? r - a.NB : (r < a.NB ? r : a.NB);      // rg is the last row of the bonds' tables
  for (int j = tid; j <= bins; j += SHP_THREADS) {
    const unsigned cnt = s_count[j];
    if (cnt == 0) continue;
    unsigned long long* to;
    if (angle) {
      if (j == bins) continue;
      to = a.count_angle + (grp * a.NA + row) * a.A + j;
    } else {
      to = j < bins ? a.count_bond + (grp * (a.NB + 1) + row) * a.B + j : a.above + grp * (a.NB + 1) + row;
    }
    atomicAdd(to, (unsigned long long)cnt);
  }
  if (r == 0 && tid == 0 && s_n) atomicAdd(a.n + grp, (unsigned long long)s_n);
}

__global__ __launch_bounds__(SHP_THREADS) void shape_density_kernel(ShpHistArgs a) {
  const long long i = (long long)blockIdx.x * SHP_THREADS + threadIdx.x;
  const long long per_b = (long long)(a.NB + 1) * a.B, per_a = (long long)a.NA * a.A;
  const long long nb = a.G * per_b, na = a.G * per_a;
  if (i < nb) {
    const double n = (double)a.n[i / per_b];
    a.density_bond[i] = n > 0. ? (double)a.count_bond[i] / (n * a.bond_dr) : NAN;
  } else if (i < nb + na) {
    const long long k = i - nb;
    const double n = (double)a.n[k / per_a];
    a.density_angle[k] = n > 0. ? (double)a.count_angle[k] / (n * a.angle_width) : NAN;
  }
}

#endif  // CTREFINE_SHAPE_KERNELS_H
