// train_kernels.h -- training of shared fit parameters (ctr_train_device; the rule:
// include/ctrefine.h).  Included by tu_train.hip inside its anonymous namespace,
// after device_common.h.
//
// One iteration of a problem is two launches.  train_accumulate_kernel: one workgroup per cluster
// sums, over the pixels of the cluster's window, the entries of J^T J, J^T r and r^2 at the
// problem's trial point, divided by the cluster's pixel count, into its row of the partials
// table.  train_step_kernel: one workgroup per problem adds the rows of its clusters and runs the
// bookkeeping of the bounded LM (accept or reject the trial, the damping, the next trial, the
// stopping tests), all of it in the problem's state block that the next accumulate reads.  The
// kernel boundary is the only synchronisation: no workgroup waits for another, no atomics on
// floats, every sum in an order fixed by the launch geometry alone.
#ifndef CTREFINE_TRAIN_KERNELS_H
#define CTREFINE_TRAIN_KERNELS_H

constexpr int TRN_THREADS = 256;            // accumulate: lanes over the pixels of the window
constexpr int TRN_WAVES = TRN_THREADS / WAVE;
constexpr int TRN_MAXQ = CTR_TRAIN_MAX_GLOBALS;   // candidate columns: sizes, then the profile's
// a row of the partials table: r^2, pixel count, J^T r [q], J^T J packed [tri(q) + q']; padded
constexpr int TRN_K = 48;                   // >= 2 + 8 + 36
constexpr int TRN_R = 8;                    // step: clusters summed side by side (chunk of the reduce)
constexpr int TRN_STEP_THREADS = TRN_R * WAVE;
constexpr int TRN_FP = 20;                  // per-feature constants in LDS (accumulate)

// the state block of a problem, in doubles
enum {
  TS_X = 0,        // [8] accepted point
  TS_XT = 8,       // [8] trial point (what the accumulate kernel evaluates)
  TS_LO = 16, TS_HI = 24,
  TS_G = 32,       // [8] gradient of F / 2 at the accepted point
  TS_A = 40,       // [36] J^T J there, packed
  TS_S = 76,       // F there
  TS_MU = 77, TS_NU = 78,
  TS_PRED = 79,    // predicted decrease of the pending trial
  TS_STEP = 80,    // its relative size
  TS_GAIN = 82,    // relative decrease of F by the last accepted step
  TS_NORM = 83,
  TS_IT = 84,      // iterations begun
  TS_LAST = 85,    // the last trial was accepted
  TS_PHASE = 86,   // 0: the pending evaluation is the start's, 1: a trial's
  TS_SIZE = 96
};

struct TrnArgs {
  const void* frames;
  int frame_dtype;
  long long frame_elems;
  long long n_frames;
  long fshape[3];
  int radius[3];
  int n_params;
  int nx;                 // profile parameters (inv_series: N + 1)
  int nq;                 // candidate columns: sizes + nx
  int G;                  // variables
  int slot_of[TRN_MAXQ];  // candidate -> variable, or -1 (a constant column)
  int cand_of[TRN_MAXQ];  // variable -> candidate
  long long C, N;
  const double* params;
  const int* feat_offset;
  const int* frame_index;
  const int* problem_offset;
  const double* start;
  const double* low;
  const double* high;
  double* globals;
  double* cost;
  int* status;
  int* n_iter;
  double residual_factor, max_rms_dev, xtol, ftol;
  int maxiter;
  // scratch
  const double* fmax;     // [n_frames]
  double* partials;       // [C, TRN_K]
  double* state;          // [P, TS_SIZE]
  int* prob_of;           // [C]
  int* done;              // [P]
  int* n_done;            // [1]
};

__device__ __forceinline__ void train_finish(const TrnArgs& a, long long p, int status, const double* x, double cost,
                                             int iters) {
  const bool ok = status == CTR_STATUS_OK;
  for (int v = 0; v < a.G; ++v) a.globals[p * a.G + v] = ok ? x[v] : NAN;
  a.cost[p] = ok ? cost : NAN;
  a.status[p] = status;
  a.n_iter[p] = iters;
  a.done[p] = 1;
  atomicAdd(a.n_done, 1);
}

// One workgroup per problem: the tables are the caller's, so every offset is checked here before
// any kernel follows it; a problem that fails a check is finished with its status and its clusters
// are never looked at.
__global__ __launch_bounds__(TRN_THREADS) void train_setup_kernel(TrnArgs a) {
  const long long p = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ int s_bad[4];      // offsets, too large, non-finite, frame
  __shared__ double s_max[TRN_WAVES];
  if (tid < 4) s_bad[tid] = 0;
  __syncthreads();
  const long long c0 = a.problem_offset[p], c1 = a.problem_offset[p + 1];
  const bool range_ok = c0 >= 0 && c0 < c1 && c1 <= a.C;
  double m = 0.;
  if (range_ok) {
    for (long long c = c0 + tid; c < c1; c += TRN_THREADS) {
      const long long f0 = a.feat_offset[c], f1 = a.feat_offset[c + 1];
      const int t = a.frame_index[c];
      a.prob_of[c] = (int)p;
      if (f0 < 0 || f1 < f0 || f1 > a.N) { atomicOr(&s_bad[0], 1); continue; }
      if (f1 - f0 > MAXF) atomicOr(&s_bad[1], 1);
      if (t < 0 || t >= a.n_frames) { atomicOr(&s_bad[3], 1); continue; }
      m = fmax(m, a.fmax[t]);   // Python's max(norm, x): a NaN never wins
    }
  }
  m = wave_max(m);
  if ((tid & 63) == 0) s_max[tid >> 6] = m;
  __syncthreads();
  if (range_ok && !s_bad[0]) {
    // the features of a problem are the rows from its first cluster's to its last cluster's
    const long long r0 = (long long)a.feat_offset[c0] * a.n_params, r1 = (long long)a.feat_offset[c1] * a.n_params;
    bool bad = false;
    for (long long i = r0 + tid; i < r1; i += TRN_THREADS) bad = bad || !isfinite(a.params[i]);
    if (bad) atomicOr(&s_bad[2], 1);
  }
  __syncthreads();
  if (tid != 0) return;
  double* st = a.state + p * TS_SIZE;
  double x[TRN_MAXQ];
  bool infeasible = false;
#pragma unroll
  for (int v = 0; v < TRN_MAXQ; ++v) {
    x[v] = 0.;
    if (v < a.G) {
      const double lo = a.low[p * a.G + v], hi = a.high[p * a.G + v], s = a.start[p * a.G + v];
      infeasible = infeasible || !(lo <= hi);
      x[v] = s < lo ? lo : (s > hi ? hi : s);
      st[TS_LO + v] = lo;
      st[TS_HI + v] = hi;
    }
    st[TS_X + v] = x[v];
    st[TS_XT + v] = x[v];
  }
  double fm = s_max[0];
  for (int w = 1; w < TRN_WAVES; ++w) fm = fmax(fm, s_max[w]);
  st[TS_NORM] = fm * fm / a.residual_factor;
  st[TS_S] = 0.; st[TS_MU] = 1.; st[TS_NU] = 2.; st[TS_PRED] = 0.; st[TS_STEP] = 0.;
  st[TS_GAIN] = INFINITY; st[TS_IT] = 0.; st[TS_LAST] = 1.; st[TS_PHASE] = 0.;
  int status = CTR_STATUS_OK;
  if (!range_ok || s_bad[0] || s_bad[3]) status = CTR_STATUS_OUT_OF_BOUNDS;
  else if (s_bad[1]) status = CTR_STATUS_TOO_LARGE;
  else if (s_bad[2]) status = CTR_STATUS_NONFINITE;
  else if (infeasible) status = CTR_STATUS_NO_CONVERGENCE;
  a.done[p] = 0;
  if (status != CTR_STATUS_OK) train_finish(a, p, status, x, NAN, 0);
}

// ND, ISO, FIT as refine_block_kernel.  NQ candidate columns: the sizes, then the profile's
// parameters (inv_series: up to TRN_MAXQ in all, the absent ones are zero columns).
template <int ND, bool ISO, int FIT>
__global__ __launch_bounds__(TRN_THREADS) void train_accumulate_kernel(TrnArgs a) {
  constexpr int NSZ = ISO ? 1 : ND;
  constexpr int NXC = FIT == CTR_FIT_GAUSS ? 0 : (FIT == CTR_FIT_INV_SERIES ? TRN_MAXQ - NSZ : 1);
  constexpr int NQ = NSZ + NXC;
  constexpr int NA = NQ * (NQ + 1) / 2;
  constexpr bool SAFE_R2 = FIT == CTR_FIT_RING || FIT == CTR_FIT_DISC;   // r2_*_safe (fitfunc.py:396-411)
  static_assert(2 + NQ + NA <= TRN_K, "a row of the partials table");
  static_assert(NXC <= INV_NX, "profile parameters");
  const long long cl = blockIdx.x;
  const int prob = a.prob_of[cl];
  if (prob < 0 || a.done[prob]) return;   // a cluster of no problem; a finished problem
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NP = a.n_params;
  const int f0 = a.feat_offset[cl];
  const int n = a.feat_offset[cl + 1] - f0;      // 0 .. MAXF (train_setup_kernel)
  const double* xt = a.state + (long long)prob * TS_SIZE + TS_XT;

  __shared__ double fpar[MAXF * TRN_FP];
  __shared__ double red[TRN_WAVES][TRN_K];
  __shared__ int s_win[8];    // origin[3], wshape[3], valid, a size of 0

  // per-feature constants at the trial point: [0] signal, [1..3] centre, [4..6] 1 / size^2,
  // [7..9] 2 / size^3, [10 ..] the profile's parameters
  if (tid < 8) s_win[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += TRN_THREADS) {
    const double* row = a.params + (long long)(f0 + i) * NP;
    double* f = fpar + i * TRN_FP;
    f[0] = row[1];
    bool zero = false;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      f[1 + d] = row[2 + d];
      const int q = ISO ? 0 : d;
      const double s = a.slot_of[q] >= 0 ? xt[a.slot_of[q]] : row[2 + ND + q];
      zero = zero || s == 0.;
      f[4 + d] = 1. / (s * s);
      f[7 + d] = 2. / (s * s * s);
    }
#pragma unroll
    for (int t = 0; t < NXC; ++t)
      f[10 + t] = t < a.nx ? (a.slot_of[NSZ + t] >= 0 ? xt[a.slot_of[NSZ + t]] : row[2 + ND + NSZ + t]) : 0.;
    if (zero) s_win[7] = 1;
  }
  __syncthreads();
  // masks.py:42-68 on the centres: the union window, clipped to the frame
  if (tid == 0) {
    long wlo[ND], whi[ND];
    bool any = false;
    for (int i = 0; i < n; ++i) {
      long ci[ND];
      bool ok = true;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        ci[d] = (long)rint(fpar[i * TRN_FP + 1 + d]);
        if (!(ci[d] >= -(long)a.radius[d] && ci[d] < a.fshape[d] + a.radius[d])) ok = false;
      }
      if (!ok) continue;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        wlo[d] = (!any || ci[d] < wlo[d]) ? ci[d] : wlo[d];
        whi[d] = (!any || ci[d] > whi[d]) ? ci[d] : whi[d];
      }
      any = true;
    }
    if (any) {
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        long l = wlo[d] - a.radius[d], u = whi[d] + a.radius[d] + 1;
        l = l < 0 ? 0 : l;
        u = u > a.fshape[d] ? a.fshape[d] : u;
        s_win[d] = (int)l;
        s_win[3 + d] = (int)(u - l);
      }
      s_win[6] = 1;
    }
  }
  __syncthreads();

  double S = 0., cnt = 0., g[NQ], A[NA];
#pragma unroll
  for (int q = 0; q < NQ; ++q) g[q] = 0.;
#pragma unroll
  for (int q = 0; q < NA; ++q) A[q] = 0.;

  if (s_win[6]) {
    int origin[ND], wshape[ND], radius[ND];
    double inv_r2[ND];
    long long npix = 1;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      origin[d] = s_win[d];
      wshape[d] = s_win[3 + d];
      radius[d] = a.radius[d];
      inv_r2[d] = 1. / ((double)radius[d] * (double)radius[d]);
      npix *= wshape[d];
    }
    const char* frame = (const char*)a.frames + (size_t)a.frame_index[cl] * (size_t)a.frame_elems * dtype_size(a.frame_dtype);
    const double bg = a.params[(long long)f0 * NP];
    for (long long p = tid; p < npix; p += TRN_THREADS) {
      int idx[ND];
      long long q = p;
#pragma unroll
      for (int d = ND - 1; d > 0; --d) { idx[d] = (int)(q % wshape[d]); q /= wshape[d]; }
      idx[0] = (int)q;
      size_t off = 0;
#pragma unroll
      for (int d = 0; d < ND; ++d) off = off * (size_t)a.fshape[d] + (size_t)(idx[d] + origin[d]);
      const double pix = load_pixel(frame, a.frame_dtype, off);
      bool any = false;
      double res = pix - bg, J[NQ];
#pragma unroll
      for (int k = 0; k < NQ; ++k) J[k] = 0.;
      for (int i = 0; i < n; ++i) {
        const double* f = fpar + i * TRN_FP;
        double rel[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) rel[d] = f[1 + d] - (double)origin[d];
        if (!in_mask<ND>(idx, rel, inv_r2, radius)) continue;
        any = true;
        double r2 = 0., dd[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          dd[d] = (double)(idx[d] + origin[d]) - f[1 + d];
          r2 += dd[d] * dd[d] * f[4 + d];
        }
        const double sig = f[0];
        double gv, dg;
        if constexpr (FIT == CTR_FIT_GAUSS) {
          gv = exp(-0.5 * ND * r2);
          dg = -0.5 * ND * gv;
        } else if constexpr (FIT == CTR_FIT_INV_SERIES) {
          double ex[INV_NX], dge[INV_NX];
#pragma unroll
          for (int t = 0; t < INV_NX; ++t) ex[t] = t < NXC ? f[10 + t] : 0.;
          profile_inv_dev(a.nx, r2, ex, gv, dg, dge);
#pragma unroll
          for (int t = 0; t < NXC; ++t) J[NSZ + t] -= sig * dge[t];
        } else {
          double qraw = 0., dge;
#pragma unroll
          for (int d = ND - 1; d >= 0; --d) qraw += dd[d] * dd[d];
          profile_dev<FIT, ND>(r2, f[10], gv, dg, dge);
          // r2_*_safe: no value within one pixel of the centre (the disc has the value 1 there)
          if (SAFE_R2 && qraw < 1.) { gv = (FIT == CTR_FIT_DISC && f[10] > 0.) ? 1. : NAN; dg = 0.; dge = 0.; }
          J[NSZ] -= sig * dge;
        }
        res -= sig * gv;
        // d res / d size_a = -s dg/dr2 dr2/dsize_a, dr2/dsize_a = -2 dd_a^2 / size_a^3
        const double sdg = sig * dg;
        if (ISO) {
          double q2 = 0.;
#pragma unroll
          for (int d = 0; d < ND; ++d) q2 += dd[d] * dd[d];
          J[0] += sdg * (q2 * f[7]);
        } else {
#pragma unroll
          for (int d = 0; d < ND; ++d) J[d] += sdg * (dd[d] * dd[d] * f[7 + d]);
        }
      }
      if (!any) continue;
      cnt += 1.;
      if (res == res) {   // nansum (fitfunc.py:449,483)
        S += res * res;
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
          const double jk = J[k] == J[k] ? J[k] : 0.;
          g[k] += jk * res;
#pragma unroll
          for (int l = 0; l <= k; ++l) A[k * (k + 1) / 2 + l] += jk * (J[l] == J[l] ? J[l] : 0.);
        }
      }
    }
  }

  // lanes, then wavefronts, in a fixed order
  S = wave_sum(S);
  cnt = wave_sum(cnt);
  if (lane == 0) { red[wave][0] = S; red[wave][1] = cnt; }
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    const double t = wave_sum(g[k]);
    if (lane == 0) red[wave][2 + k] = t;
  }
#pragma unroll
  for (int k = 0; k < NA; ++k) {
    const double t = wave_sum(A[k]);
    if (lane == 0) red[wave][2 + NQ + k] = t;
  }
  __syncthreads();
  if (tid < TRN_K) {
    double t = 0.;
    if (tid < 2 + NQ + NA) {
      t = red[0][tid];
#pragma unroll
      for (int w = 1; w < TRN_WAVES; ++w) t += red[w][tid];
    }
    double P = red[0][1];
#pragma unroll
    for (int w = 1; w < TRN_WAVES; ++w) P += red[w][1];
    if (tid != 1) t = P > 0. ? t / P : 0.;
    if (tid == 0 && s_win[7]) t = NAN;   // a size of 0: no valid model
    a.partials[cl * TRN_K + tid] = t;
  }
}

// Cholesky factor of the leading n x n block of H (row-major, leading dimension TRN_MAXQ, lower
// triangle), in place; false where it is not positive definite
__device__ inline bool train_cholesky(double* H, int n) {
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j <= i; ++j) {
      double t = H[i * TRN_MAXQ + j];
      for (int k = 0; k < j; ++k) t -= H[i * TRN_MAXQ + k] * H[j * TRN_MAXQ + k];
      if (i == j) {
        if (!(t > 0.) || !isfinite(t)) return false;
        H[i * TRN_MAXQ + i] = sqrt(t);
      } else {
        H[i * TRN_MAXQ + j] = t / H[j * TRN_MAXQ + j];
      }
    }
  }
  return true;
}

__device__ inline void train_chol_solve(const double* H, int n, double* x) {
  for (int i = 0; i < n; ++i) {
    double t = x[i];
    for (int k = 0; k < i; ++k) t -= H[i * TRN_MAXQ + k] * x[k];
    x[i] = t / H[i * TRN_MAXQ + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double t = x[i];
    for (int k = i + 1; k < n; ++k) t -= H[k * TRN_MAXQ + i] * x[k];
    x[i] = t / H[i * TRN_MAXQ + i];
  }
}

// One workgroup per problem.  Launch i of a call (i = 0 judges the start) finds at least i iterations
// begun, so the launch behind solver_maxiter trials ends every problem at the iteration limit.
__global__ __launch_bounds__(TRN_STEP_THREADS) void train_step_kernel(TrnArgs a) {
  const long long p = blockIdx.x;
  if (a.done[p]) return;
  const int tid = threadIdx.x, k = tid & 63, j = tid >> 6;
  __shared__ double red[TRN_R][WAVE];
  __shared__ int empty[TRN_R];
  __shared__ double tot[TRN_K];
  __shared__ double st[TS_SIZE];
  // the solver's vectors live in LDS: they are indexed at run time (G, the free set)
  __shared__ double gt[TRN_MAXQ], At[TRN_MAXQ * TRN_MAXQ], H[TRN_MAXQ * TRN_MAXQ], w[TRN_MAXQ], dl[TRN_MAXQ],
      vt[TRN_MAXQ];
  __shared__ int fr[TRN_MAXQ];

  const long long c0 = a.problem_offset[p], c1 = a.problem_offset[p + 1];
  // the rows of the clusters c0 + j, c0 + j + TRN_R, ... in that order, then the TRN_R sums in order
  double acc = 0.;
  int none = 0;
  if (k < TRN_K)
    for (long long c = c0 + j; c < c1; c += TRN_R) {
      const double t = a.partials[c * TRN_K + k];
      acc += t;
      if (k == 1 && !(t > 0.)) none = 1;
    }
  red[j][k] = acc;
  if (k == 1) empty[j] = none;
  if (tid < TS_SIZE) st[tid] = a.state[p * TS_SIZE + tid];
  __syncthreads();
  if (tid < TRN_K) {
    double t = red[0][tid];
#pragma unroll
    for (int r = 1; r < TRN_R; ++r) t += red[r][tid];
    tot[tid] = t;
  }
  __syncthreads();

  if (tid == 0) {
    const int G = a.G;
    const double norm = st[TS_NORM];
    const double xtol = a.xtol > 0. ? a.xtol : 1e-9, ftol = a.ftol > 0. ? a.ftol : 1e-14;
    bool oob = false;
    for (int r = 0; r < TRN_R; ++r) oob = oob || empty[r] != 0;
    const double St = tot[0] / norm;
    for (int v = 0; v < G; ++v) {
      const int qv = a.cand_of[v];
      gt[v] = tot[2 + qv] / norm;
      for (int u = 0; u < G; ++u) {
        const int qu = a.cand_of[u];
        const int hi = qv > qu ? qv : qu, lo = qv > qu ? qu : qv;
        At[v * TRN_MAXQ + u] = tot[2 + a.nq + tri(hi) + lo] / norm;
      }
    }
    double S = st[TS_S], mu = st[TS_MU], nu = st[TS_NU], gain = st[TS_GAIN];
    int it = (int)st[TS_IT];
    bool last_acc = st[TS_LAST] != 0.;
    int finished = 0;     // 1 converged, 2 failed
    int status = CTR_STATUS_OK;
    bool take = false;

    if (st[TS_PHASE] == 0.) {
      if (oob) { finished = 2; status = CTR_STATUS_OUT_OF_BOUNDS; }
      else if (!isfinite(St)) { finished = 2; status = CTR_STATUS_NO_CONVERGENCE; }
      S = St;
      take = true;
    } else {
      const double pred = st[TS_PRED], act = 0.5 * (S - St);
      // Near the minimum the decrease of F drops below the rounding of its sum (F - Fmin is
      // quadratic in the distance) long before the gradient does: a trial whose F cannot be told
      // from the accepted point's is judged by the projected gradient instead, which both
      // evaluations carry.  Without this the iteration stalls at a relative distance of
      // sqrt(eps), where the reference's converged run is within tens of units in the last place.
      bool flat_better = false;
      if (isfinite(St) && pred > 0. && !(act > 0.) && fabs(act) <= 16. * 2.220446049250313e-16 * S) {
        double pg = 0., pgt = 0.;
        for (int v = 0; v < G; ++v) {
          const double lo = st[TS_LO + v], hi = st[TS_HI + v];
          const double x = st[TS_X + v], gx = st[TS_G + v], xn = st[TS_XT + v], gn = gt[v];
          if (!(lo == hi || (x <= lo && gx > 0.) || (x >= hi && gx < 0.))) pg = fmax(pg, fabs(gx));
          if (!(lo == hi || (xn <= lo && gn > 0.) || (xn >= hi && gn < 0.))) pgt = fmax(pgt, fabs(gn));
        }
        flat_better = pgt < pg;
      }
      if (isfinite(St) && pred > 0. && (act > 0. || flat_better)) {
        const double rho = act > 0. ? act / pred : 1., t = 2. * rho - 1., f = 1. - t * t * t;
        mu *= f > 1. / 3. ? f : 1. / 3.;
        nu = 2.;
        gain = (act > 0. ? act : 0.) / (0.5 * S + 1e-300);
        S = St;
        last_acc = true;
        take = true;
      } else {
        mu *= nu;
        nu *= 2.;
        last_acc = false;
        if (mu > 1e30) { finished = 2; status = CTR_STATUS_NO_CONVERGENCE; }
      }
      ++it;
    }
    if (take) {
      for (int v = 0; v < G; ++v) {
        st[TS_X + v] = st[TS_XT + v];
        st[TS_G + v] = gt[v];
        for (int u = 0; u <= v; ++u) st[TS_A + tri(v) + u] = At[v * TRN_MAXQ + u];
      }
    }
    int iters = it;
    // the next trial: iterations that need no pixel pass (a model that is not positive definite,
    // a step the projection turned uphill) are spent here
    bool pending = false;
    while (!finished && it < a.maxiter) {
      iters = it + 1;
      int nf = 0;
      for (int v = 0; v < G; ++v) {
        const double x = st[TS_X + v], gl = st[TS_G + v], lo = st[TS_LO + v], hi = st[TS_HI + v];
        const bool fixed = lo == hi || (x <= lo && gl > 0.) || (x >= hi && gl < 0.);
        if (!fixed) fr[nf++] = v;
      }
      if (nf == 0) { finished = 1; break; }
      for (int r = 0; r < nf; ++r) {
        for (int c = 0; c <= r; ++c) {
          const int hi = fr[r] > fr[c] ? fr[r] : fr[c], lo = fr[r] > fr[c] ? fr[c] : fr[r];
          H[r * TRN_MAXQ + c] = st[TS_A + tri(hi) + lo];
        }
        const double d = st[TS_A + tri(fr[r]) + fr[r]];
        H[r * TRN_MAXQ + r] += mu * (d > 1e-300 ? d : 1.);
        w[r] = st[TS_G + fr[r]];
      }
      bool reject = !train_cholesky(H, nf);
      double pred = 0., stepmax = 0.;
      if (!reject) {
        train_chol_solve(H, nf, w);
        for (int v = 0; v < G; ++v) dl[v] = 0.;
        for (int r = 0; r < nf; ++r) dl[fr[r]] = -w[r];
        for (int v = 0; v < G; ++v) {
          const double x = st[TS_X + v], t = x + dl[v], lo = st[TS_LO + v], hi = st[TS_HI + v];
          vt[v] = t < lo ? lo : (t > hi ? hi : t);
          dl[v] = vt[v] - x;
          const double rel = fabs(dl[v]) / (fabs(x) + 1.);
          stepmax = rel > stepmax ? rel : stepmax;
        }
        double gd = 0., dAd = 0.;
        for (int v = 0; v < G; ++v) {
          double t = 0.;
          for (int u = 0; u < G; ++u) {
            const int hi = v > u ? v : u, lo = v > u ? u : v;
            t += st[TS_A + tri(hi) + lo] * dl[u];
          }
          dAd += dl[v] * t;
          gd += st[TS_G + v] * dl[v];
        }
        pred = -(gd + 0.5 * dAd);
        if ((last_acc && stepmax <= xtol) || fabs(pred) <= ftol * (0.5 * S) + 1e-300) { finished = 1; break; }
        reject = !(pred > 0.);
      }
      if (reject) {
        mu *= nu;
        nu *= 2.;
        last_acc = false;
        if (mu > 1e30) { finished = 2; status = CTR_STATUS_NO_CONVERGENCE; break; }
        ++it;
        continue;
      }
      // an evaluation with a size of 0 is not valid: the accumulate kernel answers it with NaN
      for (int v = 0; v < G; ++v) st[TS_XT + v] = vt[v];
      st[TS_PRED] = pred;
      st[TS_STEP] = stepmax;
      pending = true;
      break;
    }
    if (!finished && !pending) {   // it == maxiter: stationary objective counts as converged
      finished = gain <= CTR_STALL_TOL ? 1 : 2;
      status = finished == 1 ? CTR_STATUS_OK : CTR_STATUS_NO_CONVERGENCE;
      iters = a.maxiter;
    }
    st[TS_S] = S; st[TS_MU] = mu; st[TS_NU] = nu; st[TS_GAIN] = gain;
    st[TS_IT] = (double)it; st[TS_LAST] = last_acc ? 1. : 0.; st[TS_PHASE] = 1.;
    if (finished) {
      double cost = sqrt(S / a.residual_factor);
      bool finite = true;
      for (int v = 0; v < G; ++v) finite = finite && isfinite(st[TS_X + v]);
      if (finished == 1) {
        if (!finite || !isfinite(cost)) status = CTR_STATUS_NO_CONVERGENCE;
        else if (cost > a.max_rms_dev) status = CTR_STATUS_RMS_DEV;
      }
      train_finish(a, p, status, st + TS_X, cost, iters);
    }
  }
  __syncthreads();
  if (tid < TS_SIZE) a.state[p * TS_SIZE + tid] = st[tid];
}

#endif  // CTREFINE_TRAIN_KERNELS_H
