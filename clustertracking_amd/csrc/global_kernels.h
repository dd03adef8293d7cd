// global_kernels.h -- shared and per-feature parameters fitted in one problem (ctr_refine_global_device;
// the rule: include/ctrefine.h).  Included by tu_global.hip inside its anonymous
// namespace, after device_common.h and block_kernel.h (wsync, chol_factor_w, chol_solve_w).
//
// The damped normal matrix of a problem is an arrowhead: a block A_c + mu D_c per cluster, its
// coupling B_c to the G shared columns, the G x G corner.  One iteration is four launches:
//   global_eval_kernel    one workgroup per cluster: back-substitutes the cluster's part of the
//                         step, projects it, and builds the rows [J_local | J_global | r] of its
//                         window at the trial point in LDS row tiles (the block kernel's scheme),
//                         contracted with v_mfma_f64_16x16x4_f64: A_c, B_c, the cluster's part of
//                         the corner, both gradients and F_c out of one contraction;
//   global_judge_kernel   one workgroup per problem: adds F, the predicted decrease and the corner
//                         over its clusters, accepts or rejects, Nielsen's update, the stopping tests;
//   global_factor_kernel  one wavefront per cluster: Cholesky of the free part of A_c + mu D_c,
//                         (A_c + mu D_c)^-1 [B_c g_c], the Schur row G_c - B_c^T (..)^-1 B_c and
//                         the reduced gradient; at the end of a round, whether a feature moved;
//   global_solve_kernel   one workgroup per problem: adds the Schur rows, solves the G x G system
//                         on the free shared variables, projects; at the end of a round, decides
//                         between another window round and the result.
// Which of them has work is the problem's phase word; the kernel boundary is the only
// synchronisation, no float atomics, every sum in an order fixed by the launch geometry.
#ifndef CTREFINE_GLOBAL_KERNELS_H
#define CTREFINE_GLOBAL_KERNELS_H

constexpr int GLB_MAXG = CTR_REFINE_GLOBAL_MAX_GLOBALS;
constexpr int GLB_MAXNV = CTR_REFINE_GLOBAL_MAX_COLUMNS;   // locals + globals + the residual column
constexpr int GLB_MAXNT = GLB_MAXNV / 16;
constexpr int GLB_TPMAX = GLB_MAXNV * (GLB_MAXNV + 1) / 2;
constexpr int GLB_SK = 48;      // a Schur row: S packed [36], reduced gradient [8], [44] a flag
constexpr int GLB_EK = 56;      // an evaluation row: F, P, pred, step, pg, pg trial, ., ., g_g [8], G_c packed [36]
constexpr int GLB_R = 8;        // problem kernels: clusters summed side by side (chunk of the reduce)
constexpr int GLB_PROB_THREADS = GLB_R * WAVE;
constexpr int GLB_SETUP_THREADS = 256;
constexpr int GLB_FP = 20;      // per-feature constants in LDS (evaluation)
constexpr int GLB_CONST = -100; // value table: a constant column

static_assert(GLB_MAXG * (GLB_MAXG + 1) / 2 + GLB_MAXG + 1 <= GLB_SK, "a Schur row");
static_assert(16 + GLB_MAXG * (GLB_MAXG + 1) / 2 <= GLB_EK && GLB_EK <= WAVE && GLB_SK <= WAVE, "an evaluation row");

// what the next kernel of a problem has to do
enum { GP_EVAL0 = 0, GP_TRIAL = 1, GP_SKIP = 2, GP_WRITE = 3, GP_REWINDOW = 4, GP_FACTOR = 5, GP_CHECK = 6 };

// the state block of a problem, in doubles
enum {
  GS_X = 0,        // [8] accepted shared values
  GS_XT = 8,       // [8] trial
  GS_LO = 16, GS_HI = 24,
  GS_G = 32,       // [8] gradient of F / 2 at the accepted point, shared part
  GS_A = 40,       // [36] the corner of J^T J there, packed
  GS_DG = 76,      // [8] the unprojected shared step of the pending trial
  GS_X0 = 84,      // [8] the call's start (every round begins there)
  GS_S = 92,       // F at the accepted point
  GS_MU = 93, GS_NU = 94, GS_GAIN = 95, GS_NORM = 96,
  GS_IT = 97,      // iterations begun in this round
  GS_LAST = 98,    // the last trial was accepted
  GS_PHASE = 99,
  GS_ROUND = 100,  // window rounds finished
  GS_NIT = 101,    // iterations of the rounds finished
  GS_CUR = 102,    // which of the two buffers of a cluster's row holds the accepted point
  GS_COST = 103,
  GS_SIZE = 104
};

struct GlbArgs {
  const void* frames;
  int frame_dtype;
  long long frame_elems;
  long long n_frames;
  long fshape[3];
  int radius[3];
  int ndim, n_params, nx;
  int G, LM;              // shared variables; the call's stated most locals of a cluster
  int ncl, nvar;          // CLUSTER columns, VAR columns: L_c = ncl + n_c * nvar
  int xbase;              // the first profile column: 2 + ndim + size columns
  int inv_shift;          // inv_series: the slots of the evaluation's series minus nx (see global_eval_kernel); else 0
  int mode[CTR_MAX_PARAMS];
  int gslot[CTR_MAX_PARAMS];   // column -> shared variable, or -1
  long long C, N;
  const double* params;
  const int* feat_offset;
  const int* frame_index;
  const int* problem_offset;
  const double* start;    // [P, G]
  const double* low;
  const double* high;
  const double* lstart;   // [C, LM]
  const double* llow;
  const double* lhigh;
  double* params_out;
  double* globals;
  double* cost;
  int* status;
  int* n_rounds;
  int* n_iter;
  double residual_factor, max_rms_dev, max_shift, xtol, ftol;
  int maxiter, max_rounds;
  // scratch
  const double* fmax;     // [n_frames]
  double* rows;           // [C, row_stride]: M [2][TP], x [2][LM], start, low, high [LM], Y [G + 1][LM]
  long long row_stride;
  int TP;                 // packed triangle of LM + G + 1 columns
  double* sch;            // [C, GLB_SK]
  double* ev;             // [C, GLB_EK]
  double* state;          // [P, GS_SIZE]
  double* mco;            // [N, 3] mask centres of the round
  int* prob_of;           // [C]
  int* done;              // [P]
  int* n_done;            // [1]
};

// Where the columns of a cluster of n features live.  vb/vs: the value of column k of feature i is
// local variable vb + vs * i (vb >= 0), shared variable -1 - vb, or the table's (GLB_CONST).
// rb/rs: its derivative goes to column rb + rs * i of the row tile; constants go to the pad column.
// rb/rs are indexed by the SLOT of the derivative in the evaluation: the column itself, except
// the inv_series coefficients behind signal_mult, which sit inv_shift slots further on.
__device__ inline void glb_tables(const GlbArgs& a, int n, int L, int pad, int* vb, int* vs, int* rb, int* rs) {
  int base = 0;
  for (int k = 0; k < CTR_MAX_PARAMS; ++k) { rb[k] = pad; rs[k] = 0; }
  for (int k = 0; k < CTR_MAX_PARAMS; ++k) {
    const int m = k < a.n_params ? a.mode[k] : CTR_MODE_CONST;
    const int slot = k > a.xbase ? k + a.inv_shift : k;      // < CTR_MAX_PARAMS (the host's choice of inv_shift)
    if (m == CTR_MODE_VAR) { vb[k] = base; vs[k] = 1; rb[slot] = base; rs[slot] = 1; base += n; }
    else if (m == CTR_MODE_CLUSTER) { vb[k] = base; vs[k] = 0; rb[slot] = base; rs[slot] = 0; base += 1; }
    else if (m == CTR_MODE_GLOBAL) { vb[k] = -1 - a.gslot[k]; vs[k] = 0; rb[slot] = L + a.gslot[k]; rs[slot] = 0; }
    else { vb[k] = GLB_CONST; vs[k] = 0; }
  }
}

__device__ __forceinline__ double glb_val(const int* vb, const int* vs, const double* xl, const double* xg,
                                          const double* prow, int k, int i) {
  const int b = vb[k];
  if (b >= 0) return xl[b + vs[k] * i];
  if (b > GLB_CONST) return xg[-1 - b];
  return prow[k];
}

__device__ __forceinline__ bool glb_fixed(double x, double g, double lo, double hi) {
  return lo == hi || (x <= lo && g > 0.) || (x >= hi && g < 0.);
}

__device__ __forceinline__ void glb_finish(const GlbArgs& a, long long p, const double* st, int status, double cost) {
  const bool ok = status == CTR_STATUS_OK;
  for (int v = 0; v < a.G; ++v) a.globals[p * a.G + v] = ok ? st[GS_X + v] : NAN;
  a.cost[p] = ok ? cost : NAN;
  a.status[p] = status;
  a.n_rounds[p] = (int)st[GS_ROUND];
  a.n_iter[p] = (int)st[GS_NIT];
  a.done[p] = 1;
  atomicAdd(a.n_done, 1);
}

// One workgroup per problem: the tables are the caller's, so every offset is checked here before
// any kernel follows it; a problem that fails a check is finished with its status and its clusters
// are never looked at.  Then the rows of its clusters: start clipped into the box, the bounds, the
// mask centres of the first round.
__global__ __launch_bounds__(GLB_SETUP_THREADS) void global_setup_kernel(GlbArgs a) {
  const long long p = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ int s_bad[5];      // offsets, too large, non-finite, frame, an empty box
  __shared__ double s_max[GLB_SETUP_THREADS / WAVE];
  if (tid < 5) s_bad[tid] = 0;
  __syncthreads();
  const long long c0 = a.problem_offset[p], c1 = a.problem_offset[p + 1];
  const bool range_ok = c0 >= 0 && c0 < c1 && c1 <= a.C;
  double m = 0.;
  if (range_ok) {
    for (long long c = c0 + tid; c < c1; c += GLB_SETUP_THREADS) {
      const long long f0 = a.feat_offset[c], f1 = a.feat_offset[c + 1];
      const int t = a.frame_index[c];
      a.prob_of[c] = (int)p;
      if (f0 < 0 || f1 < f0 || f1 > a.N) { atomicOr(&s_bad[0], 1); continue; }
      const long long L = a.ncl + (f1 - f0) * a.nvar;
      if (f1 - f0 > MAXF || L > a.LM || L + a.G + 1 > GLB_MAXNV) atomicOr(&s_bad[1], 1);
      if (t < 0 || t >= a.n_frames) { atomicOr(&s_bad[3], 1); continue; }
      m = fmax(m, a.fmax[t]);   // Python's max(norm, x): a NaN never wins
    }
  }
  m = wave_max(m);
  if ((tid & 63) == 0) s_max[tid >> 6] = m;
  __syncthreads();
  const bool tables_ok = range_ok && !s_bad[0] && !s_bad[1] && !s_bad[3];
  if (range_ok && !s_bad[0]) {
    const long long r0 = (long long)a.feat_offset[c0] * a.n_params, r1 = (long long)a.feat_offset[c1] * a.n_params;
    bool bad = false;
    for (long long i = r0 + tid; i < r1; i += GLB_SETUP_THREADS) bad = bad || !isfinite(a.params[i]);
    if (bad) atomicOr(&s_bad[2], 1);
  }
  if (tables_ok) {
    const int LM = a.LM;
    const long long oX = 2LL * a.TP;
    for (long long e = tid; e < (c1 - c0) * LM; e += GLB_SETUP_THREADS) {
      const long long c = c0 + e / LM;
      const int v = (int)(e % LM);
      const int L = a.ncl + (a.feat_offset[c + 1] - a.feat_offset[c]) * a.nvar;
      double* x = a.rows + c * a.row_stride + oX;
      double lo = 0., hi = 0., s = 0.;
      if (v < L) {
        lo = a.llow[c * LM + v]; hi = a.lhigh[c * LM + v]; s = a.lstart[c * LM + v];
        if (!(lo <= hi) || !isfinite(s)) atomicOr(&s_bad[4], 1);
        s = s < lo ? lo : (s > hi ? hi : s);
      }
      x[v] = s; x[LM + v] = s; x[2 * LM + v] = s; x[3 * LM + v] = lo; x[4 * LM + v] = hi;
    }
    const long long q0 = a.feat_offset[c0], q1 = a.feat_offset[c1];
    for (long long e = 3 * q0 + tid; e < 3 * q1; e += GLB_SETUP_THREADS) {
      const long long r = e / 3;
      const int d = (int)(e % 3);
      a.mco[e] = d < a.ndim ? a.params[r * a.n_params + 2 + d] : 0.;
    }
  }
  __syncthreads();
  if (tid != 0) return;
  double* st = a.state + p * GS_SIZE;
  for (int i = 0; i < GS_SIZE; ++i) st[i] = 0.;
  bool infeasible = s_bad[4] != 0;
  for (int v = 0; v < a.G; ++v) {
    const double lo = a.low[p * a.G + v], hi = a.high[p * a.G + v], s = a.start[p * a.G + v];
    infeasible = infeasible || !(lo <= hi);
    const double x = s < lo ? lo : (s > hi ? hi : s);
    st[GS_LO + v] = lo; st[GS_HI + v] = hi;
    st[GS_X + v] = x; st[GS_XT + v] = x; st[GS_X0 + v] = x;
  }
  double fm = s_max[0];
  for (int w = 1; w < GLB_SETUP_THREADS / WAVE; ++w) fm = fmax(fm, s_max[w]);
  st[GS_NORM] = fm * fm / a.residual_factor;
  st[GS_MU] = 1.; st[GS_NU] = 2.; st[GS_GAIN] = INFINITY; st[GS_LAST] = 1.; st[GS_PHASE] = GP_EVAL0;
  int status = CTR_STATUS_OK;
  if (!range_ok || s_bad[0] || s_bad[3]) status = CTR_STATUS_OUT_OF_BOUNDS;
  else if (s_bad[1]) status = CTR_STATUS_TOO_LARGE;
  else if (s_bad[2]) status = CTR_STATUS_NONFINITE;
  else if (infeasible) status = CTR_STATUS_NO_CONVERGENCE;
  a.done[p] = 0;
  if (status != CTR_STATUS_OK) glb_finish(a, p, st, status, NAN);
}

constexpr int glb_waves(int nt) { return nt == 1 ? 4 : (nt == 2 ? 2 : 1); }

// ND, ISO, FIT as refine_block_kernel; NT: 16-column tiles of the row (locals + globals + residual).
// Column order of a row: the cluster's locals (per column of the table: a CLUSTER column one entry,
// a VAR column one per feature), the G shared columns, the residual.
template <int ND, bool ISO, int FIT, int NT>
__global__ __launch_bounds__(WAVE * glb_waves(NT)) void global_eval_kernel(GlbArgs a) {
  constexpr int W = glb_waves(NT), NVP = 16 * NT, RS = NVP + 1, NTILE = NT * (NT + 1) / 2, ROWS = WAVE * RS;
  constexpr int T = WAVE * W;
  constexpr int NSZ = ISO ? 1 : ND;
  constexpr int NXMAX = CTR_MAX_PARAMS - (2 + ND + NSZ);
  constexpr int NXC = FIT == CTR_FIT_GAUSS ? 0 : (FIT == CTR_FIT_INV_SERIES ? (NXMAX < INV_NX ? NXMAX : INV_NX) : 1);
  constexpr int NPC = 2 + ND + NSZ + NXC;
  constexpr bool SAFE_R2 = FIT == CTR_FIT_RING || FIT == CTR_FIT_DISC;   // r2_*_safe (fitfunc.py:396-411)
  static_assert(W == 1 || (4 / W) * NTILE * 4 * WAVE <= ROWS, "the parked accumulators must fit a row tile");
  static_assert(NPC <= CTR_MAX_PARAMS && 10 + NXC <= 17 && 17 < GLB_FP, "columns");

  const long long cl = blockIdx.x;
  const int prob = a.prob_of[cl];
  if (prob < 0 || a.done[prob]) return;   // a cluster of no problem; a finished problem
  const double* st = a.state + (long long)prob * GS_SIZE;
  const int phase = (int)st[GS_PHASE];
  if (phase != GP_EVAL0 && phase != GP_TRIAL && phase != GP_WRITE && phase != GP_REWINDOW) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NP = a.n_params, G = a.G, LM = a.LM;
  const int f0 = a.feat_offset[cl];
  const int n = a.feat_offset[cl + 1] - f0;      // 0 .. MAXF (global_setup_kernel)
  const int L = a.ncl + n * a.nvar, nv = L + G;  // nv + 1 <= 16 NT (the host chose NT from LM >= L)
  const int cur = (int)st[GS_CUR];
  double* crow = a.rows + cl * a.row_stride;
  const double* Macc = crow + (size_t)cur * a.TP;
  double* Mtr = crow + (size_t)(1 - cur) * a.TP;
  const double* Xacc = crow + 2 * (size_t)a.TP + (size_t)cur * LM;
  double* Xtr = crow + 2 * (size_t)a.TP + (size_t)(1 - cur) * LM;
  const double* X0 = crow + 2 * (size_t)a.TP + 2 * (size_t)LM;
  const double *LO = X0 + LM, *HI = LO + LM, *Y = HI + LM;

  __shared__ double rows[W * ROWS];
  __shared__ double Mp[NVP * (NVP + 1) / 2];
  __shared__ double fpar[MAXF * GLB_FP];
  __shared__ double s_mco[MAXF * 3];
  __shared__ double xl[WAVE], dfull[WAVE], xg[GLB_MAXG], xga[GLB_MAXG], s_ev[WAVE];
  __shared__ double s_bg;
  __shared__ int s_vb[CTR_MAX_PARAMS], s_vs[CTR_MAX_PARAMS], s_rb[CTR_MAX_PARAMS], s_rs[CTR_MAX_PARAMS];
  __shared__ int s_win[8];    // origin[3], wshape[3], valid, a size of 0
  __shared__ int s_P[W];

  if (tid == 0) glb_tables(a, n, L, NVP, s_vb, s_vs, s_rb, s_rs);
  if (tid < 8) s_win[tid] = 0;
  if (tid < GLB_MAXG) { xg[tid] = tid < G ? st[GS_XT + tid] : 0.; xga[tid] = tid < G ? st[GS_X + tid] : 0.; }
  __syncthreads();

  if (phase == GP_WRITE) {   // the result: the accepted point into the rows of the cluster's features
    for (int e = tid; e < n * NP; e += T) {
      const int i = e / NP, k = e - i * NP;
      if (s_vb[k] > GLB_CONST) a.params_out[(long long)(f0 + i) * NP + k] = glb_val(s_vb, s_vs, Xacc, xga, nullptr, k, i);
    }
    return;
  }
  // the mask centres of this round: the table's, or (a new round) the last round's positions
  for (int e = tid; e < n * 3; e += T) {
    const int i = e / 3, d = e - i * 3;
    double c = a.mco[(long long)(f0 + i) * 3 + d];
    if (phase == GP_REWINDOW) {
      c = d < ND ? glb_val(s_vb, s_vs, Xacc, xga, a.params + (long long)(f0 + i) * NP, 2 + d, i) : 0.;
      a.mco[(long long)(f0 + i) * 3 + d] = c;
    }
    s_mco[e] = c;
  }
  // the trial point of the cluster: the start, or the accepted point plus the back-substituted,
  // projected step; with it the cluster's part of the model's predicted decrease
  double pred = 0., stepmax = 0., pga = 0.;
  if (wave == 0) {
    if (phase == GP_TRIAL) {
      double dv = 0.;
      if (lane < L) {
        double s = Y[(size_t)G * LM + lane];
        for (int u = 0; u < G; ++u) s += Y[(size_t)u * LM + lane] * st[GS_DG + u];
        const double x = Xacc[lane], lo = LO[lane], hi = HI[lane];
        double t = x - s;
        t = t < lo ? lo : (t > hi ? hi : t);
        dv = t - x;
        xl[lane] = t;
        Xtr[lane] = t;
        stepmax = fabs(dv) / (fabs(x) + 1.);
        const double g = Macc[tri(nv) + lane];
        if (!glb_fixed(x, g, lo, hi)) pga = fabs(g);
      } else if (lane < nv) {
        dv = xg[lane - L] - xga[lane - L];
      }
      dfull[lane] = dv;
      wsync();
      // -(g.d + d.A d / 2) over the cluster's rows of the arrowhead (its share of the corner included)
      double acc = 0.;
      for (int i = 0; i <= nv; ++i) {
        if (lane <= i && lane < nv) {
          const double mij = Macc[tri(i) + lane];
          acc += i < nv ? mij * dfull[i] * dfull[lane] * (lane == i ? 0.5 : 1.) : mij * dfull[lane];
        }
      }
      pred = -wave_sum(acc);
      stepmax = wave_max(stepmax);
      pga = wave_max(pga);
    } else if (lane < L) {
      const double x = X0[lane];
      xl[lane] = x;
      Xtr[lane] = x;
    }
  }
  __syncthreads();

  // per-feature constants at the trial point: [0] signal, [1..3] centre, [4..6] 1 / size^2,
  // [7..9] 2 / size^3, [10 ..] the profile's parameters
  for (int i = tid; i < n; i += T) {
    const double* prow = a.params + (long long)(f0 + i) * NP;
    double* f = fpar + i * GLB_FP;
    f[0] = glb_val(s_vb, s_vs, xl, xg, prow, 1, i);
    bool zero = false;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      f[1 + d] = glb_val(s_vb, s_vs, xl, xg, prow, 2 + d, i);
      const double s = glb_val(s_vb, s_vs, xl, xg, prow, 2 + ND + (ISO ? 0 : d), i);
      zero = zero || s == 0.;
      f[4 + d] = 1. / (s * s);
      f[7 + d] = 2. / (s * s * s);
    }
    if constexpr (FIT == CTR_FIT_INV_SERIES) {
      // y = r2^N + e[1] r2^(N-1) + ... + e[N] in Horner's order over a FIXED number of NXC slots, so that the
      // pixel loop has no test on nx: slot 0 is e[0]; the series sits right-aligned in the slots 1 .. NXC - 1,
      // zeros in front of its leading 1 (slot inv_shift; with inv_shift = 0 the start value f[17] = 1 is it).
      // Leading zeros leave Horner's y and y' at exactly 0: the same operations on the same values.
      f[10] = glb_val(s_vb, s_vs, xl, xg, prow, 2 + ND + NSZ, i);
#pragma unroll 1
      for (int j = 1; j < NXC; ++j) {      // (not unrolled: every copy of glb_val's branches holds its masks in scalar registers)
        const int t = j - a.inv_shift;
        f[10 + j] = t >= 1 ? glb_val(s_vb, s_vs, xl, xg, prow, 2 + ND + NSZ + t, i) : (t == 0 ? 1. : 0.);
      }
      f[17] = a.inv_shift == 0 ? 1. : 0.;
    } else {
#pragma unroll
      for (int t = 0; t < NXC; ++t) f[10 + t] = glb_val(s_vb, s_vs, xl, xg, prow, 2 + ND + NSZ + t, i);
    }
    if (zero) s_win[7] = 1;
    if (i == 0) s_bg = glb_val(s_vb, s_vs, xl, xg, prow, 0, 0);
  }
  // masks.py:42-68 on the mask centres: the union window, clipped to the frame
  if (tid == 0) {
    long wlo[ND], whi[ND];
    bool any = false;
    for (int i = 0; i < n; ++i) {
      long ci[ND];
      bool ok = true;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        ci[d] = (long)rint(s_mco[i * 3 + d]);
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

  // The pixels are dealt in tiles of 64 to FOUR virtual waves, whatever NT: tile k belongs to virtual
  // wave k % 4, and the four partial matrices are added in the order ((A0 + A1) + A2) + A3.  The W
  // wavefronts of the workgroup take the virtual waves wave, wave + W, ...: the bytes of a cluster do
  // not depend on the instantiation, that is on the largest cluster of the call.
  constexpr int VPW = 4 / W;
  v4d acc[NTILE], tot[NTILE];
#pragma unroll
  for (int t = 0; t < NTILE; ++t) { acc[t] = v4d{0., 0., 0., 0.}; tot[t] = v4d{0., 0., 0., 0.}; }
  int P = 0;
  double* myrows = rows + wave * ROWS;
  if (s_win[6]) {
    int origin[ND], wshape[ND], radius[ND], fsh[ND];
    double inv_r2[ND];
    unsigned npix = 1;      // a window is part of a frame: fewer than 2^31 pixels (the descriptor's check)
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      origin[d] = s_win[d];
      wshape[d] = s_win[3 + d];
      radius[d] = a.radius[d];
      inv_r2[d] = 1. / ((double)radius[d] * (double)radius[d]);
      fsh[d] = (int)a.fshape[d];
      npix *= (unsigned)wshape[d];
      // (a uniform double that the pixel loop keeps: in vector registers, which have room)
      asm volatile("" : "+v"(inv_r2[d]));
    }
    const char* frame = (const char*)a.frames + (size_t)a.frame_index[cl] * (size_t)a.frame_elems * dtype_size(a.frame_dtype);
    double bg = s_bg;
    asm volatile("" : "+v"(bg));
    const int rb0 = s_rb[0];
    double* row = myrows + lane * RS;

#pragma unroll 1
    for (int vv = 0; vv < VPW; ++vv) {
    if (vv > 0) {      // W = 2: tot keeps the first of the wave's two; W = 1: the running sum in the order above
#pragma unroll
      for (int t = 0; t < NTILE; ++t) { tot[t] += acc[t]; acc[t] = v4d{0., 0., 0., 0.}; }
    }
    for (unsigned base = (unsigned)(wave + vv * W) * WAVE; base < npix; base += 4 * WAVE) {
      const unsigned p = base + lane;
      for (int j = 0; j < RS; ++j) row[j] = 0.;
      bool any = false;
      if (p < npix) {
        int idx[ND];
        unsigned q = p;
#pragma unroll
        for (int d = ND - 1; d > 0; --d) { idx[d] = (int)(q % (unsigned)wshape[d]); q /= (unsigned)wshape[d]; }
        idx[0] = (int)q;
        unsigned off = 0;      // a frame has fewer than 2^31 pixels
#pragma unroll
        for (int d = 0; d < ND; ++d) off = off * (unsigned)fsh[d] + (unsigned)(idx[d] + origin[d]);
        double res = load_pixel(frame, a.frame_dtype, off) - bg;
        for (int i = 0; i < n; ++i) {
          const double* f = fpar + i * GLB_FP;
          double rel[ND];
#pragma unroll
          for (int d = 0; d < ND; ++d) rel[d] = s_mco[i * 3 + d] - (double)origin[d];
          if (!in_mask<ND>(idx, rel, inv_r2, radius)) continue;
          any = true;
          double r2 = 0., dd[ND], dj[NPC];
#pragma unroll
          for (int k = 0; k < NPC; ++k) dj[k] = 0.;
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
            // profile_inv_dev's operations over the fixed slots (see the per-feature constants above)
            double y = f[17], dy = 0.;
#pragma unroll
            for (int j = 1; j < NXC; ++j) { dy = dy * r2 + y; y = y * r2 + f[10 + j]; }
            const double inv = 1. / y, c = -f[10] * (inv * inv);
            gv = f[10] / y;
            dg = c * dy;
            dj[2 + ND + NSZ] = -sig * inv;
            double pw = 1.;
#pragma unroll
            for (int j = NXC - 1; j >= 1; --j) { dj[2 + ND + NSZ + j] = -sig * (c * pw); pw *= r2; }
          } else {
            double qraw = 0., dge;
#pragma unroll
            for (int d = ND - 1; d >= 0; --d) qraw += dd[d] * dd[d];
            profile_dev<FIT, ND>(r2, f[10], gv, dg, dge);
            // r2_*_safe: no value within one pixel of the centre (the disc has the value 1 there)
            if (SAFE_R2 && qraw < 1.) { gv = (FIT == CTR_FIT_DISC && f[10] > 0.) ? 1. : NAN; dg = 0.; dge = 0.; }
            dj[2 + ND + NSZ] = -sig * dge;
          }
          res -= sig * gv;
          dj[1] = -gv;
          const double sdg = sig * dg;
          double q2 = 0.;
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            dj[2 + d] = sdg * (2. * dd[d] * f[4 + d]);     // dr2 / dc = -2 dd / size^2
            if (ISO) q2 += dd[d] * dd[d];
            else dj[2 + ND + d] = sdg * (dd[d] * dd[d] * f[7 + d]);
          }
          if (ISO) dj[2 + ND] = sdg * (q2 * f[7]);
#pragma unroll
          for (int k = 1; k < NPC; ++k) {
            double* e = row + s_rb[k] + s_rs[k] * i;
            *e += dj[k] == dj[k] ? dj[k] : 0.;
          }
        }
        if (any) {
          if (res == res) {   // nansum (fitfunc.py:449,483): a NaN pixel is left out and still counts in P
            row[rb0] -= 1.;
            row[nv] = res;
          } else {
            for (int j = 0; j <= nv; ++j) row[j] = 0.;
          }
        }
      }
      const unsigned long long bal = __ballot(any);
      P += __popcll(bal);
      wsync();
      if (bal != 0ull) {
        const int kr = lane >> 4, cc = lane & 15;
        const double* rbase = myrows + kr * RS + cc;
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
          double val[NT];
#pragma unroll
          for (int t = 0; t < NT; ++t) val[t] = rbase[4 * s * RS + 16 * t];
          int tt = 0;
#pragma unroll
          for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj <= ti; ++tj) {
              acc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(val[ti], val[tj], acc[tt], 0, 0, 0);
              ++tt;
            }
        }
      }
      wsync();
    }
    }
  }
  // the partial accumulators meet in LDS: wave w parks its tiles in its own row tile, wave 0 adds
  // them in the order of the virtual waves
  if (W > 1) {
    if (wave != 0) {
#pragma unroll
      for (int t = 0; t < NTILE; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (W == 2) {      // virtual waves 1 (tot) and 3 (acc)
            myrows[(t * 4 + r) * WAVE + lane] = tot[t][r];
            myrows[((NTILE + t) * 4 + r) * WAVE + lane] = acc[t][r];
          } else {
            myrows[(t * 4 + r) * WAVE + lane] = acc[t][r];
          }
        }
    }
    if (lane == 0) s_P[wave] = P;
    __syncthreads();
  }
  if (wave == 0) {
    if (W == 1) {
#pragma unroll
      for (int t = 0; t < NTILE; ++t) acc[t] = tot[t] + acc[t];
    } else if (W == 2) {      // tot = A0, acc = A2; wave 1 parked A1 and A3
      const double* pr = rows + ROWS;
#pragma unroll
      for (int t = 0; t < NTILE; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double x = tot[t][r] + pr[(t * 4 + r) * WAVE + lane];
          x += acc[t][r];
          x += pr[((NTILE + t) * 4 + r) * WAVE + lane];
          acc[t][r] = x;
        }
      P += s_P[1];
    } else {
#pragma unroll
      for (int ww = 1; ww < W; ++ww) {
        const double* pr = rows + ww * ROWS;
#pragma unroll
        for (int t = 0; t < NTILE; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[t][r] += pr[(t * 4 + r) * WAVE + lane];
        P += s_P[ww];
      }
    }
    // every entry weighted by 1 / (P_c norm); D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
    const double scale = P > 0 ? 1. / ((double)P * st[GS_NORM]) : 0.;
    const int cc = lane & 15, r0 = lane >> 4;
    int tt = 0;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
      for (int tj = 0; tj <= ti; ++tj) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = 16 * ti + r0 + 4 * r, gj = 16 * tj + cc;
          if (gi >= gj && gi <= nv) Mp[tri(gi) + gj] = acc[tt][r] * scale;
        }
        ++tt;
      }
    wsync();
    if (lane == 0 && s_win[7]) Mp[tri(nv) + nv] = NAN;   // a size of 0: no valid model
    wsync();
    // the cluster's row of the evaluation table
    double pgt = 0.;
    if (lane < L) {
      const double g = Mp[tri(nv) + lane];
      if (!glb_fixed(xl[lane], g, LO[lane], HI[lane])) pgt = fabs(g);
    }
    pgt = wave_max(pgt);
    s_ev[lane] = 0.;
    wsync();
    if (lane == 0) {
      s_ev[0] = Mp[tri(nv) + nv]; s_ev[1] = (double)P; s_ev[2] = pred; s_ev[3] = stepmax; s_ev[4] = pga; s_ev[5] = pgt;
    }
    if (lane < G) {
      s_ev[8 + lane] = Mp[tri(nv) + L + lane];
      for (int v = 0; v <= lane; ++v) s_ev[16 + tri(lane) + v] = Mp[tri(L + lane) + L + v];
    }
    wsync();
    if (lane < GLB_EK) a.ev[cl * GLB_EK + lane] = s_ev[lane];
  }
  __syncthreads();
  const int ne = (nv + 1) * (nv + 2) / 2;
  for (int e = tid; e < ne; e += T) Mtr[e] = Mp[e];
}

// One wavefront per cluster.  GP_FACTOR: with the accepted point's A_c, B_c, g_c and the problem's mu,
// Y = (A_c + mu D_c)^-1 [B_c g_c] on the free locals (a fixed local is an identity row with a zero
// right-hand side), kept in the cluster's row for the back-substitution, and the Schur row.
// GP_CHECK: whether a feature is max_shift or more from its mask centre.
__global__ __launch_bounds__(WAVE) void global_factor_kernel(GlbArgs a) {
  const long long cl = blockIdx.x;
  const int prob = a.prob_of[cl];
  if (prob < 0 || a.done[prob]) return;
  const double* st = a.state + (long long)prob * GS_SIZE;
  const int phase = (int)st[GS_PHASE];
  if (phase != GP_FACTOR && phase != GP_CHECK) return;
  const int lane = threadIdx.x;
  const int NP = a.n_params, G = a.G, LM = a.LM;
  const int f0 = a.feat_offset[cl];
  const int n = a.feat_offset[cl + 1] - f0;
  const int L = a.ncl + n * a.nvar, nv = L + G;
  const int cur = (int)st[GS_CUR];
  double* crow = a.rows + cl * a.row_stride;
  const double* Macc = crow + (size_t)cur * a.TP;
  const double* Xacc = crow + 2 * (size_t)a.TP + (size_t)cur * LM;
  const double* LO = crow + 2 * (size_t)a.TP + 3 * (size_t)LM;
  const double* HI = LO + LM;
  double* Y = crow + 2 * (size_t)a.TP + 5 * (size_t)LM;

  __shared__ double Mp[GLB_TPMAX], H[GLB_TPMAX], rhs[(GLB_MAXG + 1) * GLB_MAXNV], dinv[GLB_MAXNV], s_out[WAVE], xga[GLB_MAXG];
  __shared__ int s_vb[CTR_MAX_PARAMS], s_vs[CTR_MAX_PARAMS], s_rb[CTR_MAX_PARAMS], s_rs[CTR_MAX_PARAMS];
  __shared__ int s_fix[WAVE];

  if (phase == GP_CHECK) {
    if (lane == 0) glb_tables(a, n, L, 0, s_vb, s_vs, s_rb, s_rs);
    if (lane < GLB_MAXG) xga[lane] = lane < G ? st[GS_X + lane] : 0.;
    wsync();
    bool moved = false;
    const double ms2 = a.max_shift * a.max_shift;
    for (int i = lane; i < n; i += WAVE) {
      double d2 = 0.;
      for (int d = 0; d < a.ndim; ++d) {
        const double t = glb_val(s_vb, s_vs, Xacc, xga, a.params + (long long)(f0 + i) * NP, 2 + d, i) -
                         a.mco[(long long)(f0 + i) * 3 + d];
        d2 += t * t;
      }
      if (!(d2 < ms2)) moved = true;   // refine.py:384
    }
    const bool any = __ballot(moved) != 0ull;
    if (lane < GLB_SK) a.sch[cl * GLB_SK + lane] = (lane == 44 && any) ? 1. : 0.;
    return;
  }

  const int ne = (nv + 1) * (nv + 2) / 2;
  for (int e = lane; e < ne; e += WAVE) Mp[e] = Macc[e];
  const double mu = st[GS_MU];
  wsync();
  s_fix[lane] = lane < L ? (glb_fixed(Xacc[lane], Mp[tri(nv) + lane], LO[lane], HI[lane]) ? 1 : 0) : 1;
  wsync();
  for (int i = 0; i < L; ++i) {
    if (lane <= i) {
      double h;
      if (s_fix[i] || s_fix[lane]) h = lane == i ? 1. : 0.;
      else {
        h = Mp[tri(i) + lane];
        if (lane == i) h += mu * (h > 1e-300 ? h : 1.);   // Marquardt scaling by the Gauss-Newton diagonal
      }
      H[tri(i) + lane] = h;
    }
  }
  for (int u = 0; u <= G; ++u)
    if (lane < L) rhs[u * GLB_MAXNV + lane] = s_fix[lane] ? 0. : Mp[tri(L + u) + lane];   // u = G: row nv, the gradient
  wsync();
  const bool ok = chol_factor_w(H, dinv, L, lane);
  if (ok) chol_solve_w(H, dinv, L, rhs, G + 1, GLB_MAXNV, lane);
  wsync();
  for (int u = 0; u <= G; ++u)
    if (lane < L) Y[(size_t)u * LM + lane] = rhs[u * GLB_MAXNV + lane];
  // S_c = G_c - B_c^T Y, the reduced gradient g_g,c - B_c^T y_g: lane (u, v) of the packed corner
  s_out[lane] = 0.;
  wsync();
  if (lane < G * (G + 1) / 2 + G) {
    int u, v;
    if (lane < G * (G + 1) / 2) {
      u = 0;
      while (tri(u + 1) <= lane) ++u;
      v = lane - tri(u);
    } else {
      u = lane - G * (G + 1) / 2;
      v = G;
    }
    // v < G: entry (u, v) of S_c; v = G: entry u of the reduced gradient
    double s = v < G ? Mp[tri(L + u) + L + v] : Mp[tri(nv) + L + u];
    for (int i = 0; i < L; ++i) s -= Mp[tri(L + u) + i] * rhs[v * GLB_MAXNV + i];
    s_out[v < G ? tri(u) + v : 36 + u] = s;
  }
  if (lane == 0) s_out[44] = ok ? 0. : 1.;
  wsync();
  if (lane < GLB_SK) a.sch[cl * GLB_SK + lane] = s_out[lane];
}

// Cholesky factor of the leading n x n block of H (row-major, leading dimension GLB_MAXG, lower
// triangle), in place; false where it is not positive definite
__device__ inline bool glb_cholesky(double* H, int n) {
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j <= i; ++j) {
      double t = H[i * GLB_MAXG + j];
      for (int k = 0; k < j; ++k) t -= H[i * GLB_MAXG + k] * H[j * GLB_MAXG + k];
      if (i == j) {
        if (!(t > 0.) || !isfinite(t)) return false;
        H[i * GLB_MAXG + i] = sqrt(t);
      } else {
        H[i * GLB_MAXG + j] = t / H[j * GLB_MAXG + j];
      }
    }
  }
  return true;
}

__device__ inline void glb_chol_solve(const double* H, int n, double* x) {
  for (int i = 0; i < n; ++i) {
    double t = x[i];
    for (int k = 0; k < i; ++k) t -= H[i * GLB_MAXG + k] * x[k];
    x[i] = t / H[i * GLB_MAXG + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double t = x[i];
    for (int k = i + 1; k < n; ++k) t -= H[k * GLB_MAXG + i] * x[k];
    x[i] = t / H[i * GLB_MAXG + i];
  }
}

// the rows of the clusters c0 + j, c0 + j + GLB_R, ... of column k in that order, then the GLB_R
// partial results in order; a column of `maxcols` (bit k) is a maximum, every other one a sum
__device__ __forceinline__ void glb_reduce(const double* table, int K, long long c0, long long c1, unsigned long long maxcols,
                                           double (*red)[WAVE], double* tot, int tid) {
  const int k = tid & 63, j = tid >> 6;
  const bool is_max = ((maxcols >> k) & 1ull) != 0ull;
  double acc = 0.;
  if (k < K)
    for (long long c = c0 + j; c < c1; c += GLB_R) {
      const double t = table[c * K + k];
      acc = is_max ? fmax(acc, t) : acc + t;
    }
  red[j][k] = acc;
  __syncthreads();
  if (tid < K) {
    double t = red[0][tid];
#pragma unroll
    for (int r = 1; r < GLB_R; ++r) t = is_max ? fmax(t, red[r][tid]) : t + red[r][tid];
    tot[tid] = t;
  }
  __syncthreads();
}

// the end of a round's minimisation without a result: the iteration limit
__device__ __forceinline__ int glb_at_limit(double gain) { return gain <= CTR_STALL_TOL ? 1 : 2; }

// One workgroup per problem, behind global_eval_kernel: F, the predicted decrease, the step, the
// projected gradients and the corner of the trial, summed over the clusters; then the bookkeeping
// of the bounded LM as train_step_kernel does it.
__global__ __launch_bounds__(GLB_PROB_THREADS) void global_judge_kernel(GlbArgs a) {
  const long long p = blockIdx.x;
  if (a.done[p]) return;
  const int tid = threadIdx.x;
  __shared__ double red[GLB_R][WAVE];
  __shared__ double tot[WAVE];
  __shared__ double st[GS_SIZE];
  __shared__ int s_empty;
  const int phase = (int)a.state[p * GS_SIZE + GS_PHASE];
  if (phase == GP_FACTOR || phase == GP_CHECK) return;
  const long long c0 = a.problem_offset[p], c1 = a.problem_offset[p + 1];
  if (tid == 0) s_empty = 0;
  if (tid < GS_SIZE) st[tid] = a.state[p * GS_SIZE + tid];
  __syncthreads();
  const bool evaluated = phase == GP_EVAL0 || phase == GP_REWINDOW || phase == GP_TRIAL;
  if (evaluated) {
    glb_reduce(a.ev, GLB_EK, c0, c1, (1ull << 3) | (1ull << 4) | (1ull << 5), red, tot, tid);
    bool none = false;
    for (long long c = c0 + tid; c < c1; c += GLB_PROB_THREADS) none = none || !(a.ev[c * GLB_EK + 1] > 0.);
    if (none) atomicOr(&s_empty, 1);
    __syncthreads();
  }
  if (tid == 0) {
    const int G = a.G;
    const double xtol = a.xtol > 0. ? a.xtol : 1e-9, ftol = a.ftol > 0. ? a.ftol : 1e-14;
    double S = st[GS_S], mu = st[GS_MU], nu = st[GS_NU], gain = st[GS_GAIN];
    int it = (int)st[GS_IT];
    bool last_acc = st[GS_LAST] != 0.;
    int finished = 0;     // 1 the round's minimisation has ended, 2 failed
    int status = CTR_STATUS_OK;
    bool take = false;
    const double St = evaluated ? tot[0] : 0.;

    if (phase == GP_WRITE) {
      glb_finish(a, p, st, CTR_STATUS_OK, st[GS_COST]);
    } else if (phase == GP_EVAL0 || phase == GP_REWINDOW) {
      if (s_empty) { finished = 2; status = CTR_STATUS_OUT_OF_BOUNDS; }
      else if (!isfinite(St)) { finished = 2; status = CTR_STATUS_NO_CONVERGENCE; }
      S = St; mu = 1.; nu = 2.; gain = INFINITY; last_acc = true; it = 0;
      take = true;
    } else if (phase == GP_TRIAL) {
      const double pred = tot[2];
      double stepmax = tot[3], pg = tot[4], pgt = tot[5];
      for (int v = 0; v < G; ++v) {
        const double lo = st[GS_LO + v], hi = st[GS_HI + v];
        const double x = st[GS_X + v], gx = st[GS_G + v], xn = st[GS_XT + v], gn = tot[8 + v];
        const double rel = fabs(xn - x) / (fabs(x) + 1.);
        stepmax = rel > stepmax ? rel : stepmax;
        if (!glb_fixed(x, gx, lo, hi)) pg = fmax(pg, fabs(gx));
        if (!glb_fixed(xn, gn, lo, hi)) pgt = fmax(pgt, fabs(gn));
      }
      if ((last_acc && stepmax <= xtol) || fabs(pred) <= ftol * (0.5 * S) + 1e-300) {
        finished = 1;     // converged at the accepted point; the trial is not looked at
      } else {
        const double act = 0.5 * (S - St);
        // the flat-trial rule (include/ctrefine.h, training): a trial whose F cannot be told from
        // the accepted point's is judged by the projected gradient
        const bool flat_better = isfinite(St) && pred > 0. && !(act > 0.) &&
                                 fabs(act) <= 16. * 2.220446049250313e-16 * S && pgt < pg;
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
    }
    if (take && finished != 2) {
      for (int v = 0; v < G; ++v) {
        st[GS_X + v] = st[GS_XT + v];
        st[GS_G + v] = tot[8 + v];
      }
      for (int e = 0; e < G * (G + 1) / 2; ++e) st[GS_A + e] = tot[16 + e];
      st[GS_CUR] = 1. - st[GS_CUR];
    }
    if (phase != GP_WRITE) {
      if (!finished && it >= a.maxiter) {   // a stationary objective at the limit counts as converged
        finished = glb_at_limit(gain);
        status = finished == 1 ? CTR_STATUS_OK : CTR_STATUS_NO_CONVERGENCE;
      }
      st[GS_S] = S; st[GS_MU] = mu; st[GS_NU] = nu; st[GS_GAIN] = gain;
      st[GS_IT] = (double)it; st[GS_LAST] = last_acc ? 1. : 0.;
      st[GS_PHASE] = finished == 1 ? GP_CHECK : GP_FACTOR;
      if (finished) { st[GS_NIT] += (double)it; st[GS_IT] = 0.; }
      if (finished == 2) { st[GS_ROUND] += 1.; glb_finish(a, p, st, status, NAN); }
    }
  }
  __syncthreads();
  if (tid < GS_SIZE) a.state[p * GS_SIZE + tid] = st[tid];
}

// One workgroup per problem, behind global_factor_kernel.  GP_FACTOR: the Schur rows and reduced
// gradients of the clusters summed, (S + mu diag(corner)) d_g = -g on the free shared variables, the
// projected trial.  A cluster or a corner that is not positive definite spends the iteration here
// (more damping, no pixel pass).  GP_CHECK: the round has ended; another one, or the result.
__global__ __launch_bounds__(GLB_PROB_THREADS) void global_solve_kernel(GlbArgs a) {
  const long long p = blockIdx.x;
  if (a.done[p]) return;
  const int tid = threadIdx.x;
  __shared__ double red[GLB_R][WAVE];
  __shared__ double tot[WAVE];
  __shared__ double st[GS_SIZE];
  __shared__ double H[GLB_MAXG * GLB_MAXG], w[GLB_MAXG];
  __shared__ int fr[GLB_MAXG];
  const int phase = (int)a.state[p * GS_SIZE + GS_PHASE];
  if (phase != GP_FACTOR && phase != GP_CHECK) return;
  const long long c0 = a.problem_offset[p], c1 = a.problem_offset[p + 1];
  if (tid < GS_SIZE) st[tid] = a.state[p * GS_SIZE + tid];
  glb_reduce(a.sch, GLB_SK, c0, c1, 0ull, red, tot, tid);
  if (tid == 0) {
    const int G = a.G;
    if (phase == GP_CHECK) {
      const bool moved = tot[44] > 0.;
      st[GS_ROUND] += 1.;
      if (!moved || (int)st[GS_ROUND] >= a.max_rounds) {
        const double cost = sqrt(st[GS_S] / a.residual_factor);
        bool finite = isfinite(cost);
        for (int v = 0; v < G; ++v) finite = finite && isfinite(st[GS_X + v]);
        if (!finite) glb_finish(a, p, st, CTR_STATUS_NO_CONVERGENCE, NAN);
        else if (cost > a.max_rms_dev) glb_finish(a, p, st, CTR_STATUS_RMS_DEV, NAN);
        else { st[GS_COST] = cost; st[GS_PHASE] = GP_WRITE; }
      } else {
        for (int v = 0; v < G; ++v) st[GS_XT + v] = st[GS_X0 + v];
        st[GS_PHASE] = GP_REWINDOW;
      }
    } else {
      double mu = st[GS_MU], nu = st[GS_NU];
      int nf = 0;
      for (int v = 0; v < G; ++v)
        if (!glb_fixed(st[GS_X + v], st[GS_G + v], st[GS_LO + v], st[GS_HI + v])) fr[nf++] = v;
      bool reject = tot[44] > 0.;
      if (!reject) {
        for (int r = 0; r < nf; ++r) {
          for (int c = 0; c <= r; ++c) H[r * GLB_MAXG + c] = tot[tri(fr[r]) + fr[c]];
          const double d = st[GS_A + tri(fr[r]) + fr[r]];
          H[r * GLB_MAXG + r] += mu * (d > 1e-300 ? d : 1.);
          w[r] = tot[36 + fr[r]];
        }
        reject = !glb_cholesky(H, nf);
      }
      if (!reject) {
        glb_chol_solve(H, nf, w);
        for (int v = 0; v < G; ++v) st[GS_DG + v] = 0.;
        for (int r = 0; r < nf; ++r) st[GS_DG + fr[r]] = -w[r];
        for (int v = 0; v < G; ++v) {
          const double t = st[GS_X + v] + st[GS_DG + v], lo = st[GS_LO + v], hi = st[GS_HI + v];
          st[GS_XT + v] = t < lo ? lo : (t > hi ? hi : t);
        }
        st[GS_PHASE] = GP_TRIAL;
      } else {
        mu *= nu;
        nu *= 2.;
        st[GS_MU] = mu; st[GS_NU] = nu; st[GS_LAST] = 0.;
        st[GS_IT] += 1.;
        st[GS_PHASE] = GP_SKIP;
        if (mu > 1e30) {
          st[GS_NIT] += st[GS_IT];
          st[GS_ROUND] += 1.;
          glb_finish(a, p, st, CTR_STATUS_NO_CONVERGENCE, NAN);
        }
      }
    }
  }
  __syncthreads();
  if (tid < GS_SIZE) a.state[p * GS_SIZE + tid] = st[tid];
}

#endif  // CTREFINE_GLOBAL_KERNELS_H
