// block_kernel.h -- refine_block_kernel: W wavefronts per cluster, LDS row tiles + f64 MFMA
// Part of the MI355X cluster-refinement engine; included by ctrefine.hip inside its
// anonymous namespace (device code only, gfx950).
#ifndef CTREFINE_BLOCK_KERNEL_H
#define CTREFINE_BLOCK_KERNEL_H

// ---- generic clusters: one workgroup of W wavefronts per cluster ------------------------
//
// Any number of features / any parameter modes / constraints.  The W waves split
// the 64-pixel tiles of the window among themselves; each builds Jacobian rows in
// its own LDS row tile and contracts them with v_mfma_f64_16x16x4_f64 into
// register accumulators of the augmented matrix [J r]^T [J r]; the partial
// accumulators meet in LDS, wave 0 runs the bounded / constrained LM step on the
// sum (cooperative Cholesky on LDS) and publishes the next trial vector.  Two
// workgroup barriers per solver iteration.  W = 4 (NT <= 3), 2 (NT <= 6), 1.

__device__ __forceinline__ void wsync() {
  // LDS ordering inside ONE wavefront (DS operations of a wave execute in order)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}


// ---- register-resident Cholesky step for small systems (one matrix column per lane) ----
//
// Lane c < NR holds column c of the damped normal matrix with the active set
// folded in (fixed variables and unused rows are identity rows).  Right-looking
// Cholesky: at step j the pivot column is broadcast row by row with v_readlane,
// every later column updates itself from its own (symmetric) entry col[j]; the
// right-hand side rides along as one more row, so the forward substitution is
// free.  The back substitution broadcasts each solved component once.  No LDS
// round trips, no dynamic register indexing.  Returns false if not positive definite.
// 1/sqrt(x) to double precision: hardware estimate + two Newton steps (the
// correctly rounded sqrt and division cost ~60 dependent instructions per pivot)
__device__ __forceinline__ double fast_rsqrt(double x) {
  double r = __builtin_amdgcn_rsq(x);
  r = r * fma(-0.5 * x * r, r, 1.5);
  r = r * fma(-0.5 * x * r, r, 1.5);
  return r;
}

__device__ __forceinline__ double readlane_f64(double x, int srclane) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), srclane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), srclane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// a value that is the same in every lane, moved to scalar registers (the kernel's loop-invariant
// doubles would otherwise each hold two vector registers for the whole kernel)
__device__ __forceinline__ double uniform_f64(double x) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffLL));
  const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// nwt: add the exact second-order part.  qk[kr] is the entry between this lane's variable
// and the variable of kind kr (0 signal, 1 + a position) of the same feature; ic = vinfo[c].
template <int NR, int NK>
__device__ __forceinline__ bool column_solve(const double* Mp, int nv, double mu, bool is_free,
                                             int lane, double& x_own, bool nwt, const int* vinfo,
                                             int ic, const double (&qk)[NK]) {
  // the lane's addresses below are invariant in the loops around the call (the kernel's phase loop,
  // the step's attempts): an opaque copy of the lane index keeps the compiler from hoisting all NR
  // of them out of those (they would be carried through the pixel pass in registers, or spilled)
  int c = lane;
  asm volatile("" : "+v"(c));
  const bool colv = c < nv && is_free;
  const unsigned long long fmask = __ballot(colv);
  double col[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const bool rowv = ((fmask >> i) & 1ull) != 0ull;
    double x = 0., xq = 0.;
    if (rowv && colv) x = Msym(Mp, i + 1, c + 1);
    if (nwt) {
      const int ir = vinfo[i];   // same address in every lane
      const int kr = (ir & 7) - 1;
      double q = qk[0];
#pragma unroll
      for (int t = 1; t < NK; ++t) q = kr == t ? qk[t] : q;
      xq = (rowv && colv && ic >= 0 && ((ir ^ ic) >> 3) == 0 && kr >= 0) ? q : 0.;
    }
    // Marquardt scaling by the Gauss-Newton diagonal in both models
    if (i == c) x = colv ? x + xq + mu * (x > 1e-300 ? x : 1.) : 1.;
    else x += xq;
    col[i] = x;
  }
  double y = colv ? Mp[tri(c + 1)] : 0.;
  double mydinv = 1., yown = 0.;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    if (j < nv && ok) {  // rows beyond the variables are identity: nothing to eliminate; a failed
                         // pivot ends the factorisation (both conditions are wave-uniform)
      const double dj = readlane_f64(col[j], j);
      if (!(dj > 0.) || !isfinite(dj)) ok = false;
      const double dinv = fast_rsqrt(dj);
      const double lkj = c > j ? col[j] * dinv : 0.;  // L[c][j] for the columns still open
      const double yj = readlane_f64(y, j) * dinv;
      if (c == j) { mydinv = dinv; yown = yj; }
#pragma unroll
      for (int i = j + 1; i < NR; ++i) {
        const double lij = readlane_f64(col[i], j) * dinv;
        col[i] -= lij * lkj;
      }
      y -= yj * lkj;
    }
  }
  double s = 0.;
  x_own = 0.;
#pragma unroll
  for (int j = NR - 1; j >= 0; --j) {
    if (j < nv && ok) {
      const double xj = readlane_f64((yown - s) * mydinv, j);
      if (c == j) x_own = xj;
      s += (c < j ? col[j] * mydinv : 0.) * xj;
    }
  }
  return ok;
}

// Internal column order of the block kernel's [r J] matrix: column 0 is the
// residual, then the shared variables (background, any 'cluster'-mode column), then
// the per-feature variables FEATURE-MAJOR, so that a feature occupies one (at most
// two) 16-column MFMA blocks and a pixel tile only pays for the blocks of its
// candidate features.  Variable c lives in column c + 1.  (The reference's
// parameter-major order, fitfunc.py:207-263, is an external convention only: the
// engine's inputs and outputs are parameter tables.)
struct LayoutB {
  int n, nv, nshared, npf;
  int slot[CTR_MAX_PARAMS];     // rank among the shared / per-feature variables, -1 if constant
  int per_feat[CTR_MAX_PARAMS];
  __device__ __forceinline__ int vidx(int kk, int i) const {
    return slot[kk] < 0 ? -1 : (per_feat[kk] ? nshared + i * npf + slot[kk] : slot[kk]);
  }
  // vidx for a parameter column known only at run time (or different in every lane): selected
  // from the unrolled compile-time cases, so that slot / per_feat are never indexed at run time
  // (a runtime index puts the whole layout in per-lane scratch memory)
  __device__ __forceinline__ int vidx_any(int kk, int i) const {
    int b = -1;
#pragma unroll
    for (int t = 0; t < CTR_MAX_PARAMS; ++t) b = kk == t ? vidx(t, i) : b;
    return b;
  }
  // bit mask of the 16-column blocks that hold the columns of feature i
  __device__ __forceinline__ unsigned blocks(int i) const {
    if (npf == 0) return 0u;
    const int c0 = 1 + nshared + i * npf, c1 = c0 + npf - 1;
    return (1u << (c0 >> 4)) | (1u << (c1 >> 4));
  }
};

__device__ __forceinline__ void make_layout_b(const ctr_problem& p, int n, LayoutB& L) {
  int ns = 0, np = 0;
  L.n = n;
#pragma unroll
  for (int k = 0; k < CTR_MAX_PARAMS; ++k) {
    const int m = k < p.n_params ? p.modes[k] : CTR_MODE_CONST;
    if (m == CTR_MODE_CONST) { L.slot[k] = -1; L.per_feat[k] = 0; }
    else if (m == CTR_MODE_VAR) { L.slot[k] = np++; L.per_feat[k] = 1; }
    else { L.slot[k] = ns++; L.per_feat[k] = 0; }
  }
  L.nshared = ns;
  L.npf = np;
  L.nv = ns + n * np;
}

constexpr int QT = 9;  // second-order entries kept per feature: ND (signal, pos_a) + ND(ND+1)/2 (pos_a, pos_b)

template <int NT, int W, bool CONS = false>
struct SmemB {
  static constexpr int NVP = 16 * NT;
  static constexpr int RS = NVP + 1;
  static constexpr int NTILE = NT * (NT + 1) / 2;
  static constexpr int NF = NVP < MAXF ? NVP : MAXF;
  // constraint Jacobians: constrained clusters have 2..4 features = at most 29 variables (NT <= 2)
  static constexpr int NVC = NT <= 2 ? NVP : 1;
  static constexpr int ROWS = WAVE * RS;               // one wave's row tile
  static constexpr int o_rows = 0;                      // W row tiles; tile 0 doubles as packed H
  static constexpr int o_M = o_rows + W * ROWS;
  static constexpr int o_v = o_M + NVP * (NVP + 1) / 2;
  static constexpr int o_vt = o_v + NVP;
  static constexpr int o_v0 = o_vt + NVP;
  static constexpr int o_lo = o_v0 + NVP;
  static constexpr int o_hi = o_lo + NVP;
  static constexpr int o_dl = o_hi + NVP;
  static constexpr int o_w = o_dl + NVP;
  static constexpr int o_cur = o_w + NVP;
  static constexpr int o_mco = o_cur + NF * CTR_MAX_PARAMS;
  static constexpr int o_fpar = o_mco + NF * 3;
  static constexpr int o_Cj = o_fpar + NF * FP;
  static constexpr int o_Cjt = o_Cj + MAXC * NVC;
  static constexpr int o_Y = o_Cjt + MAXC * NVC;
  static constexpr int o_small = o_Y + MAXC * NVC;      // cv[6] cvt[6] mult[6] . Sc[36] flag
  static constexpr int o_fr = o_small + 64;
  static constexpr int o_part = o_fr + NVP / 2 + 2;     // per wave: S, P
  static constexpr int o_ctl = o_part + 2 * W;          // ints: phase, origin[3], wshape[3]
  // second-order entries of the current point, QT per feature (features with >= 3 variables each)
  static constexpr int NFQ = (NVP + 2) / 3 < MAXF ? (NVP + 2) / 3 : MAXF;
  static constexpr int o_uc = o_ctl + 8;
  static constexpr int o_vinfo = o_uc + NFQ * QT;       // ints: 8 * feature + kind + 1 of every variable
  static constexpr int o_cpair = o_vinfo + NVP / 2;     // ints: pair behind constraint r (current, trial)
  // constrained fits (cons_qp): 1/diag of the factor, gradient of the model, and the
  // second-order part in all variables as a packed triangle (non-default modes)
  static constexpr int o_qd = o_cpair + MAXC;
  static constexpr int o_gq = o_qd + (CONS ? NVP : 0);
  static constexpr int o_Qp = o_gq + (CONS ? NVP : 0);
  static constexpr int total = o_Qp + (CONS ? NVP * (NVP + 1) / 2 : 0);
  static constexpr size_t bytes = (size_t)total * sizeof(double);
  static_assert(W == 1 || NTILE * 256 + 6 * WAVE <= ROWS, "partial accumulators must fit a row tile");
};

enum { BP_EVAL_INIT = 1, BP_EVAL_TRIAL = 2, BP_STEP_ONLY = 3, BP_FINISH = 4 };

// in-place Cholesky of a packed lower-triangular matrix in LDS by ONE wave.
// Right-looking: per column one reciprocal square root, then the trailing
// update spread over the lanes as an 8 x 8 grid of (row, column) entries, so a
// lane does ~(nf - j)^2 / 128 multiply-subtracts per column instead of nf - j.
// dinv[j] = 1 / L[j][j] is kept for the substitutions.
__device__ bool chol_factor_w(double* Hp, double* dinv, int nf, int lane) {
  const int ty = lane >> 3, tx = lane & 7;
  for (int j = 0; j < nf; ++j) {
    const double d = Hp[tri(j) + j];
    if (!(d > 0.) || !isfinite(d)) return false;
    const double inv = fast_rsqrt(d);
    wsync();
    for (int i = j + 1 + lane; i < nf; i += WAVE) Hp[tri(i) + j] *= inv;
    if (lane == 0) { Hp[tri(j) + j] = d * inv; dinv[j] = inv; }
    wsync();
    for (int i = j + 1 + ty; i < nf; i += 8) {
      const double lij = Hp[tri(i) + j];
      double* ri = Hp + tri(i);
      for (int kk = j + 1 + tx; kk <= i; kk += 8) ri[kk] -= lij * Hp[tri(kk) + j];
    }
    wsync();
  }
  return true;
}

// solve L L^T x = b in place for nrhs right-hand sides x[r*ldx + i]
__device__ void chol_solve_w(const double* Lp, const double* dinv, int nf, double* x, int nrhs,
                             int ldx, int lane) {
  for (int j = 0; j < nf; ++j) {
    const double dj = dinv[j];
    for (int r = 0; r < nrhs; ++r) {
      const double yj = x[r * ldx + j] * dj;
      for (int i = j + 1 + lane; i < nf; i += WAVE) x[r * ldx + i] -= Lp[tri(i) + j] * yj;
      if (lane == 0) x[r * ldx + j] = yj;
    }
    wsync();
  }
  for (int j = nf - 1; j >= 0; --j) {
    const double dj = dinv[j];
    for (int r = 0; r < nrhs; ++r) {
      const double xj = x[r * ldx + j] * dj;
      for (int i = lane; i < j; i += WAVE) x[r * ldx + i] -= Lp[tri(j) + i] * xj;
      if (lane == 0) x[r * ldx + j] = xj;
    }
    wsync();
  }
}

#ifdef CTR_STAMPS
__device__ unsigned long long g_stamps[16];
#define STAMP(slot) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    if (wave == 0 && lane == 0) atomicAdd(&g_stamps[slot], now_ - t_prev_); t_prev_ = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define STAMP(slot) do {} while (0)
#endif

// CONS: the instantiation that takes the clusters with equality constraints (dimers, trimers,
// tetramers: at most 29 variables, NT <= 2); in the others the constrained code is compiled out
// (it costs the unconstrained fits registers otherwise: 700 B of scratch per lane, measured).
// LP: the instantiation for problems with a lowpass of the window (ctr_problem.noise_size): every
// pixel value is the filtered one, computed from the raw frame where it is needed.
// FIT: the radial profile (CTR_FIT_GAUSS / RING / DISC / INV_SERIES; device_common.h:profile_dev,
// profile_inv_dev); ring and disc carry one more parameter column (thickness / disc_size),
// inv_series_<N> N + 1 (signal_mult, param_a, ...); all three iterate with the Gauss-Newton model.
// Minimum wavefronts per SIMD asked of the compiler (the register budget) for the instantiations
// of the throughput scheduling (2D, fewest wavefronts per cluster: W = 2 for NT <= 2, 1 above).
// NT = 1 (3-4 features): 3 -- 168 VGPRs and no scratch (2D iso and aniso; tests/test_kernel_resources.py).
// A third wavefront per SIMD gave +6 % on cfg 2 with ten batches in flight even while it spilled
// (168 VGPRs + 296 B; interleaved A/B, tools/ab_bench.sh: 48.4 -> 51.4 M fits/s): the kernel waits
// on dependent FP64 chains.  The spills were not the step's working set but values the compiler
// hoisted out of the phase loop (per-lane LDS addresses, the layout in scratch through a runtime
// index, a few invariant doubles); see `lane` at the top of the loop and LayoutB::vidx_any.
// 4 per SIMD buys nothing here: 26.6 KB of LDS per workgroup already limit a CU to 6 workgroups
// (3 wavefronts per SIMD), and the compiler spills again at 128 VGPRs.
// NT = 2 and NT = 3-4 ask for 1, as every other instantiation does.
constexpr int block_occ(int nt, int w, bool cons, bool lp, int fit) {
  return (cons || lp || fit != 0) ? 1 : (nt == 1 && w == 2) ? 3 : 1;
}
// One workgroup per cluster of the bin.  k.split != nullptr (a plan with a tail launch,
// ctrefine.hip): the first min(*k.split, k.split_cap) entries of the bin are fitted by
// refine_tail_kernel, their workgroups have nothing to do here.
//
// The statements of the fit are in block_kernel_body.inc; refine_tail_kernel (tail_kernel.h)
// includes the same text -- text and not a function for the reason given in small_kernel.h.  It
// expects, in scope: ND, ISO, NT, W, CONS, LP, FIT; k; cl (the cluster); tid (thread of the
// workgroup of W wavefronts); smem (SmemB<NT, W, CONS>::bytes of LDS of the workgroup).
template <int ND, bool ISO, int NT, int W, bool CONS, bool LP = false, int FIT = 0>
__global__ void __launch_bounds__(WAVE * W, (block_occ(NT, W, CONS, LP, FIT)))
refine_block_kernel(const KArgs k) {
  extern __shared__ double smem[];
  if (k.split != nullptr) {
    const int first = *k.split;
    if ((int)blockIdx.x < (first < k.split_cap ? first : k.split_cap)) return;
  }
  const int tid = threadIdx.x;
  const int cl = k.order[blockIdx.x];
#include "block_kernel_body.inc"
}

#endif  // CTREFINE_BLOCK_KERNEL_H
