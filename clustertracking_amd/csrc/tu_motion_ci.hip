// tu_motion_ci.hip -- bootstrap confidence interval of the diffusion tensor (ctr_diffusion_ci_device,
// ctr_diffusion_ci_plan; motion_ci_kernels.h).  No floating-point contraction: a
// resample is the same bytes whether its rows come from LDS or from global memory.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "motion_kernels.h"
#include "motion_ci_kernels.h"

static_assert(CI_MAX_ALPHA == CTR_DIFFUSION_CI_MAX_ALPHA, "z_alpha / alphas of the descriptor");

// The launch decision.  It follows the host-known bound n_max on the rows of a pair, never the
// count n, which lives on the device:
//   rows in LDS: where n_max rows of D doubles fit into CTR_DIFFUSION_CI_LDS_BYTES (two workgroups
//     of CI_THREADS per CU: four wavefronts per SIMD); the workgroup then takes
//     exactly those bytes.  Otherwise the rows are gathered from the scratch in global memory.
//   scratch of a pair: its rows [n_max, D], its statistics [D (D + 1) / 2, B] and its count;
//   chunk: as many pairs as CTR_DIFFUSION_CI_SCRATCH_BYTES hold, at most all of them.
struct CiPlan {
  int D, NE;
  long long n_pairs, n_max, pair_bytes;
  ctr_ci_plan out;
};

template <int D>
void launch_resample(bool lds, const CiArgs& a, unsigned grid, size_t lds_bytes, hipStream_t s) {
  if (lds) hipLaunchKernelGGL((ci_resample_kernel<D, true>), dim3(grid), dim3(CI_THREADS), lds_bytes, s, a);
  else hipLaunchKernelGGL((ci_resample_kernel<D, false>), dim3(grid), dim3(CI_THREADS), 0, s, a);
}

}  // namespace

int ctr_diffusion_ci_launch(const ctr_diffusion_ci* d, StageRun* stage, const char** msg, ctr_ci_plan* plan) {
  *msg = "";
  if (!d) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (d->ndim != 2 && d->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (d->n_perm < 1 || d->n_perm > 4096) { *msg = "n_perm must be in [1, 4096]"; return CTR_ERR_INVALID; }
  if (d->n_tracks < 0 || d->n_frames < 0 || d->n_lags < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (!std::isfinite(d->fps) || !(d->fps > 0.)) { *msg = "fps must be positive"; return CTR_ERR_INVALID; }
  if (d->method != CTR_CI_BCA && d->method != CTR_CI_PI) { *msg = "method must be CTR_CI_BCA or CTR_CI_PI"; return CTR_ERR_INVALID; }
  if (d->n_alpha < 1 || d->n_alpha > CTR_DIFFUSION_CI_MAX_ALPHA) { *msg = "n_alpha must be in [1, CTR_DIFFUSION_CI_MAX_ALPHA]"; return CTR_ERR_INVALID; }
  for (int q = 0; q < d->n_alpha; ++q) {
    if (!(d->alphas[q] >= 0. && d->alphas[q] <= 1.)) { *msg = "alphas must be probabilities"; return CTR_ERR_INVALID; }
    if (d->method == CTR_CI_BCA && d->z_alpha[q] != d->z_alpha[q]) { *msg = "z_alpha is NaN"; return CTR_ERR_INVALID; }
  }
  if (d->n_samples < 1) { *msg = "n_samples must be >= 1"; return CTR_ERR_INVALID; }
  if (d->n_samples > CTR_DIFFUSION_CI_MAX_SAMPLES) { *msg = "n_samples above CTR_DIFFUSION_CI_MAX_SAMPLES"; return CTR_ERR_UNSUPPORTED; }
  const long long lim = (1LL << 31) - 1;
  if (d->n_tracks > lim || d->n_frames > lim || d->n_lags > lim) { *msg = "too many tracks, frames or lags for one call"; return CTR_ERR_INVALID; }
  const bool pool = d->pool_tracks != 0;
  CiPlan p;
  p.D = d->ndim == 2 ? 3 : 6;
  p.NE = p.D * (p.D + 1) / 2;
  p.n_max = (long long)d->n_perm * d->n_frames;                  // < 2^12 2^31
  if (pool && d->n_tracks > 0 && p.n_max > lim / d->n_tracks) { *msg = "more than 2^31 - 1 pooled rows"; return CTR_ERR_INVALID; }
  if (pool) p.n_max *= d->n_tracks;
  if (p.n_max > lim) { *msg = "more than 2^31 - 1 rows"; return CTR_ERR_INVALID; }
  if (!pool && d->n_lags > 0 && d->n_tracks > lim / d->n_lags) { *msg = "too many tracks, frames or lags for one call"; return CTR_ERR_INVALID; }
  p.n_pairs = pool ? d->n_lags : d->n_tracks * d->n_lags;
  p.pair_bytes = 8 * (p.n_max * p.D + p.NE * d->n_samples + 1);
  const long long row_bytes = p.n_max * p.D * 8;
  p.out.rows_in_lds = row_bytes <= CTR_DIFFUSION_CI_LDS_BYTES ? 1 : 0;
  p.out.lds_bytes = p.out.rows_in_lds ? row_bytes : 0;
  const long long fit = (long long)CTR_DIFFUSION_CI_SCRATCH_BYTES / p.pair_bytes;
  p.out.pairs_per_chunk = p.n_pairs < fit ? p.n_pairs : fit;
  p.out.scratch_bytes = p.out.pairs_per_chunk * p.pair_bytes;
  if (p.n_pairs > 0 && fit == 0) {
    *msg = "the rows and statistics of one (track, lag) exceed CTR_DIFFUSION_CI_SCRATCH_BYTES";
    return CTR_ERR_UNSUPPORTED;
  }
  if (plan) *plan = p.out;
  stage->scratch_bytes = p.out.pairs_per_chunk ? (size_t)p.out.scratch_bytes + 256 : 0;   // (0: nothing to resample)
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (p.n_pairs > 0 && (!d->lags || !d->interval)) { *msg = "null lags or interval"; return CTR_ERR_INVALID; }
  if (p.n_pairs > 0 && p.n_max > 0 && d->n_tracks > 0 && (!d->positions || !d->bases)) { *msg = "null input"; return CTR_ERR_INVALID; }
  if (stage->mode != STAGE_LAUNCH || p.n_pairs == 0) return CTR_OK;
  const hipStream_t s = stage->stream;

  CiArgs a;
  a.ndim = d->ndim;
  a.n_perm = d->n_perm;
  a.n_alpha = d->n_alpha;
  a.method = d->method;
  a.pool = pool ? 1 : 0;
  a.T = d->n_tracks;
  a.F = d->n_frames;
  a.n_lags = d->n_lags;
  a.n_max = p.n_max;
  a.B = d->n_samples;
  a.B2 = 1;
  while (a.B2 < a.B) a.B2 <<= 1;
  {                                                     // mix64(seed), as the device's
    unsigned long long z = d->seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    a.seed_mix = z ^ (z >> 31);
  }
  a.fps = d->fps;
  for (int q = 0; q < CI_MAX_ALPHA; ++q) {
    a.z_alpha[q] = q < d->n_alpha ? d->z_alpha[q] : 0.;
    a.alphas[q] = q < d->n_alpha ? d->alphas[q] : 0.;
  }
  a.lags = (const long long*)d->lags;
  a.positions = d->positions;
  a.bases = d->bases;
  const long long c = p.out.pairs_per_chunk;
  a.rows = (double*)stage->scratch;
  a.stats = a.rows + c * p.n_max * p.D;
  a.n = (long long*)(a.stats + c * p.NE * a.B);
  a.interval = d->interval;
  a.tensor = d->tensor;
  a.n_rows = (long long*)d->n_rows;
  a.z0 = d->z0;
  a.accel = d->accel;
  a.ranks = (long long*)d->ranks;
  const size_t sort_bytes = sizeof(double) * (size_t)a.B2;
  if (sort_bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)ci_order_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_bytes);
    if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  }
  const long long per_pair = (a.B + CI_THREADS - 1) / CI_THREADS;
  for (long long first = 0; first < p.n_pairs; first += c) {
    const long long m = p.n_pairs - first < c ? p.n_pairs - first : c;      // pairs of this chunk
    a.pair0 = first;
    hipLaunchKernelGGL(ci_rows_kernel, dim3((unsigned)m), dim3(MOT_THREADS), 0, s, a);
    const unsigned grid = (unsigned)(m * per_pair);
    if (p.D == 3) launch_resample<3>(p.out.rows_in_lds != 0, a, grid, (size_t)p.out.lds_bytes, s);
    else launch_resample<6>(p.out.rows_in_lds != 0, a, grid, (size_t)p.out.lds_bytes, s);
    hipLaunchKernelGGL(ci_order_kernel, dim3((unsigned)(m * p.NE)), dim3(CI_THREADS), sort_bytes, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  }
  return CTR_OK;
}
