// tu_residual.hip -- model and residual frames of a fitted table (ctr_residual_device,
// ctr_residual_plan; residual_kernels.h).  The covering test, r2 and the order of the
// terms must equal the NumPy restatement operation for operation: no floating-point contraction
// anywhere in this unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "stage_common.h"
#include "frame_max_kernels.h"
#include "residual_kernels.h"

template <int FIT, int ND>
void launch_frame_iso(bool iso, const ResidArgs& a, unsigned grid, hipStream_t s) {
  if (iso) hipLaunchKernelGGL((resid_frame_kernel<FIT, ND, true>), dim3(grid), dim3(RESID_THREADS), 0, s, a);
  else hipLaunchKernelGGL((resid_frame_kernel<FIT, ND, false>), dim3(grid), dim3(RESID_THREADS), 0, s, a);
}

template <int ND>
void launch_frame(int fit, bool iso, const ResidArgs& a, unsigned grid, hipStream_t s) {
  switch (fit) {
    case CTR_FIT_GAUSS: launch_frame_iso<CTR_FIT_GAUSS, ND>(iso, a, grid, s); break;
    case CTR_FIT_RING: launch_frame_iso<CTR_FIT_RING, ND>(iso, a, grid, s); break;
    case CTR_FIT_DISC: launch_frame_iso<CTR_FIT_DISC, ND>(iso, a, grid, s); break;
    default: launch_frame_iso<CTR_FIT_INV_SERIES, ND>(iso, a, grid, s); break;
  }
}

// at least one workgroup, at most cap
unsigned capped(long long n, unsigned cap) { return n < 1 ? 1u : n > (long long)cap ? cap : (unsigned)n; }

}  // namespace

int ctr_residual_launch(const ctr_residual* r, StageRun* stage, const char** msg, ctr_residual_launch_plan* plan) {
  *msg = "";
  if (!r) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (r->ndim != 2 && r->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (r->frame_dtype < CTR_DTYPE_U8 || r->frame_dtype > CTR_DTYPE_F64) { *msg = "unknown frame dtype"; return CTR_ERR_UNSUPPORTED; }
  if (r->fit_function < CTR_FIT_GAUSS || r->fit_function > CTR_FIT_INV_SERIES) { *msg = "unknown fit function"; return CTR_ERR_INVALID; }
  if (r->isotropic != 0 && r->isotropic != 1) { *msg = "isotropic must be 0 or 1"; return CTR_ERR_INVALID; }
  const int ND = r->ndim, nsz = r->isotropic ? 1 : ND;
  const int nx_want = r->fit_function == CTR_FIT_GAUSS ? 0 : r->fit_function == CTR_FIT_INV_SERIES ? -1 : 1;
  if (nx_want >= 0 ? r->n_profile != nx_want : (r->n_profile < 1 || r->n_profile > INV_NX || 2 + ND + nsz + r->n_profile > CTR_MAX_PARAMS)) {
    *msg = "n_profile does not fit the fit function (inv_series: at most CTR_MAX_PARAMS columns)";
    return CTR_ERR_INVALID;
  }
  if (r->outside < CTR_RESID_ZERO || r->outside > CTR_RESID_IMAGE) { *msg = "outside must be CTR_RESID_ZERO, _NAN or _IMAGE"; return CTR_ERR_INVALID; }
  if ((r->want_frames | 1) != 1 || (r->want_model | 1) != 1 || (r->has_cluster | 1) != 1) { *msg = "want_frames, want_model and has_cluster must be 0 or 1"; return CTR_ERR_INVALID; }
  if (r->max_grid < 0) { *msg = "max_grid must be >= 0"; return CTR_ERR_INVALID; }
  if (r->n_frames < 0 || r->n_features < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (r->n_features >= 0x7fffffffLL) { *msg = "too many features for one call"; return CTR_ERR_INVALID; }
  if (r->n_frames > 0x7fffffffLL) { *msg = "too many frames for one call"; return CTR_ERR_INVALID; }
  ResidArgs a = {};
  long long E = 1, tiles = 1;
  const int tile2[3] = {8, 32, 1}, tile3[3] = {2, 8, 16};
  for (int d = 0; d < 3; ++d) { a.shape[d] = 1; a.radius[d] = 0; a.tile[d] = 1; a.ntile[d] = 1; }
  for (int d = 0; d < ND; ++d) {
    if (r->shape[d] < 1 || r->shape[d] > (1LL << 30)) { *msg = "frame shape must be in [1, 2^30]"; return CTR_ERR_INVALID; }
    if (r->radius[d] < 1) { *msg = "radius must be >= 1"; return CTR_ERR_INVALID; }
    if (r->radius[d] > 1024) { *msg = "radius above 1024"; return CTR_ERR_UNSUPPORTED; }
    E *= r->shape[d];
    if (E > 0x7fffffffLL) { *msg = "more than 2^31 - 1 pixels per frame"; return CTR_ERR_INVALID; }
    a.shape[d] = (int)r->shape[d];
    a.radius[d] = (int)r->radius[d];
    a.tile[d] = ND == 2 ? tile2[d] : tile3[d];
    a.ntile[d] = (a.shape[d] + a.tile[d] - 1) / a.tile[d];
    tiles *= a.ntile[d];
  }
  const long long T = r->n_frames, N = r->n_features;
  if (T > 0 && E > (1LL << 40) / T) { *msg = "more than 2^40 pixels in one call"; return CTR_ERR_INVALID; }
  const unsigned cap = r->max_grid > 0 && (unsigned)r->max_grid < stage->max_grid ? (unsigned)r->max_grid : stage->max_grid;
  const long long n_items = T * tiles;
  const unsigned g_check = stride_grid(T + 1, RESID_THREADS, cap);
  const unsigned g_frame = capped(n_items, cap);
  const unsigned g_feature = capped((N + RESID_THREADS / WAVE - 1) / (RESID_THREADS / WAVE), cap);
  const unsigned g_cluster = capped(T, cap);
  size_t at = 0;
  const size_t o_res = r->want_frames ? 0 : carve(at, sizeof(double) * (size_t)(T * E));
  const size_t o_own = r->want_frames ? 0 : carve(at, sizeof(int32_t) * (size_t)(T * E));
  const size_t o_enc = r->has_cluster ? carve(at, sizeof(unsigned long long) * (size_t)T) : 0;
  const size_t o_max = r->has_cluster ? carve(at, sizeof(double) * (size_t)T) : 0;
  at += STAGE_ALIGN;    // never 0: a call without rows still writes its frames
  if (plan) {
    for (int d = 0; d < 3; ++d) plan->tile[d] = a.tile[d];
    plan->chunk = RESID_CHUNK;
    plan->n_tiles = n_items;
    plan->grids[0] = g_check;
    plan->grids[1] = n_items > 0 ? g_frame : 0;
    plan->grids[2] = N > 0 ? g_feature : 0;
    plan->grids[3] = r->has_cluster && N > 0 ? g_cluster : 0;
    plan->lds_bytes = (long long)(sizeof(double) * RESID_CHUNK * RESID_ROWD + sizeof(int) * RESID_CHUNK + sizeof(int) * (RESID_THREADS / 64));
    plan->scratch_bytes = (long long)at;
  }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!r->frame_offset || !r->status) { *msg = "null frame_offset or status"; return CTR_ERR_INVALID; }
  if (n_items > 0 && !r->frames) { *msg = "null frames"; return CTR_ERR_INVALID; }
  if (N > 0 && (T < 1 || !r->params)) { *msg = "features without frames or params"; return CTR_ERR_INVALID; }
  if (N > 0 && (!r->n_pix || !r->n_own || !r->n_nan || !r->sum || !r->sum_sq || !r->own_sum_sq || !r->max_abs || !r->rms)) { *msg = "null output"; return CTR_ERR_INVALID; }
  if (r->want_frames ? n_items > 0 && (!r->residual || !r->coverage || !r->owner) : (r->residual || r->coverage || r->owner)) { *msg = "residual, coverage and owner go with want_frames"; return CTR_ERR_INVALID; }
  if (r->want_model ? n_items > 0 && !r->model : r->model != nullptr) { *msg = "model goes with want_model"; return CTR_ERR_INVALID; }
  if (r->has_cluster ? N > 0 && (!r->cluster || !r->cluster_n_pix || !r->cluster_sum_sq || !r->cost) : (r->cluster || r->cluster_n_pix || r->cluster_sum_sq || r->cost)) { *msg = "cluster and its three outputs go with has_cluster"; return CTR_ERR_INVALID; }
  stage->scratch_bytes = at;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;
  const hipStream_t s = stage->stream;
  char* scratch = (char*)stage->scratch;
  a.nx = r->n_profile;
  a.n_params = 2 + ND + nsz + r->n_profile;
  a.outside = r->outside;
  a.dtype = r->frame_dtype;
  a.T = T; a.N = N; a.E = E;
  a.tiles_per_frame = tiles;
  a.n_items = n_items;
  a.frames = r->frames;
  a.frame_offset = (const long long*)r->frame_offset;
  a.params = r->params;
  a.mask_pos = r->mask_pos;
  a.cluster = (const long long*)r->cluster;
  a.fmax = (const double*)(scratch + o_max);
  a.residual = r->want_frames ? r->residual : (double*)(scratch + o_res);
  a.owner = r->want_frames ? r->owner : (int*)(scratch + o_own);
  a.coverage = r->coverage;
  a.model = r->model;
  a.n_pix = (long long*)r->n_pix; a.n_own = (long long*)r->n_own; a.n_nan = (long long*)r->n_nan;
  a.sum = r->sum; a.sum_sq = r->sum_sq; a.own_sum_sq = r->own_sum_sq; a.max_abs = r->max_abs; a.rms = r->rms;
  a.cluster_n_pix = (long long*)r->cluster_n_pix;
  a.cluster_sum_sq = r->cluster_sum_sq;
  a.cost = r->cost;
  a.status = r->status;
  STAGE_TRY(hipMemsetAsync(r->status, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(resid_check_kernel, dim3(g_check), dim3(RESID_THREADS), 0, s, a);
  if (n_items > 0) {
    if (ND == 2) launch_frame<2>(r->fit_function, r->isotropic != 0, a, g_frame, s);
    else launch_frame<3>(r->fit_function, r->isotropic != 0, a, g_frame, s);
  }
  if (N > 0) {
    if (ND == 2) hipLaunchKernelGGL(resid_feature_kernel<2>, dim3(g_feature), dim3(RESID_THREADS), 0, s, a);
    else hipLaunchKernelGGL(resid_feature_kernel<3>, dim3(g_feature), dim3(RESID_THREADS), 0, s, a);
    if (r->has_cluster) {
      bool too_large = false;
      STAGE_TRY(queue_frame_max(r->frames, r->frame_dtype, T, E, (unsigned long long*)(scratch + o_enc), (double*)(scratch + o_max), s, &too_large));
      if (too_large) { *msg = "frame block too large for one launch"; return CTR_ERR_INVALID; }
      hipLaunchKernelGGL(resid_cluster_kernel, dim3(g_cluster), dim3(RESID_THREADS), 0, s, a);
    }
  }
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
