// tu_fit_error.hip -- standard errors and covariance of a fitted table (ctr_fit_error_device,
// ctr_fit_error_plan; fit_error_kernels.h).  The covering test, r2 and the order of the
// terms are those of the residual stage: no floating-point contraction anywhere in this unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "stage_common.h"
#include "frame_max_kernels.h"
#include "fit_error_kernels.h"

template <int ND, bool ISO, int FIT>
hipError_t launch_class(const FitErrArgs& a, unsigned grid, size_t lds, hipStream_t s) {
  const hipError_t e = hipFuncSetAttribute((const void*)fit_error_kernel<ND, ISO, FIT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((fit_error_kernel<ND, ISO, FIT>), dim3(grid), dim3(FE_THREADS), lds, s, a);
  return hipSuccess;
}

template <int ND, bool ISO>
hipError_t launch_fit(int fit, const FitErrArgs& a, unsigned grid, size_t lds, hipStream_t s) {
  switch (fit) {
    case CTR_FIT_GAUSS: return launch_class<ND, ISO, CTR_FIT_GAUSS>(a, grid, lds, s);
    case CTR_FIT_RING: return launch_class<ND, ISO, CTR_FIT_RING>(a, grid, lds, s);
    case CTR_FIT_DISC: return launch_class<ND, ISO, CTR_FIT_DISC>(a, grid, lds, s);
    default: return launch_class<ND, ISO, CTR_FIT_INV_SERIES>(a, grid, lds, s);
  }
}

}  // namespace

int ctr_fit_error_launch(const ctr_fit_error* r, StageRun* stage, const char** msg, ctr_fit_error_launch_plan* plan) {
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
  const int np = 2 + ND + nsz + r->n_profile;
  if ((r->want_cov | 1) != 1) { *msg = "want_cov must be 0 or 1"; return CTR_ERR_INVALID; }
  if (r->max_grid < 0) { *msg = "max_grid must be >= 0"; return CTR_ERR_INVALID; }
  if (!(r->residual_factor > 0.) || !(r->residual_factor < INFINITY)) { *msg = "residual_factor must be positive"; return CTR_ERR_INVALID; }
  FitErrArgs a = {};
  for (int k = 0; k < np; ++k) {
    const int mode = r->modes[k];
    if (mode == CTR_MODE_GLOBAL) { *msg = "param_mode 'global' is not a mode of the fit of a cluster"; return CTR_ERR_UNSUPPORTED; }
    if (mode != CTR_MODE_CONST && mode != CTR_MODE_VAR && mode != CTR_MODE_CLUSTER) { *msg = "modes must be CTR_MODE_CONST, _VAR or _CLUSTER"; return CTR_ERR_INVALID; }
    if (k == 0 && mode == CTR_MODE_VAR) { *msg = "the background is constant or one per cluster"; return CTR_ERR_INVALID; }
    a.modes[k] = mode;
    a.n_var_cols += mode == CTR_MODE_VAR;
    a.n_cl_cols += mode == CTR_MODE_CLUSTER;
  }
  if (r->n_frames < 0 || r->n_features < 0 || r->n_clusters < 0 || r->n_vars_total < 0 || r->n_cov_total < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (r->n_features >= 0x7fffffffLL) { *msg = "too many features for one call"; return CTR_ERR_INVALID; }
  if (r->n_frames > 0x7fffffffLL) { *msg = "too many frames for one call"; return CTR_ERR_INVALID; }
  if (r->n_clusters > r->n_features) { *msg = "more clusters than features"; return CTR_ERR_INVALID; }
  long long E = 1;
  for (int d = 0; d < 3; ++d) { a.shape[d] = 1; a.radius[d] = 0; }
  for (int d = 0; d < ND; ++d) {
    if (r->shape[d] < 1 || r->shape[d] > (1LL << 30)) { *msg = "frame shape must be in [1, 2^30]"; return CTR_ERR_INVALID; }
    if (r->radius[d] < 1) { *msg = "radius must be >= 1"; return CTR_ERR_INVALID; }
    if (r->radius[d] > 1024) { *msg = "radius above 1024"; return CTR_ERR_UNSUPPORTED; }
    E *= r->shape[d];
    if (E > 0x7fffffffLL) { *msg = "more than 2^31 - 1 pixels per frame"; return CTR_ERR_INVALID; }
    a.shape[d] = (int)r->shape[d];
    a.radius[d] = (int)r->radius[d];
  }
  const long long T = r->n_frames, N = r->n_features, C = r->n_clusters;
  if (T > 0 && E > (1LL << 40) / T) { *msg = "more than 2^40 pixels in one call"; return CTR_ERR_INVALID; }
  const unsigned cap = r->max_grid > 0 && (unsigned)r->max_grid < stage->max_grid ? (unsigned)r->max_grid : stage->max_grid;
  long long most = T + 1 > N ? T + 1 : N;
  most = C + 1 > most ? C + 1 : most;
  const unsigned g_check = stride_grid(most, FE_THREADS, cap);
  const unsigned g_fit = C < 1 ? 1u : C > (long long)cap ? cap : (unsigned)C;
  size_t at = 0;
  const size_t o_table = carve(at, sizeof(int32_t));
  const size_t o_enc = carve(at, sizeof(unsigned long long) * (size_t)T);
  const size_t o_max = carve(at, sizeof(double) * (size_t)T);
  if (N == 0) at = 0;     // nothing to launch
  if (plan) {
    for (int k = 0; k < CTR_FITERR_CLASSES; ++k) {
      plan->max_vars[k] = FE_CLASS_VARS[k];
      plan->chunk[k] = FE_CLASS_CHUNK[k];
      plan->lds_bytes[k] = (long long)(sizeof(double) * fe_lds_doubles(k));
    }
    plan->grid = N > 0 ? g_fit : 0;
    plan->scratch_bytes = (long long)at;
  }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (N > 0 && (T < 1 || !r->frames || !r->frame_offset || !r->params || !r->order || !r->cluster_offset)) { *msg = "features without frames, params, order or cluster_offset"; return CTR_ERR_INVALID; }
  if (N > 0 && (!r->params_std || !r->status || !r->n_vars || !r->n_pix)) { *msg = "null output"; return CTR_ERR_INVALID; }
  if (r->want_cov ? N > 0 && (!r->var_offset || !r->cov_offset || (r->n_cov_total > 0 && !r->cov) || (r->n_vars_total > 0 && (!r->var_row || !r->var_col)))
                  : (r->var_offset || r->cov_offset || r->cov || r->var_row || r->var_col)) {
    *msg = "cov, var_row, var_col and their offsets go with want_cov";
    return CTR_ERR_INVALID;
  }
  stage->scratch_bytes = at;
  if (stage->mode != STAGE_LAUNCH || N == 0) return CTR_OK;
  const hipStream_t s = stage->stream;
  char* scratch = (char*)stage->scratch;
  a.nx = r->n_profile;
  a.n_params = np;
  a.dtype = r->frame_dtype;
  a.want_cov = r->want_cov;
  a.T = T; a.N = N; a.C = C; a.E = E;
  a.n_vars_total = r->n_vars_total;
  a.n_cov_total = r->n_cov_total;
  a.residual_factor = r->residual_factor;
  a.frames = r->frames;
  a.frame_offset = (const long long*)r->frame_offset;
  a.params = r->params;
  a.mask_pos = r->mask_pos;
  a.order = (const long long*)r->order;
  a.cluster_offset = (const long long*)r->cluster_offset;
  a.var_offset = (const long long*)r->var_offset;
  a.cov_offset = (const long long*)r->cov_offset;
  a.fmax = (const double*)(scratch + o_max);
  a.params_std = r->params_std;
  a.status = r->status;
  a.n_vars = r->n_vars;
  a.n_pix = (long long*)r->n_pix;
  a.cov = r->cov;
  a.var_row = (long long*)r->var_row;
  a.var_col = r->var_col;
  a.table = (int*)(scratch + o_table);
  STAGE_TRY(hipMemsetAsync(a.table, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(fiterr_check_kernel, dim3(g_check), dim3(FE_THREADS), 0, s, a);
  hipLaunchKernelGGL(fiterr_refuse_kernel, dim3(g_check), dim3(FE_THREADS), 0, s, a);
  bool too_large = false;
  STAGE_TRY(queue_frame_max(r->frames, r->frame_dtype, T, E, (unsigned long long*)(scratch + o_enc), (double*)(scratch + o_max), s, &too_large));
  if (too_large) { *msg = "frame block too large for one launch"; return CTR_ERR_INVALID; }
  for (int k = 0; k < CTR_FITERR_CLASSES; ++k) {
    a.cls = k;
    a.cls_lo = k > 0 ? FE_CLASS_VARS[k - 1] : 0;
    a.cls_hi = FE_CLASS_VARS[k];
    a.chunk = FE_CLASS_CHUNK[k];
    const size_t lds = sizeof(double) * fe_lds_doubles(k);
    if (ND == 2) STAGE_TRY(r->isotropic ? (launch_fit<2, true>(r->fit_function, a, g_fit, lds, s)) : (launch_fit<2, false>(r->fit_function, a, g_fit, lds, s)));
    else STAGE_TRY(r->isotropic ? (launch_fit<3, true>(r->fit_function, a, g_fit, lds, s)) : (launch_fit<3, false>(r->fit_function, a, g_fit, lds, s)));
  }
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
