// tu_refine_prepare.hip -- a refine batch from device tables and the scatter of its results
// (ctr_refine_prepare_device, ctr_refine_prepare_plan; refine_prepare_kernels.h): the
// descriptor's checks, the scratch layout and the queue of kernels.  The pair test and the bounds
// must equal NumPy's bit for bit: no floating-point contraction anywhere in this unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "stage_common.h"
#include "refine_prepare_kernels.h"

}  // namespace

int ctr_refine_prepare_launch(const ctr_refine_prepare* r, StageRun* stage, const char** msg, long long* scratch_bytes) {
  *msg = "";
  if (!r) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (r->mode != CTR_PREPARE_BATCH && r->mode != CTR_PREPARE_SCATTER) { *msg = "unknown mode"; return CTR_ERR_INVALID; }
  if (r->ndim != 2 && r->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (r->n_params < 1 || r->n_params > CTR_MAX_PARAMS) { *msg = "n_params must be 1 .. CTR_MAX_PARAMS"; return CTR_ERR_INVALID; }
  if (r->n_frames < 0 || r->n_features < 0 || r->n_clusters < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (r->n_frames > 0x7ffffffeLL || r->n_features > 0x7ffffffeLL) { *msg = "too many frames or features for one call"; return CTR_ERR_INVALID; }
  const bool batch = r->mode == CTR_PREPARE_BATCH;
  const long long T = r->n_frames, N = r->n_features;
  if (batch) {
    for (int a = 0; a < r->ndim; ++a)
      if (!(r->separation[a] > 0.) || std::isinf(r->separation[a])) { *msg = "separation must be positive and finite"; return CTR_ERR_INVALID; }
    for (int k = 0; k < r->n_params; ++k)
      if (r->modes[k] != CTR_MODE_CONST && r->modes[k] != CTR_MODE_VAR && r->modes[k] != CTR_MODE_CLUSTER) {
        *msg = "modes must be const, var or cluster"; return CTR_ERR_INVALID;
      }
  } else if (r->n_clusters > N) { *msg = "more clusters than features"; return CTR_ERR_INVALID; }
  size_t at = 0;
  const size_t o_spos = carve(at, 8 * (size_t)N * r->ndim), o_count = carve(at, 4 * (size_t)N), o_rank = carve(at, 4 * (size_t)N),
               o_local = carve(at, 4 * (size_t)N), o_cbase = carve(at, 4 * (size_t)(T + 1)), total = batch ? at : 0;
  if (scratch_bytes) *scratch_bytes = (long long)total;
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (batch) {
    if (!r->frame_offset || !r->feat_offset || !r->n_clusters_out || !r->status) {
      *msg = "null frame_offset, feat_offset, n_clusters_out or status"; return CTR_ERR_INVALID;
    }
    if (N > 0 && (!r->pos || !r->params0 || !r->label || !r->cluster_size || !r->order || !r->frame_index || !r->params ||
                  !r->low || !r->high)) {
      *msg = "features without a table"; return CTR_ERR_INVALID;
    }
  } else {
    if (N > 0 && (!r->order || !r->feat_offset || !r->fit_params || !r->params_out || !r->cost_out)) {
      *msg = "features without a table"; return CTR_ERR_INVALID;
    }
    if (N > 0 && r->n_clusters > 0 && !r->fit_cost) { *msg = "clusters without fit_cost"; return CTR_ERR_INVALID; }
    if (r->fit_std && !r->std_out) { *msg = "fit_std without std_out"; return CTR_ERR_INVALID; }
  }
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  const dim3 block(RP_THREADS);
  RpArgs a = {};
  a.ndim = r->ndim; a.np = r->n_params;
  a.T = T; a.N = N; a.C = r->n_clusters;
  a.order = r->order;
  a.feat_offset = r->feat_offset;
  if (!batch) {
    if (N == 0) return CTR_OK;
    a.fit_params = r->fit_params; a.fit_cost = r->fit_cost; a.fit_std = r->fit_std;
    a.params_out = r->params_out; a.cost_out = r->cost_out; a.std_out = r->std_out;
    hipLaunchKernelGGL(rp_scatter_kernel, dim3(stride_grid(N * a.np, RP_THREADS, stage->max_grid)), block, 0, s, a);
    STAGE_TRY(hipGetLastError());
    return CTR_OK;
  }
  char* ws = (char*)stage->scratch;
  for (int d = 0; d < 3; ++d) a.sep[d] = d < r->ndim ? r->separation[d] : 1.;
  RpBounds b;
  for (int k = 0; k < 2 * CTR_MAX_PARAMS; ++k) {
    b.abs[k] = r->bound_abs[k]; b.diff[k] = r->bound_diff[k]; b.rel[k] = r->bound_rel[k];
  }
  for (int k = 0; k < CTR_MAX_PARAMS; ++k) a.modes[k] = k < r->n_params ? r->modes[k] : CTR_MODE_CONST;
  a.pos = r->pos;
  a.frame_offset = (const long long*)r->frame_offset;
  a.params0 = r->params0;
  a.spos = (double*)(ws + o_spos);
  a.count = (int*)(ws + o_count);
  a.rank = (int*)(ws + o_rank);
  a.local = (int*)(ws + o_local);
  a.cbase = (int*)(ws + o_cbase);
  a.label = r->label; a.size = r->cluster_size; a.frame_index = r->frame_index;
  a.n_clusters = r->n_clusters_out;
  a.params = r->params; a.low = r->low; a.high = r->high;
  a.status = r->status;
  STAGE_TRY(hipMemsetAsync(r->status, 0, 2 * sizeof(int32_t), s));
  hipLaunchKernelGGL(rp_setup_kernel, dim3(stride_grid(T + 1 > N ? T + 1 : N, RP_THREADS, stage->max_grid)), block, 0, s, a);
  const dim3 gT(frame_grid(T, stage->max_grid));
  if (T > 0 && N > 0) {
    if (r->ndim == 2) hipLaunchKernelGGL(rp_label_kernel<2>, gT, block, 0, s, a);
    else hipLaunchKernelGGL(rp_label_kernel<3>, gT, block, 0, s, a);
  } else if (T > 0) {
    STAGE_TRY(hipMemsetAsync(a.cbase, 0, 4 * (size_t)T, s));   // frames without a row: no cluster
  }
  hipLaunchKernelGGL(rp_scan_kernel, dim3(1), block, 0, s, a);
  if (T > 0 && N > 0) {
    hipLaunchKernelGGL(rp_tables_kernel, gT, block, 0, s, a, b);
    hipLaunchKernelGGL(rp_feasible_kernel, dim3(stride_grid(N, RP_THREADS, stage->max_grid)), block, 0, s, a);
  }
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
