// tu_pair_corr.hip -- pair correlation function g(r) of a feature table (ctr_pair_correlation_device;
// pair_corr_kernels.h): the descriptor's checks, the scratch and the queue of kernels.
// A distance is compared with the edges that the host squared: every product and sum rounds on its
// own, no floating-point contraction anywhere in this unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "stage_common.h"
#include "pair_walk.h"
#include "pair_corr_kernels.h"

// a static message, or null
const char* pcf_scalars(const ctr_pair_correlation* c) {
  if (const char* why = pair_scalars(c, "too many frames or features for one call")) return why;
  if (c->edge != CTR_PCF_EDGE_NONE && c->edge != CTR_PCF_EDGE_INTERIOR && c->edge != CTR_PCF_EDGE_ARC)
    return "edge must be CTR_PCF_EDGE_NONE, _INTERIOR or _ARC";
  if (c->edge == CTR_PCF_EDGE_ARC && c->ndim != 2) return "the arc correction is for ndim 2";
  if (c->n_bins < 1) return "n_bins must be >= 1";
  if (c->n_bins > CTR_PCF_MAX_BINS) return "more than CTR_PCF_MAX_BINS bins";
  if (!std::isfinite(c->dr) || !(c->dr > 0.)) return "dr must be finite and positive";
  return nullptr;
}

}  // namespace

int ctr_pair_correlation_launch(const ctr_pair_correlation* c, StageRun* stage, const char** msg) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (const char* why = pcf_scalars(c)) { *msg = why; return CTR_ERR_INVALID; }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!c->status || !c->frame_offset) { *msg = "null status or frame_offset"; return CTR_ERR_INVALID; }
  if (!c->box || !c->edge2 || !c->shell) { *msg = "null box, edge2 or shell"; return CTR_ERR_INVALID; }
  if (const char* why = pair_columns(c)) { *msg = why; return CTR_ERR_INVALID; }
  if (!c->g) { *msg = "null output"; return CTR_ERR_INVALID; }
  if (c->n_frames > 0 && (!c->g_frame || !c->count || !c->weight || !c->n_ref || !c->n_rows)) { *msg = "null output"; return CTR_ERR_INVALID; }
  const bool arc = c->edge == CTR_PCF_EDGE_ARC;
  size_t total = 0, o_start;
  const long long max_items = pair_max_items(c, total, o_start);
  const size_t o_wpart = carve(total, arc ? sizeof(double) * (size_t)c->n_bins * (size_t)(max_items > 0 ? max_items : 1) : 0);
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  PcfArgs a = {};
  a.tab = pair_table(c, stage->scratch, o_start);
  a.edge = c->edge; a.B = c->n_bins; a.dr = c->dr;
  a.box = c->box; a.edge2 = c->edge2; a.shell = c->shell;
  a.wpart = (double*)((char*)stage->scratch + o_wpart);
  a.g = c->g; a.g_frame = c->g_frame; a.count = (long long*)c->count; a.weight = c->weight;
  a.n_ref = (long long*)c->n_ref; a.n_rows = (long long*)c->n_rows;
  const long long T = c->n_frames;
  STAGE_TRY(hipMemsetAsync(c->status, 0, sizeof(int32_t), s));
  const dim3 block(PCF_THREADS);
  hipLaunchKernelGGL(pcf_check_kernel, dim3(stride_grid(T + 1, PCF_THREADS, stage->max_grid)), block, 0, s, a);
  if (T > 0) hipLaunchKernelGGL(pcf_frames_kernel, dim3(frame_grid(T, stage->max_grid)), block, 0, s, a);
  hipLaunchKernelGGL(pcf_items_kernel, dim3(1), block, 0, s, a);
  if (max_items > 0) hipLaunchKernelGGL(pcf_pairs_kernel, dim3(frame_grid(max_items, stage->max_grid)), block, 0, s, a);
  if (T > 0) hipLaunchKernelGGL(pcf_finish_kernel, dim3(stride_grid(T * a.B, PCF_THREADS, stage->max_grid)), block, 0, s, a);
  hipLaunchKernelGGL(pcf_pool_kernel, dim3(stride_grid(a.B, PCF_THREADS, stage->max_grid)), block, 0, s, a);
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
