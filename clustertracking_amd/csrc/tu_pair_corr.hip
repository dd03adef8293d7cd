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
#include "pair_corr_kernels.h"

// a static message, or null
const char* pcf_scalars(const ctr_pair_correlation* c) {
  if (c->ndim != 2 && c->ndim != 3) return "ndim must be 2 or 3";
  if (c->edge != CTR_PCF_EDGE_NONE && c->edge != CTR_PCF_EDGE_INTERIOR && c->edge != CTR_PCF_EDGE_ARC)
    return "edge must be CTR_PCF_EDGE_NONE, _INTERIOR or _ARC";
  if (c->edge == CTR_PCF_EDGE_ARC && c->ndim != 2) return "the arc correction is for ndim 2";
  if (c->pairs != CTR_PCF_PAIRS_ALL && c->pairs != CTR_PCF_PAIRS_SAME && c->pairs != CTR_PCF_PAIRS_OTHER)
    return "pairs must be CTR_PCF_PAIRS_ALL, _SAME or _OTHER";
  if (c->n_bins < 1) return "n_bins must be >= 1";
  if (c->n_bins > CTR_PCF_MAX_BINS) return "more than CTR_PCF_MAX_BINS bins";
  if (c->n_frames < 0 || c->n_features < 0) return "negative counts";
  if (c->n_frames > 0x7ffffffdLL || c->n_features > 0x7fffffffLL) return "too many frames or features for one call";
  if (!std::isfinite(c->dr) || !(c->dr > 0.)) return "dr must be finite and positive";
  for (int d = 0; d < c->ndim; ++d)
    if (!std::isfinite(c->mpp[d]) || !(c->mpp[d] > 0.)) return "mpp must be finite and positive";
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
  if (c->n_features > 0 && !c->pos) { *msg = "features without pos"; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && c->pairs != CTR_PCF_PAIRS_ALL && !c->group) { *msg = "pairs by group without group"; return CTR_ERR_INVALID; }
  if (!c->g) { *msg = "null output"; return CTR_ERR_INVALID; }
  if (c->n_frames > 0 && (!c->g_frame || !c->count || !c->weight || !c->n_ref || !c->n_rows)) { *msg = "null output"; return CTR_ERR_INVALID; }
  // a frame of n rows has ceil(n / 256) work items: at most T + N / 256 in all, whatever the offsets
  const long long max_items = c->n_frames + c->n_features / PCF_TILE;
  const bool arc = c->edge == CTR_PCF_EDGE_ARC;
  size_t total = 0;
  const size_t o_start = carve(total, sizeof(long long) * (size_t)(c->n_frames + 1));
  const size_t o_wpart = carve(total, arc ? sizeof(double) * (size_t)c->n_bins * (size_t)(max_items > 0 ? max_items : 1) : 0);
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  PcfArgs a = {};
  a.ndim = c->ndim; a.edge = c->edge; a.pairs = c->pairs;
  a.B = c->n_bins; a.T = c->n_frames; a.N = c->n_features;
  a.dr = c->dr;
  for (int d = 0; d < c->ndim; ++d) a.mpp[d] = c->mpp[d];
  a.pos = c->pos;
  a.frame_offset = (const long long*)c->frame_offset;
  a.group = (const long long*)c->group;
  a.box = c->box; a.edge2 = c->edge2; a.shell = c->shell;
  a.item_start = (long long*)((char*)stage->scratch + o_start);
  a.wpart = (double*)((char*)stage->scratch + o_wpart);
  a.g = c->g; a.g_frame = c->g_frame; a.count = (long long*)c->count; a.weight = c->weight;
  a.n_ref = (long long*)c->n_ref; a.n_rows = (long long*)c->n_rows;
  a.status = c->status;
  STAGE_TRY(hipMemsetAsync(a.status, 0, sizeof(int32_t), s));
  const dim3 block(PCF_THREADS);
  hipLaunchKernelGGL(pcf_check_kernel, dim3(stride_grid(a.T + 1, PCF_THREADS, stage->max_grid)), block, 0, s, a);
  if (a.T > 0) hipLaunchKernelGGL(pcf_frames_kernel, dim3(frame_grid(a.T, stage->max_grid)), block, 0, s, a);
  hipLaunchKernelGGL(pcf_items_kernel, dim3(1), block, 0, s, a);
  if (max_items > 0) hipLaunchKernelGGL(pcf_pairs_kernel, dim3(frame_grid(max_items, stage->max_grid)), block, 0, s, a);
  if (a.T > 0) hipLaunchKernelGGL(pcf_finish_kernel, dim3(stride_grid(a.T * a.B, PCF_THREADS, stage->max_grid)), block, 0, s, a);
  hipLaunchKernelGGL(pcf_pool_kernel, dim3(stride_grid(a.B, PCF_THREADS, stage->max_grid)), block, 0, s, a);
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
