// tu_drift.hip -- drift of a linked video (ctr_drift_device, ctr_drift_subtract_device,
// ctr_filter_stubs_device; drift_kernels.h): the descriptors' checks, the scratch
// and the queue of kernels.
#include <cstdint>

#include "kargs.h"

namespace {

#include "stage_common.h"
#include "particle_match.h"
#include "drift_kernels.h"

}  // namespace

int ctr_drift_launch(const ctr_drift* c, StageRun* stage, const char** msg) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (c->ndim != 2 && c->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (c->smoothing < 0) { *msg = "smoothing must be >= 0"; return CTR_ERR_INVALID; }
  if (c->n_frames < 0 || c->n_features < 0 || c->n_particles < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (c->n_frames > 0x7ffffffeLL || c->n_features > 0x7fffffffLL || c->n_particles > 0x7ffffffeLL) {
    *msg = "too many frames, features or particles for one call"; return CTR_ERR_INVALID;
  }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!c->status || !c->frame_offset) { *msg = "null status or frame_offset"; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && (!c->particle || !c->pos)) { *msg = "features without particle or pos"; return CTR_ERR_INVALID; }
  if (c->n_frames > 0 && (!c->drift || !c->n_pairs)) { *msg = "null output"; return CTR_ERR_INVALID; }
  size_t total = 0;
  const size_t o_dx = carve(total, sizeof(double) * (size_t)c->ndim * (size_t)(c->n_frames > 0 ? c->n_frames : 1));
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  DriftArgs a = {};
  a.ndim = c->ndim; a.smoothing = c->smoothing;
  a.T = c->n_frames; a.N = c->n_features; a.P = c->n_particles;
  a.frame_offset = (const long long*)c->frame_offset;
  a.particle = (const long long*)c->particle;
  a.pos = c->pos;
  a.dx = (double*)((char*)stage->scratch + o_dx);
  a.drift = c->drift;
  a.n_pairs = c->n_pairs;
  a.status = c->status;
  const dim3 block(DR_THREADS);
  STAGE_TRY(hipMemsetAsync(c->status, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(drift_check_kernel, dim3(stride_grid(a.T + 1 > a.N ? a.T + 1 : a.N, DR_THREADS, stage->max_grid)), block, 0, s, a);
  if (a.T > 0) {
    hipLaunchKernelGGL(drift_pairs_kernel, dim3(frame_grid(a.T, stage->max_grid)), block, 0, s, a);
    hipLaunchKernelGGL(drift_scan_kernel, dim3(1), block, 0, s, a);
  }
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}

int ctr_drift_subtract_launch(const ctr_drift_subtract* c, StageRun* stage, const char** msg) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (c->ndim != 2 && c->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (c->n_frames < 0 || c->n_features < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (c->n_frames > 0x7ffffffeLL || c->n_features > 0x7fffffffLL) { *msg = "too many frames or features for one call"; return CTR_ERR_INVALID; }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!c->status || !c->frame_offset) { *msg = "null status or frame_offset"; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && (!c->pos || !c->pos_out)) { *msg = "features without pos or pos_out"; return CTR_ERR_INVALID; }
  if (c->n_frames > 0 && !c->drift) { *msg = "frames without drift"; return CTR_ERR_INVALID; }
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  DriftArgs a = {};
  a.ndim = c->ndim;
  a.T = c->n_frames; a.N = c->n_features;
  a.frame_offset = (const long long*)c->frame_offset;
  a.pos = c->pos;
  a.drift = (double*)c->drift;
  a.pos_out = c->pos_out;
  a.status = c->status;
  const dim3 block(DR_THREADS);
  STAGE_TRY(hipMemsetAsync(c->status, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(drift_check_kernel, dim3(stride_grid(a.T + 1, DR_THREADS, stage->max_grid)), block, 0, s, a);
  if (a.N > 0) hipLaunchKernelGGL(drift_subtract_kernel, dim3(stride_grid(a.N, DR_THREADS, stage->max_grid)), block, 0, s, a);
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}

int ctr_filter_stubs_launch(const ctr_filter_stubs* c, StageRun* stage, const char** msg) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (c->threshold < 1) { *msg = "threshold must be >= 1"; return CTR_ERR_INVALID; }
  if (c->n_features < 0 || c->n_particles < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (c->n_features > 0x7fffffffLL || c->n_particles > 0x7ffffffeLL) { *msg = "too many features or particles for one call"; return CTR_ERR_INVALID; }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!c->status) { *msg = "null status"; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && (!c->particle || !c->particle_out)) { *msg = "features without particle or particle_out"; return CTR_ERR_INVALID; }
  if (c->n_particles > 0 && !c->count) { *msg = "particles without count"; return CTR_ERR_INVALID; }
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  DriftArgs a = {};
  a.threshold = c->threshold;
  a.N = c->n_features; a.P = c->n_particles;
  a.particle = (const long long*)c->particle;
  a.particle_out = (long long*)c->particle_out;
  a.count = c->count;
  a.status = c->status;
  const dim3 block(DR_THREADS), grid(stride_grid(a.N, DR_THREADS, stage->max_grid));
  STAGE_TRY(hipMemsetAsync(c->status, 0, sizeof(int32_t), s));
  if (a.P > 0) STAGE_TRY(hipMemsetAsync(c->count, 0, sizeof(int32_t) * (size_t)a.P, s));
  if (a.N > 0) {
    hipLaunchKernelGGL(drift_check_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(drift_count_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(drift_stubs_kernel, grid, block, 0, s, a);
  }
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
