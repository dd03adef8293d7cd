// tu_link.hip -- frame-to-frame linking (ctr_link_device, ctr_link_adaptive_device, ctr_link_predict_device;
// link_kernels.h, link_predict_kernels.h).
// Distances are compared with the host linker's: no floating-point contraction in this unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "stage_common.h"
#include "link_kernels.h"
#include "link_predict_kernels.h"

// ad: the adaptive linker (link_solve_adaptive_kernel in the place of link_solve_kernel), or null
template <int ND>
void run(const LinkArgs& a, const LinkAdaptiveArgs* ad, hipStream_t s) {
  const unsigned rows = (unsigned)((a.n + LNK_THREADS - 1) / LNK_THREADS);
  hipLaunchKernelGGL(link_prep_kernel<ND>, dim3(rows), dim3(LNK_THREADS), 0, s, a);
  const int last = a.n_levels;
  if (last > 1) {
    if (a.memory == 0) {
      hipLaunchKernelGGL(link_cand_kernel<ND>, dim3(rows), dim3(LNK_THREADS), 0, s, a, 1, last);
      if (ad) hipLaunchKernelGGL(link_solve_adaptive_kernel, dim3((unsigned)(last - 1)), dim3(LNK_THREADS), 0, s, a, *ad, 1);
      else hipLaunchKernelGGL(link_solve_kernel, dim3((unsigned)(last - 1)), dim3(LNK_THREADS), 0, s, a, 1);
    } else {
      // level t reads the `used` flags level t - 1 wrote: queued level by level.  The host does
      // not know the levels' sizes (frame_offset is on the device): a fixed grid strides over them
      const unsigned per_level = rows < 64u ? rows : 64u;
      for (int t = 1; t < last; ++t) {
        hipLaunchKernelGGL(link_cand_kernel<ND>, dim3(per_level), dim3(LNK_THREADS), 0, s, a, t, t + 1);
        if (ad) hipLaunchKernelGGL(link_solve_adaptive_kernel, dim3(1), dim3(LNK_THREADS), 0, s, a, *ad, t);
        else hipLaunchKernelGGL(link_solve_kernel, dim3(1), dim3(LNK_THREADS), 0, s, a, t);
      }
    }
  }
  hipLaunchKernelGGL(link_rank_kernel<ND>, dim3(rows), dim3(LNK_THREADS), 0, s, a);
  hipLaunchKernelGGL(link_scan_kernel, dim3(1), dim3(LNK_THREADS), 0, s, a);
  for (long long reach = 1; reach < a.n_levels - 1; reach *= 2)
    hipLaunchKernelGGL(link_jump_kernel, dim3(rows), dim3(LNK_THREADS), 0, s, a);
  hipLaunchKernelGGL(link_ids_kernel, dim3(rows), dim3(LNK_THREADS), 0, s, a);
}

// ctr_link_predict_device: level by level whatever the memory.  After the solve of level t the
// velocities of its rows and the predicted positions of level t + 1's sources, then the candidates
// of level t + 1 from those
template <int ND>
void run_predict(const LinkArgs& a, const LinkAdaptiveArgs* ad, const LinkPredictArgs& pr, hipStream_t s) {
  const unsigned rows = (unsigned)((a.n + LNK_THREADS - 1) / LNK_THREADS);
  const unsigned per_level = rows < 64u ? rows : 64u;   // the levels' sizes are on the device: a fixed grid strides
  hipLaunchKernelGGL(link_prep_kernel<ND>, dim3(rows), dim3(LNK_THREADS), 0, s, a);
  for (int t = 0; t < a.n_levels; ++t) {
    if (t > 0) {
      hipLaunchKernelGGL(link_cand_predict_kernel<ND>, dim3(per_level), dim3(LNK_THREADS), 0, s, a, pr, t, t + 1);
      if (ad) hipLaunchKernelGGL(link_solve_adaptive_kernel, dim3(1), dim3(LNK_THREADS), 0, s, a, *ad, t);
      else hipLaunchKernelGGL(link_solve_kernel, dim3(1), dim3(LNK_THREADS), 0, s, a, t);
    }
    if (pr.predictor == CTR_LINK_PREDICT_DRIFT) hipLaunchKernelGGL(link_drift_kernel<ND>, dim3(1), dim3(LNK_THREADS), 0, s, a, pr, t);
    else hipLaunchKernelGGL(link_velocity_kernel<ND>, dim3(per_level), dim3(LNK_THREADS), 0, s, a, pr, t);
  }
  hipLaunchKernelGGL(link_rank_kernel<ND>, dim3(rows), dim3(LNK_THREADS), 0, s, a);
  hipLaunchKernelGGL(link_scan_kernel, dim3(1), dim3(LNK_THREADS), 0, s, a);
  for (long long reach = 1; reach < a.n_levels - 1; reach *= 2)
    hipLaunchKernelGGL(link_jump_kernel, dim3(rows), dim3(LNK_THREADS), 0, s, a);
  hipLaunchKernelGGL(link_ids_kernel, dim3(rows), dim3(LNK_THREADS), 0, s, a);
}

// checks the descriptor and queues the call; adaptive: null for ctr_link_device; predict: null but
// for ctr_link_predict_device
int launch(const ctr_link* l, const ctr_link_adaptive* adaptive, const ctr_link_predict* predict, StageRun* stage,
           const char** msg) {
  if (l->ndim != 2 && l->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (l->n_levels < 0 || l->n_features < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (l->memory < 0) { *msg = "memory must be >= 0"; return CTR_ERR_INVALID; }
  for (int d = 0; d < l->ndim; ++d)
    if (!(l->search_range[d] > 0.) || std::isinf(l->search_range[d])) { *msg = "search_range must be a positive number"; return CTR_ERR_INVALID; }
  if (l->n_features > 0x7ffffff0LL || l->n_levels > 0x7ffffff0LL) { *msg = "too many features or levels for one call"; return CTR_ERR_INVALID; }
  if (l->n_features > 0 && (l->n_levels < 1 || !l->pos || !l->frame_offset)) { *msg = "features without levels, pos or frame_offset"; return CTR_ERR_INVALID; }
  if (l->n_features > 0 && (!l->particle || !l->n_tracks || !l->status)) { *msg = "null output"; return CTR_ERR_INVALID; }
  LinkAdaptiveArgs ad = {};
  if (adaptive) {
    if (!(adaptive->stop_rel > 0. && adaptive->stop_rel < 1.)) { *msg = "stop_rel must be inside (0, 1)"; return CTR_ERR_INVALID; }
    if (!(adaptive->step > 0. && adaptive->step < 1.)) { *msg = "step must be inside (0, 1)"; return CTR_ERR_INVALID; }
    if (adaptive->max_rounds < 1 || adaptive->max_rounds > CTR_LINK_MAX_ROUNDS) { *msg = "max_rounds must be 1 .. 64"; return CTR_ERR_INVALID; }
    ad.stop_rel = adaptive->stop_rel;
    ad.step = adaptive->step;
    ad.max_rounds = adaptive->max_rounds;
    ad.around = adaptive->adaptive_round;
  }
  LinkAdaptiveArgs* adp = adaptive ? &ad : nullptr;
  LinkPredictArgs pr = {};
  if (predict) {
    if (predict->predictor != CTR_LINK_PREDICT_VELOCITY && predict->predictor != CTR_LINK_PREDICT_DRIFT) { *msg = "predictor must be CTR_LINK_PREDICT_VELOCITY or CTR_LINK_PREDICT_DRIFT"; return CTR_ERR_INVALID; }
    for (int d = 0; d < l->ndim; ++d)
      if (!std::isfinite(predict->initial_velocity[d])) { *msg = "initial_velocity must be finite"; return CTR_ERR_INVALID; }
    pr.predictor = predict->predictor;
    for (int d = 0; d < 3; ++d) pr.v0[d] = d < l->ndim ? predict->initial_velocity[d] : 0.;
  }
  LinkPredictArgs* prp = predict ? &pr : nullptr;
  LinkArgs a = {};
  stage->scratch_bytes = lnk_layout(a, nullptr, l->n_features, l->ndim, l->n_levels, adp, prp);
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;
  const hipStream_t s = stage->stream;
  if (l->status && hipMemsetAsync(l->status, 0, 4 * sizeof(int32_t), s) != hipSuccess) { *msg = "hipMemsetAsync failed"; return CTR_ERR_DEVICE; }
  if (l->n_tracks && hipMemsetAsync(l->n_tracks, 0, sizeof(int64_t), s) != hipSuccess) { *msg = "hipMemsetAsync failed"; return CTR_ERR_DEVICE; }
  if (l->n_features == 0) return CTR_OK;
  if (ad.around && hipMemsetAsync(ad.around, 0, (size_t)l->n_features * sizeof(int32_t), s) != hipSuccess) { *msg = "hipMemsetAsync failed"; return CTR_ERR_DEVICE; }
  const size_t zeroed = lnk_layout(a, (char*)stage->scratch, l->n_features, l->ndim, l->n_levels, adp, prp);
  if (predict) pr.w = predict->velocity ? predict->velocity : pr.w_own;
  if (hipMemsetAsync(stage->scratch, 0, zeroed, s) != hipSuccess) { *msg = "hipMemsetAsync failed"; return CTR_ERR_DEVICE; }
  a.ndim = l->ndim;
  a.memory = l->memory < l->n_levels ? (int)l->memory : (int)l->n_levels;   // a longer memory reaches no further
  a.n_levels = (int)l->n_levels;
  a.n = l->n_features;
  a.pos = l->pos;
  a.off = (const long long*)l->frame_offset;
  for (int d = 0; d < 3; ++d) a.sr[d] = d < l->ndim ? l->search_range[d] : 1.;
  a.particle = (long long*)l->particle;
  a.n_tracks = (long long*)l->n_tracks;
  a.status = l->status;
  if (predict && l->ndim == 2) run_predict<2>(a, adp, pr, s);
  else if (predict) run_predict<3>(a, adp, pr, s);
  else if (l->ndim == 2) run<2>(a, adp, s);
  else run<3>(a, adp, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}

}  // namespace

int ctr_link_launch(const ctr_link* l, StageRun* stage, const char** msg) {
  *msg = "";
  if (!l) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  return launch(l, nullptr, nullptr, stage, msg);
}

int ctr_link_adaptive_launch(const ctr_link_adaptive* l, StageRun* stage, const char** msg) {
  *msg = "";
  if (!l) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  ctr_link plain = {};   // the fields of ctr_link, which the descriptor begins with
  plain.ndim = l->ndim;
  plain.memory = l->memory;
  plain.n_levels = l->n_levels;
  plain.n_features = l->n_features;
  for (int d = 0; d < CTR_MAX_NDIM; ++d) plain.search_range[d] = l->search_range[d];
  plain.pos = l->pos;
  plain.frame_offset = l->frame_offset;
  plain.particle = l->particle;
  plain.n_tracks = l->n_tracks;
  plain.status = l->status;
  return launch(&plain, l, nullptr, stage, msg);
}

int ctr_link_predict_launch(const ctr_link_predict* l, StageRun* stage, const char** msg) {
  *msg = "";
  if (!l) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  ctr_link_adaptive ad = {};   // the fields of ctr_link_adaptive, which the descriptor begins with
  ad.ndim = l->ndim;
  ad.memory = l->memory;
  ad.n_levels = l->n_levels;
  ad.n_features = l->n_features;
  for (int d = 0; d < CTR_MAX_NDIM; ++d) ad.search_range[d] = l->search_range[d];
  ad.pos = l->pos;
  ad.frame_offset = l->frame_offset;
  ad.particle = l->particle;
  ad.n_tracks = l->n_tracks;
  ad.status = l->status;
  ad.stop_rel = l->stop_rel;
  ad.step = l->step;
  ad.max_rounds = l->max_rounds;
  ad.adaptive_round = l->adaptive_round;
  ctr_link plain = {};
  plain.ndim = l->ndim;
  plain.memory = l->memory;
  plain.n_levels = l->n_levels;
  plain.n_features = l->n_features;
  for (int d = 0; d < CTR_MAX_NDIM; ++d) plain.search_range[d] = l->search_range[d];
  plain.pos = l->pos;
  plain.frame_offset = l->frame_offset;
  plain.particle = l->particle;
  plain.n_tracks = l->n_tracks;
  plain.status = l->status;
  return launch(&plain, l->max_rounds != 0 ? &ad : nullptr, l, stage, msg);   // max_rounds == 0: no adaptive range
}
