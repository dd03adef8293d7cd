// tu_train.hip -- training of shared fit parameters (ctr_train_device; train_kernels.h,
// DESIGN.md 7b): the descriptor's checks, the scratch layout and the queue of iterations.
#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "stage_common.h"
#include "frame_max_kernels.h"
#include "train_kernels.h"

template <int ND, bool ISO>
const void* accumulate_fit(int fit) {
  switch (fit) {
    case CTR_FIT_GAUSS: return (const void*)train_accumulate_kernel<ND, ISO, CTR_FIT_GAUSS>;
    case CTR_FIT_RING: return (const void*)train_accumulate_kernel<ND, ISO, CTR_FIT_RING>;
    case CTR_FIT_DISC: return (const void*)train_accumulate_kernel<ND, ISO, CTR_FIT_DISC>;
    default: return (const void*)train_accumulate_kernel<ND, ISO, CTR_FIT_INV_SERIES>;
  }
}

const void* accumulate_kernel(int ndim, int iso, int fit) {
  if (ndim == 2) return iso ? accumulate_fit<2, true>(fit) : accumulate_fit<2, false>(fit);
  return iso ? accumulate_fit<3, true>(fit) : accumulate_fit<3, false>(fit);
}

}  // namespace

int ctr_train_launch(const ctr_train* t, StageRun* stage, const char** msg) {
  *msg = "";
  if (!t) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (t->ndim != 2 && t->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (t->fit_function < CTR_FIT_GAUSS || t->fit_function > CTR_FIT_INV_SERIES) { *msg = "unknown fit function"; return CTR_ERR_INVALID; }
  if (t->frame_dtype < CTR_DTYPE_U8 || t->frame_dtype > CTR_DTYPE_F64) { *msg = "unknown frame dtype"; return CTR_ERR_UNSUPPORTED; }
  const int nsz = t->isotropic ? 1 : t->ndim, base = 2 + t->ndim + nsz;
  int nx = t->fit_function == CTR_FIT_GAUSS ? 0 : 1;
  if (t->fit_function == CTR_FIT_INV_SERIES) {
    if (t->n_params < base + 1) { *msg = "inv_series needs at least the column 'signal_mult'"; return CTR_ERR_INVALID; }
    if (t->n_params > CTR_MAX_PARAMS) { *msg = "inv_series: more than CTR_MAX_PARAMS parameter columns"; return CTR_ERR_UNSUPPORTED; }
    nx = t->n_params - base;
  }
  if (t->n_params != base + nx) { *msg = "n_params does not match ndim/isotropic"; return CTR_ERR_INVALID; }
  TrnArgs a = {};
  for (int q = 0; q < TRN_MAXQ; ++q) a.slot_of[q] = -1;
  for (int k = 0; k < t->n_params; ++k) {
    const int m = t->modes[k];
    if (m == CTR_MODE_VAR || m == CTR_MODE_CLUSTER) { *msg = "only constant and global parameters are trained (param modes 'var' and 'cluster' are not)"; return CTR_ERR_UNSUPPORTED; }
    if (m != CTR_MODE_CONST && m != CTR_MODE_GLOBAL) { *msg = "unknown param mode"; return CTR_ERR_INVALID; }
    if (m != CTR_MODE_GLOBAL) continue;
    if (k < 2 + t->ndim) { *msg = "background, signal and positions are constant in training: global there couples per-feature variables"; return CTR_ERR_UNSUPPORTED; }
    a.slot_of[k - (2 + t->ndim)] = a.G;   // nsz + nx <= CTR_MAX_PARAMS - 4 = TRN_MAXQ
    a.cand_of[a.G++] = k - (2 + t->ndim);
  }
  if (a.G == 0) { *msg = "no global parameter: nothing to train"; return CTR_ERR_INVALID; }
  for (int d = 0; d < t->ndim; ++d) {
    if (t->radius[d] < 1) { *msg = "radius must be >= 1"; return CTR_ERR_INVALID; }
    if (t->radius[d] > 1024) { *msg = "radius above 1024"; return CTR_ERR_UNSUPPORTED; }
  }
  if (t->solver_maxiter < 1 || t->solver_maxiter > 10000) { *msg = "solver_maxiter must be in [1, 10000]"; return CTR_ERR_INVALID; }
  if (t->check_every < 0) { *msg = "check_every must be >= 0"; return CTR_ERR_INVALID; }
  if (!(t->residual_factor > 0.)) { *msg = "residual_factor must be positive"; return CTR_ERR_INVALID; }
  if (t->max_rms_dev != t->max_rms_dev) { *msg = "max_rms_dev is NaN"; return CTR_ERR_INVALID; }
  if (t->n_frames < 0 || t->n_problems < 0 || t->n_clusters < 0 || t->n_features < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (t->max_features < 0) { *msg = "negative max_features"; return CTR_ERR_INVALID; }
  if (t->max_features > CTR_TRAIN_MAX_FEATURES) { *msg = "a cluster of more than 64 features (max_features) is beyond the training kernels"; return CTR_ERR_UNSUPPORTED; }
  long long E = 1;
  for (int d = 0; d < t->ndim; ++d) {
    if (t->shape[d] < 1 || t->shape[d] > (1LL << 30)) { *msg = "frame shape must be in [1, 2^30]"; return CTR_ERR_INVALID; }
    E *= t->shape[d];
    if (E > 0x7fffffffLL) { *msg = "more than 2^31 - 1 pixels per frame"; return CTR_ERR_INVALID; }
  }
  if (t->n_frames > 0x7fffffffLL || t->n_problems > 0x7fffffffLL || t->n_clusters > 0x7ffffffeLL ||
      t->n_features > 0x7fffffffLL) { *msg = "too many frames, problems, clusters or features for one call"; return CTR_ERR_INVALID; }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (t->n_problems > 0) {
    if (!t->problem_offset || !t->start || !t->low || !t->high) { *msg = "problems without problem_offset, start, low or high"; return CTR_ERR_INVALID; }
    if (!t->globals || !t->cost || !t->status || !t->n_iter) { *msg = "null output"; return CTR_ERR_INVALID; }
    if (t->n_clusters > 0 && (!t->feat_offset || !t->frame_index)) { *msg = "clusters without feat_offset or frame_index"; return CTR_ERR_INVALID; }
    if (t->n_features > 0 && (!t->params || t->n_frames < 1)) { *msg = "features without params or frames"; return CTR_ERR_INVALID; }
    if (t->n_frames > 0 && !t->frames) { *msg = "null frames"; return CTR_ERR_INVALID; }
  }
  // scratch: frame maxima (encoded, decoded), the partials table, the state blocks, cluster ->
  // problem, the finished words and their count
  const size_t nF = (size_t)t->n_frames, P = (size_t)t->n_problems, C = (size_t)t->n_clusters;
  size_t total = 0;
  const size_t o_enc = carve(total, 8 * nF), o_fmax = carve(total, 8 * nF), o_part = carve(total, 8 * C * TRN_K),
               o_state = carve(total, 8 * P * TS_SIZE), o_prob = carve(total, 4 * C), o_done = carve(total, 4 * (P + 1));
  stage->scratch_bytes = P > 0 ? total : 0;
  if (stage->mode != STAGE_LAUNCH || P == 0) return CTR_OK;

  const hipStream_t s = stage->stream;
  char* ws = (char*)stage->scratch;
  a.frames = t->frames;
  a.frame_dtype = t->frame_dtype;
  a.frame_elems = E;
  a.n_frames = t->n_frames;
  for (int d = 0; d < 3; ++d) { a.fshape[d] = d < t->ndim ? (long)t->shape[d] : 1; a.radius[d] = d < t->ndim ? t->radius[d] : 0; }
  a.n_params = t->n_params;
  a.nx = nx;
  a.nq = nsz + (t->fit_function == CTR_FIT_INV_SERIES ? TRN_MAXQ - nsz : nx);
  a.C = t->n_clusters; a.N = t->n_features;
  a.params = t->params; a.feat_offset = t->feat_offset; a.frame_index = t->frame_index;
  a.problem_offset = t->problem_offset;
  a.start = t->start; a.low = t->low; a.high = t->high;
  a.globals = t->globals; a.cost = t->cost; a.status = t->status; a.n_iter = t->n_iter;
  a.residual_factor = t->residual_factor; a.max_rms_dev = t->max_rms_dev; a.xtol = t->xtol; a.ftol = t->ftol;
  a.maxiter = t->solver_maxiter;
  a.fmax = (const double*)(ws + o_fmax);
  a.partials = (double*)(ws + o_part);
  a.state = (double*)(ws + o_state);
  a.prob_of = (int*)(ws + o_prob);
  a.done = (int*)(ws + o_done);
  a.n_done = a.done + P;

  // a cluster that no problem owns keeps -1 and is passed over
  if (C) STAGE_TRY(hipMemsetAsync(ws + o_prob, 0xff, 4 * C, s));
  STAGE_TRY(hipMemsetAsync(ws + o_done, 0, 4 * (P + 1), s));
  if (nF) {
    bool too_large = false;
    STAGE_TRY(queue_frame_max(t->frames, t->frame_dtype, t->n_frames, E, (unsigned long long*)(ws + o_enc),
                            (double*)(ws + o_fmax), s, &too_large));
    if (too_large) { *msg = "frame block too large for one launch"; return CTR_ERR_INVALID; }
  }
  hipLaunchKernelGGL(train_setup_kernel, dim3((unsigned)P), dim3(TRN_THREADS), 0, s, a);
  const void* acc = accumulate_kernel(t->ndim, t->isotropic, t->fit_function);
  // iteration i judges the evaluation queued in front of it: the start's (i = 0), then one trial
  // each; iterations that need no pixel pass are spent inside the step kernel, so solver_maxiter
  // trials are the most a problem can ask for
  for (int i = 0; i <= t->solver_maxiter; ++i) {
    if (C) {
      void* args[] = {&a};
      STAGE_TRY(hipLaunchKernel(acc, dim3((unsigned)C), dim3(TRN_THREADS), args, 0, s));
    }
    hipLaunchKernelGGL(train_step_kernel, dim3((unsigned)P), dim3(TRN_STEP_THREADS), 0, s, a);
    if (t->check_every > 0 && (i + 1) % t->check_every == 0 && i < t->solver_maxiter) {
      int n_done = 0;
      STAGE_TRY(hipMemcpyAsync(&n_done, a.n_done, sizeof(int), hipMemcpyDeviceToHost, s));
      STAGE_TRY(hipStreamSynchronize(s));
      if (n_done >= (long long)P) break;
    }
  }
  STAGE_TRY(hipGetLastError());
  if (t->check_every > 0) STAGE_TRY(hipStreamSynchronize(s));
  return CTR_OK;
}
