// tu_global.hip -- shared and per-feature parameters fitted in one problem (ctr_refine_global_device;
// global_kernels.h): the descriptor's checks, the scratch layout and the queue of
// iterations.
#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "stage_common.h"
#include "block_kernel.h"
#include "frame_max_kernels.h"
#include "global_kernels.h"

template <int ND, bool ISO, int FIT>
const void* eval_nt(int nt) {
  switch (nt) {
    case 1: return (const void*)global_eval_kernel<ND, ISO, FIT, 1>;
    case 2: return (const void*)global_eval_kernel<ND, ISO, FIT, 2>;
    default: return (const void*)global_eval_kernel<ND, ISO, FIT, 3>;
  }
}

template <int ND, bool ISO>
const void* eval_fit(int fit, int nt) {
  switch (fit) {
    case CTR_FIT_GAUSS: return eval_nt<ND, ISO, CTR_FIT_GAUSS>(nt);
    case CTR_FIT_RING: return eval_nt<ND, ISO, CTR_FIT_RING>(nt);
    case CTR_FIT_DISC: return eval_nt<ND, ISO, CTR_FIT_DISC>(nt);
    default: return eval_nt<ND, ISO, CTR_FIT_INV_SERIES>(nt);
  }
}

const void* eval_kernel(int ndim, int iso, int fit, int nt) {
  if (ndim == 2) return iso ? eval_fit<2, true>(fit, nt) : eval_fit<2, false>(fit, nt);
  return iso ? eval_fit<3, true>(fit, nt) : eval_fit<3, false>(fit, nt);
}

}  // namespace

int ctr_refine_global_launch(const ctr_refine_global* t, StageRun* stage, const char** msg, ctr_global_launch_plan* plan) {
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
  GlbArgs a = {};
  for (int k = 0; k < CTR_MAX_PARAMS; ++k) { a.mode[k] = CTR_MODE_CONST; a.gslot[k] = -1; }
  for (int k = 0; k < t->n_params; ++k) {
    const int m = t->modes[k];
    if (m != CTR_MODE_CONST && m != CTR_MODE_VAR && m != CTR_MODE_CLUSTER && m != CTR_MODE_GLOBAL) { *msg = "unknown param mode"; return CTR_ERR_INVALID; }
    if (m == CTR_MODE_GLOBAL && k >= 2 && k < 2 + t->ndim) { *msg = "a global position is not supported: background, signal, the sizes and the profile's columns may be global"; return CTR_ERR_UNSUPPORTED; }
    if (m == CTR_MODE_VAR && k == 0) { *msg = "the background cannot vary per feature (param mode 'var'): 'cluster', 'global' or 'const'"; return CTR_ERR_INVALID; }
    a.mode[k] = m;
    if (m == CTR_MODE_VAR) ++a.nvar;
    if (m == CTR_MODE_CLUSTER) ++a.ncl;
    if (m == CTR_MODE_GLOBAL) {
      if (a.G == GLB_MAXG) { *msg = "more than 8 global columns"; return CTR_ERR_UNSUPPORTED; }
      a.gslot[k] = a.G++;
    }
  }
  if (a.G == 0) { *msg = "no global parameter: ctr_refine_batch fits per-feature and per-cluster parameters"; return CTR_ERR_INVALID; }
  for (int d = 0; d < t->ndim; ++d) {
    if (t->radius[d] < 1) { *msg = "radius must be >= 1"; return CTR_ERR_INVALID; }
    if (t->radius[d] > 1024) { *msg = "radius above 1024"; return CTR_ERR_UNSUPPORTED; }
  }
  if (t->solver_maxiter < 1 || t->solver_maxiter > 10000) { *msg = "solver_maxiter must be in [1, 10000]"; return CTR_ERR_INVALID; }
  if (t->max_iter < 1 || t->max_iter > 1000) { *msg = "max_iter must be in [1, 1000]"; return CTR_ERR_INVALID; }
  if (t->check_every < 1) { *msg = "check_every must be >= 1 (there is no blind queue)"; return CTR_ERR_INVALID; }
  if (!(t->residual_factor > 0.)) { *msg = "residual_factor must be positive"; return CTR_ERR_INVALID; }
  if (t->max_rms_dev != t->max_rms_dev) { *msg = "max_rms_dev is NaN"; return CTR_ERR_INVALID; }
  if (!(t->max_shift >= 0.)) { *msg = "max_shift must be >= 0"; return CTR_ERR_INVALID; }
  if (t->n_frames < 0 || t->n_problems < 0 || t->n_clusters < 0 || t->n_features < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (t->max_features < 0 || t->max_locals < 0) { *msg = "negative max_features or max_locals"; return CTR_ERR_INVALID; }
  if (t->max_features > CTR_TRAIN_MAX_FEATURES) { *msg = "a cluster of more than 64 features (max_features) is beyond the global-fit kernels"; return CTR_ERR_UNSUPPORTED; }
  if (t->max_locals + a.G + 1 > GLB_MAXNV) { *msg = "a cluster of more than 48 columns (max_locals + globals + 1) is beyond the global-fit kernels"; return CTR_ERR_UNSUPPORTED; }
  long long E = 1;
  for (int d = 0; d < t->ndim; ++d) {
    if (t->shape[d] < 1 || t->shape[d] > (1LL << 30)) { *msg = "frame shape must be in [1, 2^30]"; return CTR_ERR_INVALID; }
    E *= t->shape[d];
    if (E > 0x7fffffffLL) { *msg = "more than 2^31 - 1 pixels per frame"; return CTR_ERR_INVALID; }
  }
  if (t->n_frames > 0x7fffffffLL || t->n_problems > 0x7fffffffLL || t->n_clusters > 0x7ffffffeLL ||
      t->n_features > 0x7fffffffLL) { *msg = "too many frames, problems, clusters or features for one call"; return CTR_ERR_INVALID; }

  // the launch decision: tiles of the row, the row of a cluster, the scratch
  const int LM = t->max_locals, NVc = LM + a.G + 1, nt = (NVc + 15) / 16;
  const int TP = NVc * (NVc + 1) / 2;
  const long long row_stride = ((2LL * TP + 5LL * LM + (long long)(a.G + 1) * LM + 1) / 2) * 2;
  const size_t nF = (size_t)t->n_frames, P = (size_t)t->n_problems, C = (size_t)t->n_clusters, N = (size_t)t->n_features;
  size_t total = 0;
  const size_t o_enc = carve(total, 8 * nF), o_fmax = carve(total, 8 * nF), o_rows = carve(total, 8 * C * (size_t)row_stride),
               o_sch = carve(total, 8 * C * GLB_SK), o_ev = carve(total, 8 * C * GLB_EK), o_state = carve(total, 8 * P * GS_SIZE),
               o_mco = carve(total, 8 * 3 * N), o_prob = carve(total, 4 * C), o_done = carve(total, 4 * (P + 1));
  if (plan) {
    plan->scratch_bytes = P > 0 ? (long long)total : 0;
    plan->launches_per_iteration = 4;
    plan->tiles = nt;
    plan->row_doubles = row_stride;
  }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (t->n_problems > 0) {
    if (!t->problem_offset || !t->start || !t->low || !t->high) { *msg = "problems without problem_offset, start, low or high"; return CTR_ERR_INVALID; }
    if (!t->globals || !t->cost || !t->status || !t->n_rounds || !t->n_iter) { *msg = "null output"; return CTR_ERR_INVALID; }
    if (t->n_clusters > 0 && (!t->feat_offset || !t->frame_index)) { *msg = "clusters without feat_offset or frame_index"; return CTR_ERR_INVALID; }
    if (t->n_clusters > 0 && LM > 0 && (!t->local_start || !t->local_low || !t->local_high)) { *msg = "locals without local_start, local_low or local_high"; return CTR_ERR_INVALID; }
    if (t->n_features > 0 && (!t->params || !t->params_out || t->n_frames < 1)) { *msg = "features without params, params_out or frames"; return CTR_ERR_INVALID; }
    if (t->n_frames > 0 && !t->frames) { *msg = "null frames"; return CTR_ERR_INVALID; }
  }
  stage->scratch_bytes = P > 0 ? total : 0;
  if (stage->mode != STAGE_LAUNCH || P == 0) return CTR_OK;

  const hipStream_t s = stage->stream;
  char* ws = (char*)stage->scratch;
  a.frames = t->frames;
  a.frame_dtype = t->frame_dtype;
  a.frame_elems = E;
  a.n_frames = t->n_frames;
  for (int d = 0; d < 3; ++d) { a.fshape[d] = d < t->ndim ? (long)t->shape[d] : 1; a.radius[d] = d < t->ndim ? t->radius[d] : 0; }
  a.ndim = t->ndim;
  a.n_params = t->n_params;
  a.nx = nx;
  a.xbase = base;
  {  // the slots of the evaluation kernel's series (global_kernels.h: NXC) minus the coefficients in use
    const int room = CTR_MAX_PARAMS - base, slots = room < INV_NX ? room : INV_NX;
    a.inv_shift = t->fit_function == CTR_FIT_INV_SERIES ? slots - nx : 0;
  }
  a.LM = LM;
  a.C = t->n_clusters; a.N = t->n_features;
  a.params = t->params; a.feat_offset = t->feat_offset; a.frame_index = t->frame_index;
  a.problem_offset = t->problem_offset;
  a.start = t->start; a.low = t->low; a.high = t->high;
  a.lstart = t->local_start; a.llow = t->local_low; a.lhigh = t->local_high;
  a.params_out = t->params_out; a.globals = t->globals; a.cost = t->cost; a.status = t->status;
  a.n_rounds = t->n_rounds; a.n_iter = t->n_iter;
  a.residual_factor = t->residual_factor; a.max_rms_dev = t->max_rms_dev; a.max_shift = t->max_shift;
  a.xtol = t->xtol; a.ftol = t->ftol;
  a.maxiter = t->solver_maxiter;
  a.max_rounds = t->max_iter;
  a.fmax = (const double*)(ws + o_fmax);
  a.rows = (double*)(ws + o_rows);
  a.row_stride = row_stride;
  a.TP = TP;
  a.sch = (double*)(ws + o_sch);
  a.ev = (double*)(ws + o_ev);
  a.state = (double*)(ws + o_state);
  a.mco = (double*)(ws + o_mco);
  a.prob_of = (int*)(ws + o_prob);
  a.done = (int*)(ws + o_done);
  a.n_done = a.done + P;

  // a failed problem leaves its rows as they came in: the result starts as a copy
  if (N && t->params_out != t->params)
    STAGE_TRY(hipMemcpyAsync(t->params_out, t->params, 8 * N * (size_t)t->n_params, hipMemcpyDeviceToDevice, s));
  // a cluster that no problem owns keeps -1 and is passed over
  if (C) STAGE_TRY(hipMemsetAsync(ws + o_prob, 0xff, 4 * C, s));
  STAGE_TRY(hipMemsetAsync(ws + o_done, 0, 4 * (P + 1), s));
  if (nF) {
    bool too_large = false;
    STAGE_TRY(queue_frame_max(t->frames, t->frame_dtype, t->n_frames, E, (unsigned long long*)(ws + o_enc),
                              (double*)(ws + o_fmax), s, &too_large));
    if (too_large) { *msg = "frame block too large for one launch"; return CTR_ERR_INVALID; }
  }
  hipLaunchKernelGGL(global_setup_kernel, dim3((unsigned)P), dim3(GLB_SETUP_THREADS), 0, s, a);
  const void* ev = eval_kernel(t->ndim, t->isotropic, t->fit_function, nt);
  const unsigned ev_threads = WAVE * glb_waves(nt);
  // A round spends at most solver_maxiter + 1 evaluations and one iteration on its end; the result
  // takes one more.  The device knows what each problem needs next; the host only counts the
  // finished problems, every check_every iterations.
  const long long bound = (long long)t->max_iter * (t->solver_maxiter + 2) + 2;
  int n_done = 0;
  for (long long i = 0; i < bound; ++i) {
    if (C) {
      void* args[] = {&a};
      STAGE_TRY(hipLaunchKernel(ev, dim3((unsigned)C), dim3(ev_threads), args, 0, s));
    }
    hipLaunchKernelGGL(global_judge_kernel, dim3((unsigned)P), dim3(GLB_PROB_THREADS), 0, s, a);
    if (C) hipLaunchKernelGGL(global_factor_kernel, dim3((unsigned)C), dim3(WAVE), 0, s, a);
    hipLaunchKernelGGL(global_solve_kernel, dim3((unsigned)P), dim3(GLB_PROB_THREADS), 0, s, a);
    STAGE_TRY(hipGetLastError());      // a launch that was refused ends the queue here
    if ((i + 1) % t->check_every == 0) {
      STAGE_TRY(hipMemcpyAsync(&n_done, a.n_done, sizeof(int), hipMemcpyDeviceToHost, s));
      STAGE_TRY(hipStreamSynchronize(s));
      if (n_done >= (long long)P) break;
    }
  }
  STAGE_TRY(hipGetLastError());
  STAGE_TRY(hipStreamSynchronize(s));
  return CTR_OK;
}
