// ctrefine.hip -- MI355X (gfx950) cluster-refinement engine behind include/ctrefine.h.
//
// A cluster is fitted start to finish on the chip: window (reference masks.py:30-68),
// elliptical masks (refine.py:43-51), sum-of-Gaussians residual and Jacobian rows
// (fitfunc.py:14-118,436-487), normal equations, bounded / equality-constrained
// Levenberg-Marquardt step, re-window rounds and failure rules (refine.py:343-430).
//
// Kernels:
//   frame_max_kernel      per-frame maximum (refine.py:354); HBM streaming
//   refine_small_kernel   singles / pairs with the default parameter modes: 16 or 64 lanes per
//                         cluster, [J r]^T [J r] accumulated in registers, DPP row all-reduce,
//                         register-resident solve, clusters pulled from a work counter
//   refine_block_kernel   everything else: W wavefronts per cluster, Jacobian rows staged in LDS
//                         and contracted with v_mfma_f64_16x16x4_f64, partial accumulators meet
//                         in LDS, register column-Cholesky (<= 31 variables) or cooperative LDS
//                         Cholesky + range-space KKT step (constraints)
//   refine_tail_kernel    CTR_FLAG_THROUGHPUT: the likely slow pairs and 3-10-feature clusters of a call
//                         in one launch, each fitted by the statements of its bin's own kernel
//   find_clusters_kernel  cluster labelling of a frame (find.py:72-93)
// Clusters are binned by problem size on the host, and the launches of a call decided, once per
// plan (ctr_plan_create, refine_plan.h); the bins run concurrently on the lanes of the device
// (lane_sched.h).  gfx950 only; no CUDA paths, no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "kargs.h"
#include "lane_sched.h"
#include "refine_plan.h"

namespace {

#include "device_common.h"
#include "stage_common.h"
#include "aux_kernels.h"
#include "synth_kernels.h"

// ---- host side ------------------------------------------------------------------------

std::string g_create_error;
std::mutex g_mutex;

}  // namespace

using namespace refine_plan;   // the bins, slots and launches of a plan, and their decision

constexpr int NFAM = CTR_KFAM_LARGE_LOWPASS + 1;   // families of the handle's kernel table (ctr_handle::kernels)
constexpr int GATE_US = 20;  // head start of the block kernels over the small kernels (delay_kernel)

// The duration of one launch of a plan, for the placement of its next call (lane_sched.h): a pair
// of timing events around the kernel, read back without blocking once both have completed.  While
// a pair is pending, later calls of the plan are not timed; nor is every call after the first
// reading (TIMING_EVERY).
constexpr int TIMING_EVERY = 8;
struct LaunchTiming {
  lane_sched::Estimate est;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  bool pending = false;
  int untimed = 0;   // calls since the launch was last timed
};

struct ctr_plan {
  ctr_problem prob;
  int64_t n_clusters = 0;
  int device = 0;
  int32_t* d_order = nullptr;  // all bins back to back; second copy [n_clusters..2n): the order of one call
  int* d_front = nullptr;      // 2 * NBINS counters of front_load_kernel
  // large clusters: workspace in HBM (kargs.h:large_ws) and where each cluster's part begins.
  // The workspace belongs to the plan: calls that use one plan must not overlap in time.
  double* d_ws = nullptr;
  long long* d_ws_off = nullptr;   // [n_clusters] offset in doubles (0 for the other clusters)
  mutable int large_epoch = 0;     // launches of the large kernel on this plan (tags its leader / helper words)
  mutable LaunchTiming timing[NLAUNCH];   // guarded by the mutex of the device's lane pool
  // the bins and every launch of a call, decided once (refine_plan.h: make_plan); a call only
  // places and enqueues them
  RefinePlan rp;
  // lowpass of the window (rp.lowpass; ctr_problem.noise_size): taps per axis on the device (kargs.h: lp_w)
  double* d_lp_w = nullptr;
  int lp_half[3] = {0, 0, 0};
};

// a grow-only block of device memory of a handle (reserve).  event: the end of the last call that
// used it, where calls on several streams share the block (run_stage); null elsewhere
struct Scratch {
  void* ptr = nullptr;
  size_t bytes = 0;
  hipEvent_t event = nullptr;
};

// The lanes of a device: one non-blocking stream per hardware queue (pool_acquire finds them),
// shared by every handle of the device and counted by them.  How many at most: lane_sched.h,
// lanes_from_env(GPU_MAX_HW_QUEUES), read once when the pool is made; it decides where a kernel is
// queued, never what it computes.  mu guards the books and the enqueues of a call: the chains of
// two calls never interleave on a lane otherwise than call by call.
struct LanePool {
  int device = 0, refs = 0;
  std::mutex mu;
  std::vector<hipStream_t> lanes;
  lane_sched::Pool books;
  std::vector<hipEvent_t> spare;   // ticket events (no timing) that have completed, to be recorded again
  explicit LanePool(int n) : books(n) {}
};

struct ctr_handle {
  int device = 0;
  // The handle's own stream: what hip_stream = NULL means to every entry point.  A refine call
  // on it is queued on the lanes alone and leaves `pending` set; whoever names the stream next
  // goes through own_stream(), which makes it wait for that call first (a lazy join: no stream
  // sits in a device-side wait for a call's slowest kernel while nobody asks for its results).
  hipStream_t stream = nullptr;
  LanePool* pool = nullptr;
  bool pending = false;      // ev_done of a call on the own stream has not been joined to `stream`
  // work, or a wait (ctr_engine_wait_stream), was queued on `stream` since the last refine call:
  // the head of the next one waits for an event recorded on the stream, which covers all of it
  bool own_dirty = false;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ev_valid = false;
  std::string err;
  // host-buffer calls; the frame maxima as the kernels encode them and as doubles
  Scratch buf, enc, fmax;
  // the kernel of every cell of the dispatch: [CTR_KFAM_*][ndim-2][iso][slot] (kernel_of); an
  // unreachable cell is null.  attr_set: its dynamic LDS limit is set (table_kernel)
  struct { KernelInfo k; bool attr_set; } kernels[NFAM][2][2][NSLOT] = {};
  KernelInfo tail[2] = {};        // refine_tail_kernel by iso (2D); tail_attr_set: its dynamic LDS limit is set
  bool tail_attr_set[2] = {false, false};
  int32_t tail_absorb = TAIL_ABSORB;   // ctr_set_tail_absorb: for the plans made from now on
  hipEvent_t ev_done = nullptr;   // end of the last ctr_refine_batch_device call of this handle
  // ev_fork / ev_gate: the head chain of a call has prepared it / its small kernels may start;
  // ev_order: ctr_stream_wait_engine / ctr_engine_wait_stream; ev_own: what was queued
  // on the own stream before a call
  hipEvent_t ev_fork = nullptr, ev_gate = nullptr, ev_order = nullptr, ev_own = nullptr;
  int* d_counter = nullptr;       // work counters of the small-kernel launches
  // ctr_link_device, ctr_find_link_device and ctr_find_link_refine_device; ctr_diffusion_device and ctr_diffusion_ci_device (partial sums, rows, statistics)
  Scratch link, motion;
  Scratch train;   // ctr_train_device: frame maxima, partial sums, solver state
  Scratch global;  // ctr_refine_global_device: frame maxima, a row per cluster, Schur and evaluation tables, solver state
  Scratch tracks;  // ctr_cluster_tracks_device: labels, member counts, the words of the rounds
  Scratch prepare; // ctr_refine_prepare_device: scaled positions, member counts, ranks, clusters per frame
  Scratch drift;   // ctr_drift_device: the step of every frame
  Scratch msd;     // ctr_msd_device, ctr_emsd_device, ctr_vanhove_device: the sorted rows, row ranges, partials of the chunks
  Scratch pcf;     // ctr_pair_correlation_device: the work items of the frames, their partial weights
  Scratch nbr;     // ctr_neighbors_device: the work items of the frames, the keys of the particles
  Scratch twopt;   // ctr_twopoint_device: the work items of the frames, the partner's row of every row and lag
  Scratch shape;   // ctr_shape_dynamics_device, ctr_shape_histogram_device: the coordinates of every frame, the partials of the tiles
  Scratch resid;   // ctr_residual_device: the residual and owner of every pixel where the caller takes no frames, the frame maxima
  Scratch contacts;  // ctr_contacts_device: the work items of the frames, the sums of the scan tiles, the chains, episodes and pairs of the entries
  Scratch fiterr;  // ctr_fit_error_device: the word of the table check, the frame maxima
  unsigned stage_max_grid = STAGE_MAX_GRID;   // run_stage: StageRun::max_grid (ctr_set_stage_max_grid)
};

namespace {

int fail(ctr_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  else { std::lock_guard<std::mutex> g(g_mutex); g_create_error = msg; }
  return code;
}

#define HIP_TRY(h, call)                                                                   \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(h, CTR_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_));   \
  } while (0)

// ---- the lanes (LanePool) ------------------------------------------------------------------
// by device.  A mutex of their own: the first handle of a device holds it through the trial of
// pool_acquire (device synchronises, 10-20 ms), which must not block ctr_last_error and the like
std::map<int, LanePool*> g_pools;
std::mutex g_pool_mutex;

// Is `cand` served by a hardware queue that none of `lanes` (on distinct queues themselves) is on?
// A queue is served in order: with a delay kernel on every lane, one more on cand, queued last,
// ends one delay after it was queued when cand has a queue to itself, and nearly two when it
// stands behind a lane's (nearly: the lanes' kernels were queued a few us each earlier -- with a
// delay of 400 us and nine lanes that difference already hid a queue of its own).  Measured on the
// host, the best of three (whatever else the machine does can only lengthen a run: a wrong answer
// costs a lane, never a result).
constexpr unsigned PROBE_US = 1000;
bool on_new_queue(const std::vector<hipStream_t>& lanes, hipStream_t cand) {
  for (int rep = 0; rep < 3; ++rep) {
    for (hipStream_t st : lanes) (void)hipStreamSynchronize(st);
    (void)hipStreamSynchronize(cand);
    for (hipStream_t st : lanes) hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(WAVE), 0, st, (unsigned long long)PROBE_US * 100ull);
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(WAVE), 0, cand, (unsigned long long)PROBE_US * 100ull);
    bool ok = hipGetLastError() == hipSuccess;
    ok = hipStreamSynchronize(cand) == hipSuccess && ok;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    for (hipStream_t st : lanes) ok = hipStreamSynchronize(st) == hipSuccess && ok;
    if (!ok) return true;   // (no answer: keep the stream)
    if (us < 1.5 * PROBE_US) return true;
  }
  return false;
}

// the pool of the device, made by its first handle; null: its streams could not be created.
// How the runtime deals streams to the hardware queues is its own business (measured here: the
// first GPU_MAX_HW_QUEUES streams of a process open a queue each, a later one joins the queue with
// the fewest streams -- four streams made back to back by the first handle landed on three
// queues), so the lanes are found by trial: streams are made until as many as there are queues
// have proved to be on queues of their own, or three times that many have been tried; the
// others are destroyed again.  (The device is current.)
LanePool* pool_acquire(int device) {
  std::lock_guard<std::mutex> g(g_pool_mutex);
  LanePool*& slot = g_pools[device];
  if (!slot) {
    const int want = lane_sched::lanes_from_env(std::getenv("GPU_MAX_HW_QUEUES"));
    std::vector<hipStream_t> lanes, rejected;
    {
      hipStream_t warm = nullptr;   // (the first launch of a kernel loads its code: not part of a trial)
      if (hipStreamCreateWithFlags(&warm, hipStreamNonBlocking) != hipSuccess) { g_pools.erase(device); return nullptr; }
      hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(WAVE), 0, warm, 100ull);
      (void)hipStreamSynchronize(warm);
      (void)hipGetLastError();
      rejected.push_back(warm);
    }
    for (int tried = 0; (int)lanes.size() < want && tried < 3 * want; ++tried) {
      hipStream_t st = nullptr;
      if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) break;
      (lanes.empty() || on_new_queue(lanes, st) ? lanes : rejected).push_back(st);
    }
    // (the rejected streams lived until here: each kept its queue less attractive for the next)
    for (hipStream_t st : rejected) (void)hipStreamDestroy(st);
    if (lanes.empty()) { g_pools.erase(device); return nullptr; }
    LanePool* p = new LanePool((int)lanes.size());
    p->device = device;
    p->lanes = lanes;
    slot = p;
  }
  slot->refs++;
  return slot;
}

bool ticket_done(void*, lane_sched::EventId ev) { return hipEventQuery((hipEvent_t)ev) != hipErrorNotReady; }

// the last handle of a device takes the pool with it, once its lanes have run dry
void pool_release(LanePool* p) {
  if (!p) return;
  std::lock_guard<std::mutex> g(g_pool_mutex);
  if (--p->refs > 0) return;
  g_pools.erase(p->device);
  for (hipStream_t st : p->lanes) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
  std::vector<lane_sched::EventId> retired;
  p->books.retire([](void*, lane_sched::EventId) { return true; }, nullptr, &retired);
  for (lane_sched::EventId ev : retired) (void)hipEventDestroy((hipEvent_t)ev);
  for (hipEvent_t ev : p->spare) (void)hipEventDestroy(ev);
  delete p;
}

// a ticket event of the pool, recorded on the lane at the end of a chain; booked with the chain's
// estimate.  (p->mu is held.)
hipError_t lane_ticket(LanePool* p, int lane, double ms, hipEvent_t* out) {
  hipEvent_t ev = nullptr;
  if (!p->spare.empty()) { ev = p->spare.back(); p->spare.pop_back(); }
  else if (hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) return e;
  if (hipError_t e = hipEventRecord(ev, p->lanes[(size_t)lane])) { p->spare.push_back(ev); return e; }
  p->books.push(lane, (lane_sched::EventId)ev, ms);
  *out = ev;
  return hipSuccess;
}

// The handle's own stream for whoever queues work on it or waits for it: joined with the handle's
// pending refine call first (ctr_handle::stream).
hipStream_t own_stream(ctr_handle* h) {
  if (h->pending) {
    (void)hipStreamWaitEvent(h->stream, h->ev_done, 0);
    h->pending = false;
  }
  h->own_dirty = true;
  return h->stream;
}

int validate(const ctr_problem* p, std::string& msg) {
  if (!p) { msg = "null problem"; return CTR_ERR_INVALID; }
  if (p->ndim != 2 && p->ndim != 3) { msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (p->fit_function < CTR_FIT_GAUSS || p->fit_function > CTR_FIT_INV_SERIES) { msg = "unknown fit function"; return CTR_ERR_INVALID; }
  const bool other_profile = p->fit_function != CTR_FIT_GAUSS;
  // ring: 'thickness', disc: 'disc_size' -- one more column after the sizes (fitfunc.py:195-204);
  // inv_series_<N>: 'signal_mult', 'param_a', ... N + 1 columns (fitfunc.py:334-343)
  const int base = 2 + p->ndim + (p->isotropic ? 1 : p->ndim);
  int np = base + (other_profile ? 1 : 0);
  if (p->fit_function == CTR_FIT_INV_SERIES) {
    if (p->n_params < base + 1) { msg = "inv_series needs at least the column 'signal_mult'"; return CTR_ERR_INVALID; }
    if (p->n_params > CTR_MAX_PARAMS) { msg = "inv_series: more than CTR_MAX_PARAMS parameter columns"; return CTR_ERR_UNSUPPORTED; }
    np = p->n_params;
  }
  if (p->n_params != np) { msg = "n_params does not match ndim/isotropic"; return CTR_ERR_INVALID; }
  for (int k = 0; k < np; ++k) {
    const int m = p->modes[k];
    if (m == CTR_MODE_GLOBAL) { msg = "param mode 'global' couples all clusters and is not supported"; return CTR_ERR_UNSUPPORTED; }
    if (m != CTR_MODE_CONST && m != CTR_MODE_VAR && m != CTR_MODE_CLUSTER) { msg = "unknown param mode"; return CTR_ERR_INVALID; }
  }
  if (p->modes[0] == CTR_MODE_VAR) { msg = "background cannot vary per feature (fitfunc.py:389-392)"; return CTR_ERR_INVALID; }
  for (int a = 0; a < p->ndim; ++a)
    if (p->radius[a] < 1) { msg = "radius must be >= 1"; return CTR_ERR_INVALID; }
  if (p->max_iter < 1) { msg = "max_iter must be >= 1"; return CTR_ERR_INVALID; }
  if (p->constraint_kind < CTR_CONS_NONE || p->constraint_kind > CTR_CONS_TETRAMER) { msg = "unknown constraint kind"; return CTR_ERR_INVALID; }
  if (p->constraint_kind != CTR_CONS_NONE)
    for (int a = 0; a < p->ndim; ++a)
      if (!(p->constraint_dist[a] > 0.)) { msg = "constraint distance must be positive"; return CTR_ERR_INVALID; }
  if (!(p->residual_factor > 0.)) { msg = "residual_factor must be positive"; return CTR_ERR_INVALID; }
  for (int a = 0; a < p->ndim; ++a)
    if (!(p->noise_size[a] >= 0.) || p->noise_size[a] > CTR_MAX_NOISE_SIZE) {
      msg = "noise_size must be between 0 and CTR_MAX_NOISE_SIZE";
      return CTR_ERR_INVALID;
    }
  if (p->threshold != p->threshold) { msg = "threshold is NaN"; return CTR_ERR_INVALID; }
  if (other_profile) {
    bool lp = (p->flags & CTR_FLAG_WINDOW_FILTER) != 0;
    for (int a = 0; a < p->ndim; ++a) lp = lp || p->noise_size[a] > 0.;
    if (lp) { msg = "noise_size together with a profile other than gauss is not implemented"; return CTR_ERR_UNSUPPORTED; }
  }
  return CTR_OK;
}

// trackpy.masks.gaussian_kernel(sigma, truncate=4), the taps of the reference's lowpass
// (preprocessing.py:43).  trackpy is not part of the reference's tree: restated from its
// published source (lw = int(4 sigma + 0.5); exp(x^2 / (-2 sigma^2)) / sum, numpy's pairwise
// sum for short arrays); the same code as oracle/ctr_oracle.c:ctro_gaussian_kernel.
int gaussian_taps(double sigma, double* w) {
  const int lw = (int)(4.0 * sigma + 0.5), nw = 2 * lw + 1;
  double sum;
  for (int i = 0; i < nw; ++i) {
    const double x = (double)(i - lw);
    w[i] = std::exp((x * x) / (-2. * (sigma * sigma)));
  }
  if (nw < 8) {
    sum = 0.;
    for (int i = 0; i < nw; ++i) sum += w[i];
  } else {
    double r[8];
    int i;
    for (int j = 0; j < 8; ++j) r[j] = w[j];
    for (i = 8; i < nw - (nw % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += w[i + j];
    sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < nw; ++i) sum += w[i];
  }
  for (int i = 0; i < nw; ++i) w[i] /= sum;
  return lw;
}

// at least `need` bytes in sc.  A block that grows is replaced once the device is idle: a kernel
// of an earlier call, on whichever stream, may still use the old one.
int reserve(ctr_handle* h, Scratch& sc, size_t need, const char* or_else) {
  if (need <= sc.bytes) return CTR_OK;
  if (sc.ptr) { HIP_TRY(h, hipDeviceSynchronize()); (void)hipFree(sc.ptr); sc.ptr = nullptr; sc.bytes = 0; }
  if (hipMalloc(&sc.ptr, need) != hipSuccess) { sc.ptr = nullptr; return fail(h, CTR_ERR_NOMEM, or_else); }
  sc.bytes = need;
  return CTR_OK;
}

int ensure_fmax(ctr_handle* h, int64_t n_frames) {
  const int rc = reserve(h, h->enc, sizeof(unsigned long long) * (size_t)n_frames, "cannot allocate the frame maxima on the device");
  return rc ? rc : reserve(h, h->fmax, sizeof(double) * (size_t)n_frames, "cannot allocate the frame maxima on the device");
}

// What every ctr_<stage>_device call does around its stage unit (kargs.h: StageRun).  The
// descriptor is checked before the handle is touched: a bad one is reported (through
// ctr_last_error of a null handle) even where there is no device to make a handle on.  scratch:
// the block of the handle that the stage uses, or null; calls that share a block run one after
// the other on the device, in the order of the calls, whichever their streams.  A stage with
// scratch that asks for no byte has nothing to launch.
template <class D, class... Extra>
int run_stage(const char* name, ctr_handle* h, Scratch ctr_handle::*scratch, const D* d, void* hip_stream,
              int (*launch)(const D*, StageRun*, const char**, Extra*...)) {
  const char* msg = "";
  auto failed = [&](int rc, const char* why) { return fail(h, rc, std::string(name) + ": " + why); };
  StageRun run = {STAGE_CHECK, nullptr, nullptr, 0, h ? h->stage_max_grid : STAGE_MAX_GRID};
  int rc = launch(d, &run, &msg, (Extra*)nullptr...);
  if (rc != CTR_OK) return failed(rc, msg);
  if (!h) return failed(CTR_ERR_INVALID, "null handle");
  if (scratch && run.scratch_bytes == 0) return CTR_OK;   // nothing to launch: the device is not touched
  HIP_TRY(h, hipSetDevice(h->device));
  run.mode = STAGE_LAUNCH;
  run.stream = hip_stream ? (hipStream_t)hip_stream : own_stream(h);
  Scratch* sc = scratch ? &(h->*scratch) : nullptr;
  if (sc) {
    if (!sc->event) HIP_TRY(h, hipEventCreateWithFlags(&sc->event, hipEventDisableTiming));
    else HIP_TRY(h, hipStreamWaitEvent(run.stream, sc->event, 0));
    rc = reserve(h, *sc, run.scratch_bytes, "cannot allocate the scratch on the device");
    if (rc != CTR_OK) return failed(rc, h->err.c_str());
    run.scratch = sc->ptr;
  }
  rc = launch(d, &run, &msg, (Extra*)nullptr...);
  if (rc != CTR_OK) return failed(rc, msg);
  if (sc) HIP_TRY(h, hipEventRecord(sc->event, run.stream));
  return CTR_OK;
}

int launch_frame_max(ctr_handle* h, const void* frames, int dtype, int64_t n_frames,
                     int64_t frame_elems, double* out, hipStream_t s) {
  const size_t isz = host_dtype_size(dtype);
  if (!isz) return fail(h, CTR_ERR_INVALID, "unknown frame dtype");
  if (n_frames <= 0) return CTR_OK;
  int rc = ensure_fmax(h, n_frames);
  if (rc) return rc;
  bool too_large = false;
  const hipError_t e = queue_frame_max(frames, dtype, n_frames, frame_elems, (unsigned long long*)h->enc.ptr, out, s, &too_large);
  if (too_large) return fail(h, CTR_ERR_INVALID, "frame block too large for one launch");
  HIP_TRY(h, e);
  return CTR_OK;
}

// The instantiation of one cell of the kernel table (ctr_create); {nullptr} where there is none.
KernelInfo kernel_of(int fam, int ndim, int iso, int slot) {
  const KernelInfo none{nullptr, 0, 0};
  if (fam == CTR_KFAM_NONE) return none;
  if (fam == CTR_KFAM_SMALL) {
    static const int tier[4][2] = {{1, 8}, {1, 64}, {2, 64}, {2, 16}};   // (features, lanes) by slot
    if (slot > SLOT_PAIRS16) return none;
    return KernelInfo{ctr_small_kernel(ndim, tier[slot][0], iso, tier[slot][1]), 0, WAVE};
  }
  if (fam == CTR_KFAM_LARGE || fam == CTR_KFAM_LARGE_LOWPASS)
    return slot == 0 ? ctr_large_kernel(ndim, iso, fam == CTR_KFAM_LARGE_LOWPASS) : none;
  typedef KernelInfo (*block_unit)(int, int, int, int, int);
  static const block_unit units[] = {ctr_block_kernel_2d, ctr_block_kernel_3d, ctr_block_kernel_lp,
                                     ctr_block_kernel_fit2d, ctr_block_kernel_fit3d, ctr_block_kernel_inv};
  for (block_unit unit : units) {
    const KernelInfo k = unit(fam, ndim, iso, slot % MAXNT + 1, slot >= MAXNT);
    if (k.fn) return k;
  }
  return none;
}

// The kernel of a cell, its dynamic LDS limit set the first time it is launched.  A cell without
// an instantiation is an error (the plan's decision and the table disagree), never a launch.
int table_kernel(ctr_handle* h, int fam, int ndim, int iso, int slot, const KernelInfo** out) {
  auto& e = h->kernels[fam][ndim - 2][iso][slot];
  if (!e.k.fn)
    return fail(h, CTR_ERR_DEVICE, "no kernel instantiated for family " + std::to_string(fam) + ", " +
                                       std::to_string(ndim) + "D, iso " + std::to_string(iso) + ", slot " + std::to_string(slot));
  if (!e.attr_set) {
    if (e.k.smem > 0)   // (the small kernels have no dynamic LDS)
      HIP_TRY(h, hipFuncSetAttribute(e.k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e.k.smem));
    e.attr_set = true;
  }
  *out = &e.k;
  return CTR_OK;
}

}  // namespace

extern "C" {

int ctr_abi_version(void) { return CTR_ABI_VERSION; }

const char* ctr_last_error(const ctr_handle* h) {
  if (h) return h->err.c_str();
  return g_create_error.c_str();
}

int ctr_validate_problem(const ctr_problem* p, char* msg, int msg_len) {
  std::string m;
  const int rc = validate(p, m);
  if (msg && msg_len > 0) {
    std::snprintf(msg, (size_t)msg_len, "%s", m.c_str());
  }
  return rc;
}

int ctr_cluster_n_vars(const ctr_problem* p, int n_features) { return p ? n_vars(p, n_features) : -1; }

int ctr_cluster_kernel(const ctr_problem* p, int64_t n_features, ctr_kernel_choice* out) {
  if (!out) return CTR_ERR_INVALID;
  std::string msg;
  std::memset(out, 0, sizeof *out);
  out->n_vars = -1;
  if (validate(p, msg) || n_features < 0) return CTR_ERR_INVALID;
  if (n_features <= 0x3fffffLL) out->n_vars = n_vars(p, (int)n_features);
  const KernelChoice c = choose_kernel(p, n_features);
  out->family = c.family;
  if (c.bin < MAXNT) { out->bin = CTR_KBIN_BLOCK; out->nt = c.bin + 1; }
  else if (c.bin == BIN_CONS1 || c.bin == BIN_CONS2) { out->bin = CTR_KBIN_CONS; out->nt = c.bin == BIN_CONS1 ? 1 : 2; }
  else if (c.bin == BIN_SMALL1 || c.bin == BIN_SMALL2) {
    out->bin = c.bin == BIN_SMALL1 ? CTR_KBIN_SMALL1 : CTR_KBIN_SMALL2;
    out->lanes = c.slot == SLOT_SINGLES8 ? 8 : 64;
  }
  else out->bin = c.bin == BIN_LARGE ? CTR_KBIN_LARGE : CTR_KBIN_TOO_LARGE;
  return CTR_OK;
}

int ctr_create(ctr_handle** out, int device) {
  if (!out) return fail(nullptr, CTR_ERR_INVALID, "null out pointer");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(nullptr, CTR_ERR_DEVICE, std::string("no HIP device visible (") + hipGetErrorString(e) + "); there is no CPU fallback");
  if (device < 0 || device >= count) return fail(nullptr, CTR_ERR_INVALID, "device index out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, CTR_ERR_DEVICE, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, CTR_ERR_DEVICE, std::string("device is ") + prop.gcnArchName + ", this engine is built for gfx950 (MI355X) only");
  ctr_handle* h = new ctr_handle();
  h->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return fail(nullptr, CTR_ERR_DEVICE, "cannot create a stream on the device");
  }
  for (auto& ev : h->ev)
    if (hipEventCreate(&ev) != hipSuccess) { delete h; return fail(nullptr, CTR_ERR_DEVICE, "hipEventCreate failed"); }
  bool evok = true;
  for (hipEvent_t* ev : {&h->ev_fork, &h->ev_gate, &h->ev_order, &h->ev_own, &h->ev_done})
    evok = evok && hipEventCreateWithFlags(ev, hipEventDisableTiming) == hipSuccess;
  if (!evok || hipMalloc((void**)&h->d_counter, sizeof(int) * 8) != hipSuccess) { ctr_destroy(h); return fail(nullptr, CTR_ERR_DEVICE, "cannot create events / counters"); }
  h->pool = pool_acquire(device);
  if (!h->pool) { ctr_destroy(h); return fail(nullptr, CTR_ERR_DEVICE, "cannot create the lanes of the device"); }
  for (int fam = 0; fam < NFAM; ++fam)
    for (int di = 0; di < 2; ++di)
      for (int ii = 0; ii < 2; ++ii)
        for (int slot = 0; slot < NSLOT; ++slot) h->kernels[fam][di][ii][slot].k = kernel_of(fam, 2 + di, ii, slot);
  for (int ii = 0; ii < 2; ++ii) h->tail[ii] = ctr_tail_kernel(2, ii);
  *out = h;
  return CTR_OK;
}

void ctr_destroy(ctr_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  // the last refine call, wherever its chains run, uses the handle's scratch until ev_done
  if (h->ev_done) (void)hipEventSynchronize(h->ev_done);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (Scratch* sc : {&h->buf, &h->enc, &h->fmax, &h->link, &h->motion, &h->train, &h->global, &h->tracks, &h->prepare, &h->drift, &h->msd, &h->pcf, &h->nbr, &h->twopt, &h->shape, &h->resid, &h->contacts, &h->fiterr}) {
    if (sc->ptr) (void)hipFree(sc->ptr);
    if (sc->event) (void)hipEventDestroy(sc->event);
  }
  for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : {h->ev_fork, h->ev_gate, h->ev_order, h->ev_own, h->ev_done})
    if (ev) (void)hipEventDestroy(ev);
  if (h->d_counter) (void)hipFree(h->d_counter);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  pool_release(h->pool);
  delete h;
}

int ctr_plan_create(ctr_handle* h, const ctr_problem* p, int64_t n_clusters,
                    const int32_t* feat_offset_host, ctr_plan** out) {
  if (!h || !out) return CTR_ERR_INVALID;
  *out = nullptr;
  std::string msg;
  int rc = validate(p, msg);
  if (rc) return fail(h, rc, msg);
  if (n_clusters < 0 || (n_clusters > 0 && !feat_offset_host)) return fail(h, CTR_ERR_INVALID, "bad cluster table");
  if (n_clusters > 0x7ffffff0LL) return fail(h, CTR_ERR_INVALID, "too many clusters for one batch");
  ctr_plan* plan = new ctr_plan();
  plan->prob = *p;
  plan->n_clusters = n_clusters;
  plan->device = h->device;
  std::vector<int32_t> order, bin_of;
  if (const char* why = make_plan(p, n_clusters, feat_offset_host, h->tail_absorb, &plan->rp, &order, &bin_of)) {
    delete plan;
    return fail(h, CTR_ERR_INVALID, why);
  }
  // the workspace of the large clusters (large_ws), one after the other
  std::vector<long long> ws_off((size_t)n_clusters, 0);
  long long ws_total = 0;
  if (plan->rp.bin_count[BIN_LARGE] > 0) {
    const int nsh = n_vars(p, 0), npf = n_vars(p, 1) - nsh;   // shared / per-feature variables
    for (int64_t c = 0; c < n_clusters; ++c) {
      if (bin_of[(size_t)c] != BIN_LARGE) continue;
      ws_off[(size_t)c] = ws_total;
      ws_total += large_ws(feat_offset_host[c + 1] - feat_offset_host[c], npf, nsh, window_volume(p)).total;
    }
  }
  if (n_clusters > 0) {
    if (hipSetDevice(h->device) != hipSuccess ||
        hipMalloc((void**)&plan->d_order, sizeof(int32_t) * 2 * (size_t)n_clusters) != hipSuccess ||
        hipMalloc((void**)&plan->d_front, sizeof(int) * 2 * NBINS) != hipSuccess) {
      ctr_plan_destroy(plan);
      return fail(h, CTR_ERR_NOMEM, "cannot allocate the plan on the device");
    }
    if (hipMemcpy(plan->d_order, order.data(), sizeof(int32_t) * (size_t)n_clusters, hipMemcpyHostToDevice) != hipSuccess) {
      ctr_plan_destroy(plan);
      return fail(h, CTR_ERR_DEVICE, "cannot upload the plan");
    }
    if (plan->rp.lowpass) {
      std::vector<double> taps(3 * LP_STRIDE, 0.);
      for (int a = 0; a < p->ndim; ++a) {
        if (p->noise_size[a] > 0.) plan->lp_half[a] = gaussian_taps(p->noise_size[a], taps.data() + a * LP_STRIDE);
        else taps[(size_t)a * LP_STRIDE] = 1.;   // this axis is not filtered
      }
      if (hipMalloc((void**)&plan->d_lp_w, sizeof(double) * taps.size()) != hipSuccess ||
          hipMemcpy(plan->d_lp_w, taps.data(), sizeof(double) * taps.size(), hipMemcpyHostToDevice) != hipSuccess) {
        ctr_plan_destroy(plan);
        return fail(h, CTR_ERR_NOMEM, "cannot upload the lowpass taps");
      }
    }
    if (ws_total > 0) {
      if (hipMalloc((void**)&plan->d_ws, sizeof(double) * (size_t)ws_total) != hipSuccess ||
          hipMalloc((void**)&plan->d_ws_off, sizeof(long long) * (size_t)n_clusters) != hipSuccess) {
        ctr_plan_destroy(plan);
        return fail(h, CTR_ERR_NOMEM, "cannot allocate the workspace of the large clusters on the device");
      }
      // (the leader / helper words of every cluster start at zero: no epoch matches)
      if (hipMemset(plan->d_ws, 0, sizeof(double) * (size_t)ws_total) != hipSuccess ||
          hipMemcpy(plan->d_ws_off, ws_off.data(), sizeof(long long) * (size_t)n_clusters, hipMemcpyHostToDevice) != hipSuccess) {
        ctr_plan_destroy(plan);
        return fail(h, CTR_ERR_DEVICE, "cannot upload the plan");
      }
    }
  }
  *out = plan;
  return CTR_OK;
}

void ctr_plan_destroy(ctr_plan* plan) {
  if (!plan) return;
  if (plan->d_order) { (void)hipSetDevice(plan->device); (void)hipFree(plan->d_order); }
  if (plan->d_front) (void)hipFree(plan->d_front);
  if (plan->d_ws) (void)hipFree(plan->d_ws);
  if (plan->d_ws_off) (void)hipFree(plan->d_ws_off);
  if (plan->d_lp_w) (void)hipFree(plan->d_lp_w);
  for (LaunchTiming& t : plan->timing) {
    if (t.t0) (void)hipEventDestroy(t.t0);
    if (t.t1) (void)hipEventDestroy(t.t1);
  }
  delete plan;
}

int ctr_plan_tail(const ctr_plan* plan, int32_t* fused, int32_t* cap, int32_t* tail_grid) {
  if (!plan) return CTR_ERR_INVALID;
  if (fused) *fused = plan->rp.tail_fused ? 1 : 0;
  if (cap) *cap = TAIL_CAP;
  if (tail_grid) *tail_grid = plan->rp.tail_grid;
  return CTR_OK;
}

int ctr_plan_tail_bins(const ctr_plan* plan, int32_t* absorbed, int32_t* own_launch) {
  if (!plan) return CTR_ERR_INVALID;
  for (int sgm = 0; sgm < TAIL_SEGMENTS; ++sgm) {
    if (absorbed) absorbed[sgm] = plan->rp.tail_whole[sgm] ? 1 : 0;
    if (own_launch) own_launch[sgm] = plan->rp.tail_own[sgm] ? 1 : 0;
  }
  return CTR_OK;
}

int32_t ctr_set_tail_absorb(ctr_handle* h, int32_t max_count) {
  if (!h) return -1;
  const int32_t before = h->tail_absorb;
  if (max_count >= 0) h->tail_absorb = max_count;
  return before;
}

int ctr_frame_max_device(ctr_handle* h, const void* frames, int32_t frame_dtype, int64_t n_frames,
                         int64_t frame_elems, double* out_max, void* hip_stream) {
  if (!h) return CTR_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : own_stream(h);
  return launch_frame_max(h, frames, frame_dtype, n_frames, frame_elems, out_max, s);
}

int ctr_refine_batch_device(ctr_handle* h, const ctr_plan* plan, const ctr_batch* b, void* hip_stream) {
  if (!h || !plan || !b) return CTR_ERR_INVALID;
  if (b->n_clusters != plan->n_clusters) return fail(h, CTR_ERR_INVALID, "batch does not match the plan");
  const ctr_problem& p = plan->prob;
  if (!host_dtype_size(b->frame_dtype)) return fail(h, CTR_ERR_INVALID, "unknown frame dtype");
  for (int a = 0; a < p.ndim; ++a)
    if (b->shape[a] < 1) return fail(h, CTR_ERR_INVALID, "frame shape must be positive");
  HIP_TRY(h, hipSetDevice(h->device));
  // A call is a set of chains, each a run of work for one stream:
  //   head    waits for the handle's previous call and for what the caller ordered before this one,
  //           then frame maxima, counters and this call's order of the clusters; records ev_fork
  //           (and, after the delay of the gate, ev_gate)
  //   bins    one chain per kernel launch: waits for ev_fork (the small kernels for ev_gate),
  //           runs the kernel; the tail launch of a plan that has one is such a chain
  //   finish  waits for every bin chain, then result rows, done flag, ev_done
  // The bin chains go to the lanes of the device.  On a caller's stream the contract is stream
  // order: head and finish stay on that stream.  On the handle's own stream (hip_stream = NULL)
  // they go to lanes as well, nothing is queued on the stream itself and the call is left pending
  // (own_stream).
  // INVARIANT: a chain only waits for events that were recorded earlier in host order -- a call is
  // enqueued head, bins, finish, under the pool's mutex, and its head waits for events of earlier
  // calls alone.  Host order is therefore a valid order of execution for every placement, one lane
  // for everything included: no chain can wait for something behind it in its own lane.
  const bool own = hip_stream == nullptr;
  LanePool* const pool = h->pool;
  int64_t frame_elems = 1;
  for (int a = 0; a < p.ndim; ++a) frame_elems *= b->shape[a];
  h->ev_valid = false;
  int rc = ensure_fmax(h, b->n_frames > 0 ? b->n_frames : 1);
  if (rc) return rc;

  // squared relative residual tolerances of the large kernel's conjugate-gradient solve, far from /
  // near the solution (with the aggregated preconditioner 1e-8 far saves 12 % and costs parity:
  // 6e-7 vs 5e-8 px against the oracle)
  constexpr double LARGE_CG_TOL2_FAR = 1e-12, LARGE_CG_TOL2_NEAR = 1e-22;
  // what every launch of the call gets; a launch adds its bin and its part of it (LaunchSpec)
  const KArgs base = [&] {
    KArgs k;
    std::memset(&k, 0, sizeof k);   // (no order, n_bin 0; split = nullptr: a launch takes its whole bin)
    k.prob = p;
    k.frames = b->frames;
    k.frame_dtype = b->frame_dtype;
    for (int a = 0; a < 3; ++a) k.shape[a] = a < p.ndim ? b->shape[a] : 1;
    k.frame_elems = frame_elems;
    k.frame_index = b->frame_index;
    k.feat_offset = b->feat_offset;
    k.params = b->params;
    k.low = b->low;
    k.high = b->high;
    k.params_out = b->params_out;
    k.cost = b->cost;
    k.status = b->status;
    k.n_rounds = b->n_rounds;
    k.n_iter = b->n_iter;
    k.params_std = b->params_std;
    k.fmax = (const double*)h->fmax.ptr;
    k.lp_w = plan->rp.lowpass ? plan->d_lp_w : nullptr;
    k.cg_tol2_far = LARGE_CG_TOL2_FAR;
    k.cg_tol2_near = LARGE_CG_TOL2_NEAR;
    for (int a = 0; a < 3; ++a) k.lp_half[a] = plan->lp_half[a];
    return k;
  }();
  const int ii = p.isotropic ? 1 : 0;
  // From here on the pool's mutex is held: the plan's timing entries (their guesses included) and
  // the lanes' books belong to it.  An error return in the middle of the enqueue (HIP_TRY) leaves
  // what was queued so far queued, its tickets booked -- they retire when their events complete --
  // and ev_done of this call unrecorded: the handle's next call then waits for the call before
  // this one, as after any failed call, and the caller is told that this one failed.
  std::lock_guard<std::mutex> lock(pool->mu);
  // this call's order inside the bins: likely stragglers first (front_load_kernel)
  int32_t* ord = plan->d_order + plan->n_clusters;
  // The bins are independent: every launch is a chain of its own, so that a few slow many-feature
  // clusters overlap with the bulk.  The chains are made first -- a missing kernel is reported
  // before anything is queued -- and enqueued in the order of their placement.  launch: the entry
  // of plan->timing; gated: starts with the small kernels; run: queues the chain's kernels.
  // (CTR_FLAG_ISOLATE_TAIL changes nothing here: the placement below keeps a long kernel out of
  // the way of the others by its measured duration, whichever bin it belongs to.)
  struct Chain {
    int launch;
    bool gated;
    std::function<hipError_t(hipStream_t)> run;
  };
  std::vector<Chain> chains;
  // Which launches, with which grid, gate, counter and part of a bin: the plan's list
  // (refine_plan.h), in the order in which the placement gets them.
  const RefinePlan& rp = plan->rp;
  for (const LaunchSpec& sp : rp.launches) {
    const KernelInfo* ki = nullptr;
    if (sp.kind == KIND_TAIL) {
      ki = &h->tail[ii];
      if (!ki->fn) return fail(h, CTR_ERR_DEVICE, "no tail kernel instantiated for this problem");
      if (!h->tail_attr_set[ii]) {
        HIP_TRY(h, hipFuncSetAttribute(ki->fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ki->smem));
        h->tail_attr_set[ii] = true;
      }
    } else if (sp.kind != KIND_MARK) {
      rc = table_kernel(h, sp.family, p.ndim, ii, sp.slot, &ki);
      if (rc) return rc;
    }
    KArgs k = base;
    k.order = sp.bin < 0 ? ord : ord + rp.bin_begin[sp.bin];
    k.n_bin = sp.bin < 0 ? 0 : (int32_t)rp.bin_count[sp.bin];
    k.split = sp.split ? plan->d_front + 2 * sp.bin : nullptr;
    k.split_part = sp.split_part;
    k.split_cap = sp.split_cap;
    plan->timing[sp.launch].est.guess = lane_sched::static_guess(sp.cls, sp.count, sp.nt);
    const int kind = sp.kind;
    const bool delay = sp.delay_first;
    const unsigned grid = (unsigned)sp.grid;
    int* counter = sp.counter < 0 ? nullptr : h->d_counter + sp.counter;   // (the tail launch: one per segment)
    TailArgs ta;
    std::memset(&ta, 0, sizeof ta);
    for (int sgm = 0; kind == KIND_TAIL && sgm < TAIL_SEGMENTS; ++sgm) {
      ta.close[sgm] = rp.bin_count[TAIL_BINS[sgm]] > 0 ? plan->d_front + 2 * TAIL_BINS[sgm] : nullptr;
      ta.ord_off[sgm] = rp.tail.ord_off[sgm];
      ta.whole[sgm] = rp.tail.whole[sgm];
    }
    for (int sgm = 0; sgm <= TAIL_SEGMENTS; ++sgm) ta.grid_begin[sgm] = rp.tail.grid_begin[sgm];
    double* wsp = plan->d_ws;
    const long long* wso = plan->d_ws_off;
    const int epoch = kind == KIND_LARGE ? ++plan->large_epoch : 0;
    chains.push_back({sp.launch, sp.gated, [=](hipStream_t st) {
      if (delay) hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(WAVE), 0, st, (unsigned long long)GATE_US * 100ull);
      void* kargs[4] = {(void*)&k, nullptr, nullptr, nullptr};
      switch (kind) {   // the kernel's arguments after KArgs
        case KIND_BLOCK: break;
        case KIND_SMALL: kargs[1] = (void*)&counter; break;
        case KIND_TAIL: kargs[1] = (void*)&ta; kargs[2] = (void*)&counter; break;
        case KIND_LARGE: kargs[1] = (void*)&wsp; kargs[2] = (void*)&wso; kargs[3] = (void*)&epoch; break;
        case KIND_MARK:
          hipLaunchKernelGGL(mark_kernel, dim3(grid), dim3(256), 0, st, k, (int)CTR_STATUS_TOO_LARGE);
          return hipGetLastError();
      }
      return hipLaunchKernel(ki->fn, dim3(grid), dim3((unsigned)ki->threads), kargs, ki->smem, st);
    }});
  }

  lane_sched::Pool& books = pool->books;
  // the books: what has completed leaves the lanes, and the launches of this plan that were timed
  // and have completed give their durations
  {
    std::vector<lane_sched::EventId> retired;
    books.retire(ticket_done, nullptr, &retired);
    for (lane_sched::EventId ev : retired) pool->spare.push_back((hipEvent_t)ev);
  }
  std::vector<double> est(chains.size());
  for (size_t i = 0; i < chains.size(); ++i) {
    LaunchTiming& t = plan->timing[chains[i].launch];
    if (t.pending && hipEventQuery(t.t1) != hipErrorNotReady) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, t.t0, t.t1) == hipSuccess) t.est.update((double)ms);
      t.pending = false;
    }
    est[i] = t.est.value();
  }
  (void)hipGetLastError();   // (a query that says "not ready" is no error of this call)
  const double head_ms = lane_sched::static_guess(lane_sched::CHAIN_HEAD, 0);
  const lane_sched::Pool::Placement place = books.place(own ? head_ms : -1., est);

  // ---- head ----
  hipStream_t s = own ? pool->lanes[(size_t)place.head] : (hipStream_t)hip_stream;
  // The handle owns scratch that a call uses from start to end (frame maxima, work counters): a
  // call waits for the previous call of this handle, whichever streams the two run on.
  HIP_TRY(h, hipStreamWaitEvent(s, h->ev_done, 0));
  if (own) {
    if (h->own_dirty) {
      HIP_TRY(h, hipEventRecord(h->ev_own, h->stream));
      HIP_TRY(h, hipStreamWaitEvent(s, h->ev_own, 0));
    }
    h->own_dirty = false;
  }
  HIP_TRY(h, hipEventRecord(h->ev[0], s));
  rc = launch_frame_max(h, b->frames, b->frame_dtype, b->n_frames, frame_elems, (double*)h->fmax.ptr, s);
  if (rc) return rc;
  HIP_TRY(h, hipEventRecord(h->ev[1], s));
  {
    FrontArgs fa;
    fa.nbins = NBINS;
    fa.keep_bin = BIN_SMALL1;
    for (int bin = 0; bin < NBINS; ++bin) { fa.begin[bin] = (int)rp.bin_begin[bin]; fa.count[bin] = (int)rp.bin_count[bin]; }
    HIP_TRY(h, hipMemsetAsync(plan->d_front, 0, sizeof(int) * 2 * NBINS, s));
    // the work counters of the small-kernel launches, here rather than in their chains: a
    // fill kernel queued behind the gate would wait for a slot on a machine already flooded
    HIP_TRY(h, hipMemsetAsync(h->d_counter, 0, sizeof(int) * 8, s));
    // (base: no order, n_bin 0 -- the arguments of a bin's launch have no meaning here)
    hipLaunchKernelGGL(front_load_kernel, dim3((unsigned)((plan->n_clusters + 255) / 256)), dim3(256), 0, s, base, fa,
                       plan->d_order, ord, plan->d_front, (int)plan->n_clusters);
  }
  HIP_TRY(h, hipEventRecord(h->ev_fork, s));
  if (rp.gate) {
    hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(WAVE), 0, s, (unsigned long long)GATE_US * 100ull);
    HIP_TRY(h, hipEventRecord(h->ev_gate, s));
  }
  hipEvent_t ticket = nullptr;
  if (own) HIP_TRY(h, lane_ticket(pool, place.head, head_ms, &ticket));

  // ---- bins, the longest first ----
  // last: the ticket of this call's latest chain on every lane; gate_seen: the lane has waited
  // for ev_gate (a lane is in order: once is enough, and the head's own lane needs neither wait)
  std::vector<hipEvent_t> last((size_t)books.size(), nullptr);
  std::vector<char> gate_seen((size_t)books.size(), 0);
  for (int i : place.order) {
    const Chain& c = chains[(size_t)i];
    const int lane = place.lane[(size_t)i];
    hipStream_t st = pool->lanes[(size_t)lane];
    if (st != s && !last[(size_t)lane]) HIP_TRY(h, hipStreamWaitEvent(st, h->ev_fork, 0));
    if (c.gated && st != s && !gate_seen[(size_t)lane]) {
      HIP_TRY(h, hipStreamWaitEvent(st, h->ev_gate, 0));
      gate_seen[(size_t)lane] = 1;
    }
    LaunchTiming& t = plan->timing[c.launch];
    // (two more markers in front of and behind the kernel: 15-20 us of a call that runs alone, so
    // a launch that has a reading is timed again every TIMING_EVERY calls only)
    bool timed = !t.pending && (!t.est.has_reading || ++t.untimed >= TIMING_EVERY);
    if (timed) t.untimed = 0;
    if (timed && !t.t0) timed = hipEventCreate(&t.t0) == hipSuccess;
    if (timed && !t.t1) timed = hipEventCreate(&t.t1) == hipSuccess;
    if (timed) HIP_TRY(h, hipEventRecord(t.t0, st));   // (after the chain's waits)
    HIP_TRY(h, c.run(st));
    if (timed) {
      HIP_TRY(h, hipEventRecord(t.t1, st));
      t.pending = true;
    }
    HIP_TRY(h, lane_ticket(pool, lane, est[(size_t)i], &last[(size_t)lane]));
  }

  // ---- finish: on the lane of the longest bin chain ----
  hipStream_t fs = own ? pool->lanes[(size_t)place.finish] : s;
  for (size_t l = 0; l < last.size(); ++l)
    if (last[l] && pool->lanes[l] != fs) HIP_TRY(h, hipStreamWaitEvent(fs, last[l], 0));
  if (b->result_rows != nullptr && b->n_features > 0)
    hipLaunchKernelGGL(result_rows_kernel, dim3((unsigned)((b->n_features + 255) / 256)), dim3(256), 0, fs,
                       b->params_out, b->cost, b->feat_offset, (int)b->n_clusters, (int)b->n_features,
                       (int)p.n_params, b->result_rows);
  if (b->done_flag != nullptr)
    hipLaunchKernelGGL(done_flag_kernel, dim3(1), dim3(WAVE), 0, fs, b->done_flag, b->done_value);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipEventRecord(h->ev[2], fs));
  HIP_TRY(h, hipEventRecord(h->ev_done, fs));
  if (own) {
    HIP_TRY(h, lane_ticket(pool, place.finish, lane_sched::static_guess(lane_sched::CHAIN_FINISH, 0), &ticket));
    h->pending = true;   // joined to the handle's stream by whoever names it next (own_stream)
  }
  h->ev_valid = true;
  return CTR_OK;
}



// the exported blob: the HIP IPC handle, then the PCI bus id of the device that owns the block
// (NUL-terminated) so that an importer can identify the owner BEFORE it maps or touches anything
constexpr size_t IPC_BUSID_OFF = sizeof(hipIpcMemHandle_t);
static_assert(IPC_BUSID_OFF + 32 <= CTR_IPC_HANDLE_BYTES, "IPC handle blob size");

int ctr_ipc_alloc(ctr_handle* h, int64_t bytes, void** dev_ptr, unsigned char* handle_out) {
  if (!h || !dev_ptr || !handle_out || bytes <= 0) return CTR_ERR_INVALID;
  *dev_ptr = nullptr;
  HIP_TRY(h, hipSetDevice(h->device));
  char busid[32] = {0};
  if (hipDeviceGetPCIBusId(busid, (int)sizeof busid, h->device) != hipSuccess || busid[0] == 0) {
    (void)hipGetLastError();
    return fail(h, CTR_ERR_DEVICE, "cannot read the PCI bus id of this device (needed to export an inbox)");
  }
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)bytes) != hipSuccess) return fail(h, CTR_ERR_NOMEM, "cannot allocate the inbox");
  hipIpcMemHandle_t ih;
  hipError_t e = hipMemset(p, 0, (size_t)bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipIpcGetMemHandle(&ih, p);
  if (e != hipSuccess) { (void)hipFree(p); return fail(h, CTR_ERR_DEVICE, std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e)); }
  std::memset(handle_out, 0, CTR_IPC_HANDLE_BYTES);
  std::memcpy(handle_out, &ih, sizeof ih);
  std::memcpy(handle_out + IPC_BUSID_OFF, busid, sizeof busid - 1);
  *dev_ptr = p;
  return CTR_OK;
}

int ctr_ipc_open(ctr_handle* h, const unsigned char* handle, void** dev_ptr) {
  if (!h || !handle || !dev_ptr) return CTR_ERR_INVALID;
  *dev_ptr = nullptr;
  HIP_TRY(h, hipSetDevice(h->device));
  // Who owns the block?  A kernel of THIS device will store there, and a store that faults can
  // take the GPUs of the node down: the owner must be this device or one it has peer access to,
  // established before anything is mapped.  An owner this process cannot resolve (not visible,
  // malformed blob) counts as "no access": the caller falls back to the collective.
  char busid[32];
  std::memcpy(busid, handle + IPC_BUSID_OFF, sizeof busid);
  busid[sizeof busid - 1] = 0;
  int owner = -1;
  if (busid[0] == 0 || hipDeviceGetByPCIBusId(&owner, busid) != hipSuccess || owner < 0) {
    (void)hipGetLastError();
    return fail(h, CTR_ERR_DEVICE, "the device that owns the block is not visible to this process");
  }
  if (owner != h->device) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, h->device, owner) != hipSuccess || !can) {
      (void)hipGetLastError();
      return fail(h, CTR_ERR_DEVICE, "no peer access from this device to the device that owns the block");
    }
  }
  hipIpcMemHandle_t ih;
  std::memcpy(&ih, handle, sizeof ih);
  void* p = nullptr;
  const hipError_t e = hipIpcOpenMemHandle(&p, ih, hipIpcMemLazyEnablePeerAccess);
  if (e != hipSuccess) return fail(h, CTR_ERR_DEVICE, std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e));
  // cross-check where the runtime can tell: the mapped pointer belongs to that owner (or is
  // reported under the device that mapped it -- runtimes differ), never to a third device
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) == hipSuccess) {
    if (attr.device != owner && attr.device != h->device) {
      (void)hipIpcCloseMemHandle(p);
      return fail(h, CTR_ERR_DEVICE, "the mapped block does not belong to the device named in its handle");
    }
  } else {
    (void)hipGetLastError();
  }
  *dev_ptr = p;
  return CTR_OK;
}

int ctr_ipc_probe(ctr_handle* h, void* dst, int64_t value) {
  if (!h || !dst) return CTR_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = own_stream(h);
  hipLaunchKernelGGL(done_flag_kernel, dim3(1), dim3(WAVE), 0, s, (int64_t*)dst, value);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(s));
  return CTR_OK;
}

int ctr_ipc_read(ctr_handle* h, void* dst_host, const void* src, int64_t bytes) {
  if (!h || !dst_host || !src || bytes < 0) return CTR_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpy(dst_host, src, (size_t)bytes, hipMemcpyDeviceToHost));
  return CTR_OK;
}

int ctr_ipc_close(ctr_handle* h, void* dev_ptr) {
  if (!h || !dev_ptr) return CTR_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipIpcCloseMemHandle(dev_ptr));
  return CTR_OK;
}

int ctr_ipc_free(ctr_handle* h, void* dev_ptr) {
  if (!h || !dev_ptr) return CTR_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipFree(dev_ptr));
  return CTR_OK;
}

int ctr_find_clusters(ctr_handle* h, int32_t ndim, const double* pos, const int32_t* frame_offset,
                      int64_t n_frames, const double* separation, int32_t* label_out, int32_t* size_out) {
  if (!h || !pos || !frame_offset || !separation || !label_out || !size_out) return CTR_ERR_INVALID;
  if (ndim != 2 && ndim != 3) return fail(h, CTR_ERR_INVALID, "ndim must be 2 or 3");
  if (n_frames < 0 || n_frames > 0x7fffffffLL) return fail(h, CTR_ERR_INVALID, "bad frame count");
  if (n_frames == 0) return CTR_OK;
  const int64_t N = frame_offset[n_frames];
  if (frame_offset[0] != 0 || N < 0) return fail(h, CTR_ERR_INVALID, "frame_offset must run from 0 to the row count");
  for (int64_t f = 0; f < n_frames; ++f)
    if (frame_offset[f + 1] < frame_offset[f]) return fail(h, CTR_ERR_INVALID, "frame_offset must be non-decreasing");
  for (int a = 0; a < ndim; ++a)
    if (!(separation[a] > 0.)) return fail(h, CTR_ERR_INVALID, "separation must be positive");
  if (N == 0) return CTR_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t b_pos = sizeof(double) * (size_t)N * ndim, b_i = sizeof(int32_t) * (size_t)N;
  size_t total = 0;
  const size_t o_pos = carve(total, b_pos), o_spos = carve(total, b_pos),
               o_fo = carve(total, sizeof(int32_t) * (size_t)(n_frames + 1)), o_label = carve(total, b_i),
               o_count = carve(total, b_i), o_size = carve(total, b_i);
  if (int rc = reserve(h, h->buf, total, "cannot allocate device memory")) return rc;
  char* q = (char*)h->buf.ptr;
  double* d_pos = (double*)(q + o_pos);
  double* d_spos = (double*)(q + o_spos);
  int32_t* d_fo = (int32_t*)(q + o_fo);
  int32_t* d_label = (int32_t*)(q + o_label);
  int32_t* d_count = (int32_t*)(q + o_count);
  int32_t* d_size = (int32_t*)(q + o_size);
  hipStream_t s = own_stream(h);
  HIP_TRY(h, hipMemcpyAsync(d_pos, pos,sizeof(double) * (size_t)N * ndim, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(d_fo, frame_offset, sizeof(int32_t) * (size_t)(n_frames + 1), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)N, s));
  const double s2 = ndim == 3 ? separation[2] : 1.;
  if (ndim == 2)
    hipLaunchKernelGGL(find_clusters_kernel<2>, dim3((unsigned)n_frames), dim3(FC_THREADS), 0, s, d_pos, d_fo,
                       separation[0], separation[1], s2, d_spos, d_label, d_count, d_size);
  else
    hipLaunchKernelGGL(find_clusters_kernel<3>, dim3((unsigned)n_frames), dim3(FC_THREADS), 0, s, d_pos, d_fo,
                       separation[0], separation[1], s2, d_spos, d_label, d_count, d_size);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(label_out, d_label, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(size_out, d_size, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return CTR_OK;
}

int ctr_draw_frames_device(ctr_handle* h, const ctr_synth* sy, void* frames_out, void* hip_stream) {
  if (!h || !sy || !frames_out) return CTR_ERR_INVALID;
  if (sy->ndim != 2 && sy->ndim != 3) return fail(h, CTR_ERR_INVALID, "ndim must be 2 or 3");
  if (sy->frame_dtype != CTR_DTYPE_U8 && sy->frame_dtype != CTR_DTYPE_U16)
    return fail(h, CTR_ERR_UNSUPPORTED, "frames are drawn as uint8 or uint16 (integer wrap-around is part of the rule)");
  if (sy->n_frames < 0 || sy->n_features < 0) return fail(h, CTR_ERR_INVALID, "negative counts");
  if (!(sy->noise >= 0.)) return fail(h, CTR_ERR_INVALID, "noise must be >= 0");
  long long felems = 1;
  for (int a = 0; a < sy->ndim; ++a) {
    if (sy->shape[a] < 1) return fail(h, CTR_ERR_INVALID, "frame shape must be positive");
    felems *= sy->shape[a];
  }
  const long long total = felems * sy->n_frames;
  if (total == 0) return CTR_OK;
  if (sy->n_features > 0 && (!sy->frame_of || !sy->pos || !sy->size || !sy->max_value))
    return fail(h, CTR_ERR_INVALID, "null feature table");
  if (sy->n_features > 0x7fffffffLL) return fail(h, CTR_ERR_INVALID, "too many features for one launch");
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : own_stream(h);
  int* acc = nullptr;
  HIP_TRY(h, hipMallocAsync((void**)&acc, sizeof(int) * (size_t)total, s));
  HIP_TRY(h, hipMemsetAsync(acc, 0, sizeof(int) * (size_t)total, s));
  SynthArgs a;
  a.ndim = sy->ndim;
  for (int q = 0; q < 3; ++q) a.shape[q] = q < sy->ndim ? (long)sy->shape[q] : 1;
  a.frame_elems = (long)felems;
  a.n_features = (long)sy->n_features;
  a.frame_of = sy->frame_of;
  a.pos = sy->pos;
  a.size = sy->size;
  a.max_value = sy->max_value;
  a.acc = acc;
  if (sy->n_features > 0) {
    if (sy->ndim == 2) hipLaunchKernelGGL(draw_features_kernel<2>, dim3((unsigned)sy->n_features), dim3(SYN_THREADS), 0, s, a);
    else hipLaunchKernelGGL(draw_features_kernel<3>, dim3((unsigned)sy->n_features), dim3(SYN_THREADS), 0, s, a);
  }
  const unsigned blocks = (unsigned)((total + 255) / 256);
  if (sy->frame_dtype == CTR_DTYPE_U8)
    hipLaunchKernelGGL(finish_frames_kernel<uint8_t>, dim3(blocks), dim3(256), 0, s, acc, (uint8_t*)frames_out,
                       (long)total, sy->noise, (unsigned long long)sy->seed, 255L);
  else
    hipLaunchKernelGGL(finish_frames_kernel<uint16_t>, dim3(blocks), dim3(256), 0, s, acc, (uint16_t*)frames_out,
                       (long)total, sy->noise, (unsigned long long)sy->seed, 65535L);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipFreeAsync(acc, s));
  return CTR_OK;
}

int ctr_locate_maxima_device(ctr_handle* h, const ctr_locate* l, void* hip_stream) {
  if (!h) return CTR_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  const char* msg = "";
  const int rc = ctr_locate_launch(l, hip_stream ? (hipStream_t)hip_stream : own_stream(h), &msg);
  if (rc != CTR_OK) return fail(h, rc, std::string("ctr_locate_maxima_device: ") + msg);
  return CTR_OK;
}

int ctr_characterize_device(ctr_handle* h, const ctr_characterize* c, void* hip_stream) {
  return run_stage("ctr_characterize_device", h, nullptr, c, hip_stream, ctr_characterize_launch);
}

int ctr_preprocess_device(ctr_handle* h, const ctr_preprocess* p, void* hip_stream) {
  return run_stage("ctr_preprocess_device", h, nullptr, p, hip_stream, ctr_preprocess_launch);
}

int ctr_link_device(ctr_handle* h, const ctr_link* l, void* hip_stream) {
  return run_stage("ctr_link_device", h, &ctr_handle::link, l, hip_stream, ctr_link_launch);
}

int ctr_link_adaptive_device(ctr_handle* h, const ctr_link_adaptive* l, void* hip_stream) {
  return run_stage("ctr_link_adaptive_device", h, &ctr_handle::link, l, hip_stream, ctr_link_adaptive_launch);
}

int ctr_link_predict_device(ctr_handle* h, const ctr_link_predict* l, void* hip_stream) {
  return run_stage("ctr_link_predict_device", h, &ctr_handle::link, l, hip_stream, ctr_link_predict_launch);
}

int ctr_relocate_device(ctr_handle* h, const ctr_relocate* r, void* hip_stream) {
  return run_stage("ctr_relocate_device", h, nullptr, r, hip_stream, ctr_relocate_launch);
}

int ctr_find_link_device(ctr_handle* h, const ctr_find_link* f, void* hip_stream) {
  return run_stage("ctr_find_link_device", h, &ctr_handle::link, f, hip_stream, ctr_find_link_launch);
}

int ctr_refine_com_device(ctr_handle* h, const ctr_refine_com* c, void* hip_stream) {
  return run_stage("ctr_refine_com_device", h, nullptr, c, hip_stream, ctr_refine_com_launch);
}

int ctr_train_device(ctr_handle* h, const ctr_train* t, void* hip_stream) {
  return run_stage("ctr_train_device", h, &ctr_handle::train, t, hip_stream, ctr_train_launch);
}

int ctr_refine_global_device(ctr_handle* h, const ctr_refine_global* d, void* hip_stream) {
  return run_stage("ctr_refine_global_device", h, &ctr_handle::global, d, hip_stream, ctr_refine_global_launch);
}

int ctr_refine_global_plan(const ctr_refine_global* d, int64_t* scratch_bytes, int32_t* launches_per_iteration,
                           int32_t* tiles, int64_t* row_doubles) {
  const char* msg = "";
  ctr_global_launch_plan plan = {};
  StageRun run = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, STAGE_MAX_GRID};
  const int rc = ctr_refine_global_launch(d, &run, &msg, &plan);
  if (rc != CTR_OK) return fail(nullptr, rc, std::string("ctr_refine_global_plan: ") + msg);
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
  if (launches_per_iteration) *launches_per_iteration = plan.launches_per_iteration;
  if (tiles) *tiles = plan.tiles;
  if (row_doubles) *row_doubles = plan.row_doubles;
  return CTR_OK;
}

int ctr_cluster_tracks_device(ctr_handle* h, const ctr_cluster_tracks* c, void* hip_stream) {
  return run_stage("ctr_cluster_tracks_device", h, &ctr_handle::tracks, c, hip_stream, ctr_cluster_tracks_launch);
}

int ctr_cluster_tracks_plan(const ctr_cluster_tracks* c, int64_t* scratch_bytes, int32_t* max_rounds,
                            int32_t* jumps_per_round) {
  const char* msg = "";
  ctr_tracks_plan plan = {};
  StageRun run = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, STAGE_MAX_GRID};
  const int rc = ctr_cluster_tracks_launch(c, &run, &msg, &plan);
  if (rc != CTR_OK) return fail(nullptr, rc, std::string("ctr_cluster_tracks_plan: ") + msg);
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
  if (max_rounds) *max_rounds = plan.max_rounds;
  if (jumps_per_round) *jumps_per_round = plan.jumps_per_round;
  return CTR_OK;
}

int ctr_track_positions_device(ctr_handle* h, const ctr_track_positions* p, void* hip_stream) {
  return run_stage("ctr_track_positions_device", h, nullptr, p, hip_stream, ctr_track_positions_launch);
}

int ctr_drift_device(ctr_handle* h, const ctr_drift* d, void* hip_stream) {
  return run_stage("ctr_drift_device", h, &ctr_handle::drift, d, hip_stream, ctr_drift_launch);
}

int ctr_drift_subtract_device(ctr_handle* h, const ctr_drift_subtract* d, void* hip_stream) {
  return run_stage("ctr_drift_subtract_device", h, nullptr, d, hip_stream, ctr_drift_subtract_launch);
}

int ctr_filter_stubs_device(ctr_handle* h, const ctr_filter_stubs* d, void* hip_stream) {
  return run_stage("ctr_filter_stubs_device", h, nullptr, d, hip_stream, ctr_filter_stubs_launch);
}

int ctr_msd_device(ctr_handle* h, const ctr_msd* d, void* hip_stream) {
  return run_stage("ctr_msd_device", h, &ctr_handle::msd, d, hip_stream, ctr_msd_launch);
}

int ctr_emsd_device(ctr_handle* h, const ctr_emsd* d, void* hip_stream) {
  return run_stage("ctr_emsd_device", h, &ctr_handle::msd, d, hip_stream, ctr_emsd_launch);
}

int ctr_vanhove_device(ctr_handle* h, const ctr_vanhove* d, void* hip_stream) {
  return run_stage("ctr_vanhove_device", h, &ctr_handle::msd, d, hip_stream, ctr_vanhove_launch);
}

int ctr_pair_correlation_device(ctr_handle* h, const ctr_pair_correlation* d, void* hip_stream) {
  return run_stage("ctr_pair_correlation_device", h, &ctr_handle::pcf, d, hip_stream, ctr_pair_correlation_launch);
}

int ctr_neighbors_device(ctr_handle* h, const ctr_neighbors* d, void* hip_stream) {
  return run_stage("ctr_neighbors_device", h, &ctr_handle::nbr, d, hip_stream, ctr_neighbors_launch);
}

int ctr_twopoint_device(ctr_handle* h, const ctr_twopoint* d, void* hip_stream) {
  return run_stage("ctr_twopoint_device", h, &ctr_handle::twopt, d, hip_stream, ctr_twopoint_launch);
}

int ctr_shape_device(ctr_handle* h, const ctr_shape* s, void* hip_stream) {
  return run_stage("ctr_shape_device", h, nullptr, s, hip_stream, ctr_shape_launch);
}

int ctr_shape_dynamics_device(ctr_handle* h, const ctr_shape_dynamics* d, void* hip_stream) {
  return run_stage("ctr_shape_dynamics_device", h, &ctr_handle::shape, d, hip_stream, ctr_shape_dynamics_launch);
}

int ctr_shape_plan(const ctr_shape_dynamics* d, int32_t* tile, int32_t* halo, int64_t* lds_bytes, int64_t* n_tiles,
                   int64_t* scratch_bytes) {
  const char* msg = "";
  ctr_shape_launch_plan plan = {};
  StageRun run = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, STAGE_MAX_GRID};
  const int rc = ctr_shape_dynamics_launch(d, &run, &msg, &plan);
  if (rc != CTR_OK) return fail(nullptr, rc, std::string("ctr_shape_plan: ") + msg);
  if (tile) *tile = plan.tile;
  if (halo) *halo = plan.halo;
  if (lds_bytes) *lds_bytes = plan.lds_bytes;
  if (n_tiles) *n_tiles = plan.n_tiles;
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
  return CTR_OK;
}

int ctr_shape_histogram_device(ctr_handle* h, const ctr_shape_histogram* d, void* hip_stream) {
  return run_stage("ctr_shape_histogram_device", h, &ctr_handle::shape, d, hip_stream, ctr_shape_histogram_launch);
}

int ctr_residual_device(ctr_handle* h, const ctr_residual* r, void* hip_stream) {
  return run_stage("ctr_residual_device", h, &ctr_handle::resid, r, hip_stream, ctr_residual_launch);
}

int ctr_residual_plan(const ctr_residual* r, int32_t* tile, int32_t* chunk, int64_t* n_tiles, int64_t* grids,
                      int64_t* lds_bytes, int64_t* scratch_bytes) {
  const char* msg = "";
  ctr_residual_launch_plan plan = {};
  StageRun run = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, STAGE_MAX_GRID};
  const int rc = ctr_residual_launch(r, &run, &msg, &plan);
  if (rc != CTR_OK) return fail(nullptr, rc, std::string("ctr_residual_plan: ") + msg);
  for (int d = 0; tile && d < 3; ++d) tile[d] = plan.tile[d];
  if (chunk) *chunk = plan.chunk;
  if (n_tiles) *n_tiles = plan.n_tiles;
  for (int k = 0; grids && k < 4; ++k) grids[k] = plan.grids[k];
  if (lds_bytes) *lds_bytes = plan.lds_bytes;
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
  return CTR_OK;
}

int ctr_fit_error_device(ctr_handle* h, const ctr_fit_error* e, void* hip_stream) {
  return run_stage("ctr_fit_error_device", h, &ctr_handle::fiterr, e, hip_stream, ctr_fit_error_launch);
}

int ctr_fit_error_plan(const ctr_fit_error* e, int32_t* max_vars, int32_t* chunk, int64_t* lds_bytes, int64_t* grid,
                       int64_t* scratch_bytes) {
  const char* msg = "";
  ctr_fit_error_launch_plan plan = {};
  StageRun run = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, STAGE_MAX_GRID};
  const int rc = ctr_fit_error_launch(e, &run, &msg, &plan);
  if (rc != CTR_OK) return fail(nullptr, rc, std::string("ctr_fit_error_plan: ") + msg);
  for (int k = 0; k < CTR_FITERR_CLASSES; ++k) {
    if (max_vars) max_vars[k] = plan.max_vars[k];
    if (chunk) chunk[k] = plan.chunk[k];
    if (lds_bytes) lds_bytes[k] = plan.lds_bytes[k];
  }
  if (grid) *grid = plan.grid;
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
  return CTR_OK;
}

int ctr_contacts_device(ctr_handle* h, const ctr_contacts* d, void* hip_stream) {
  return run_stage("ctr_contacts_device", h, &ctr_handle::contacts, d, hip_stream, ctr_contacts_launch);
}

int ctr_contacts_plan(const ctr_contacts* d, int64_t* scratch_bytes, int64_t* scan_tiles, int64_t* grids) {
  const char* msg = "";
  ctr_contacts_launch_plan plan = {};
  StageRun run = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, STAGE_MAX_GRID};
  const int rc = ctr_contacts_launch(d, &run, &msg, &plan);
  if (rc != CTR_OK) return fail(nullptr, rc, std::string("ctr_contacts_plan: ") + msg);
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
  for (int k = 0; scan_tiles && k < 2; ++k) scan_tiles[k] = plan.scan_tiles[k];
  for (int k = 0; grids && k < 4; ++k) grids[k] = plan.grids[k];
  return CTR_OK;
}

int ctr_refine_prepare_device(ctr_handle* h, const ctr_refine_prepare* r, void* hip_stream) {
  // the scatter has no scratch: it is not ordered with the handle's other calls
  Scratch ctr_handle::*scratch = r && r->mode == CTR_PREPARE_SCATTER ? nullptr : &ctr_handle::prepare;
  return run_stage("ctr_refine_prepare_device", h, scratch, r, hip_stream, ctr_refine_prepare_launch);
}

int ctr_refine_prepare_plan(const ctr_refine_prepare* r, int64_t* scratch_bytes) {
  const char* msg = "";
  long long bytes = 0;
  StageRun run = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, STAGE_MAX_GRID};
  const int rc = ctr_refine_prepare_launch(r, &run, &msg, &bytes);
  if (rc != CTR_OK) return fail(nullptr, rc, std::string("ctr_refine_prepare_plan: ") + msg);
  if (scratch_bytes) *scratch_bytes = bytes;
  return CTR_OK;
}

int ctr_find_link_refine_device(ctr_handle* h, const ctr_find_link* f, const ctr_refine_com* com, void* hip_stream) {
  const FindLinkRefine d = {f, com};
  return run_stage("ctr_find_link_refine_device", h, &ctr_handle::link, &d, hip_stream, ctr_find_link_refine_launch);
}

int ctr_relocate_plan(const ctr_relocate* r, int64_t* tile_pixels, int64_t* lds_bytes) {
  const char* msg = "";
  long long tile = 0, lds = 0;
  StageRun run = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, STAGE_MAX_GRID};
  const int rc = ctr_relocate_launch(r, &run, &msg, &tile, &lds);
  if (rc != CTR_OK) return fail(nullptr, rc, std::string("ctr_relocate_plan: ") + msg);
  if (tile_pixels) *tile_pixels = tile;
  if (lds_bytes) *lds_bytes = lds;
  return CTR_OK;
}

int ctr_orientation_device(ctr_handle* h, const ctr_orientation* o, void* hip_stream) {
  return run_stage("ctr_orientation_device", h, nullptr, o, hip_stream, ctr_orientation_launch);
}

int ctr_diffusion_device(ctr_handle* h, const ctr_diffusion* d, void* hip_stream) {
  return run_stage("ctr_diffusion_device", h, &ctr_handle::motion, d, hip_stream, ctr_diffusion_launch);
}

int ctr_diffusion_ci_device(ctr_handle* h, const ctr_diffusion_ci* d, void* hip_stream) {
  // the scratch is ctr_diffusion_device's, and so is the order of the calls
  return run_stage("ctr_diffusion_ci_device", h, &ctr_handle::motion, d, hip_stream, ctr_diffusion_ci_launch);
}

int ctr_diffusion_ci_plan(const ctr_diffusion_ci* d, int32_t* rows_in_lds, int64_t* lds_bytes, int64_t* scratch_bytes,
                          int64_t* pairs_per_chunk) {
  const char* msg = "";
  ctr_ci_plan plan = {};
  StageRun run = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, STAGE_MAX_GRID};
  const int rc = ctr_diffusion_ci_launch(d, &run, &msg, &plan);
  if (rc != CTR_OK) return fail(nullptr, rc, std::string("ctr_diffusion_ci_plan: ") + msg);
  if (rows_in_lds) *rows_in_lds = plan.rows_in_lds;
  if (lds_bytes) *lds_bytes = plan.lds_bytes;
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
  if (pairs_per_chunk) *pairs_per_chunk = plan.pairs_per_chunk;
  return CTR_OK;
}

int32_t ctr_set_stage_max_grid(ctr_handle* h, int32_t max_grid) {
  if (!h || max_grid < 0 || max_grid > (int32_t)STAGE_MAX_GRID) return -1;
  const int32_t before = (int32_t)h->stage_max_grid;
  h->stage_max_grid = max_grid ? (unsigned)max_grid : STAGE_MAX_GRID;
  return before;
}

int ctr_synchronize(ctr_handle* h, void* hip_stream) {
  if (!h) return CTR_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  if (hip_stream) {
    HIP_TRY(h, hipStreamSynchronize((hipStream_t)hip_stream));
    return CTR_OK;
  }
  // the handle's own stream, and the refine call that is pending beside it
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  HIP_TRY(h, hipEventSynchronize(h->ev_done));
  h->pending = false;   // (done: there is nothing left to join)
  return CTR_OK;
}

int32_t ctr_set_lane_limit(int32_t device, int32_t n) {
  std::lock_guard<std::mutex> g(g_pool_mutex);
  const auto it = g_pools.find(device);
  if (it == g_pools.end() || !it->second) return -1;
  std::lock_guard<std::mutex> lock(it->second->mu);
  return it->second->books.set_limit(n);
}

int ctr_query_done(ctr_handle* h) {
  if (!h) return -1;
  if (hipSetDevice(h->device) != hipSuccess) return -1;
  const hipError_t e = hipEventQuery(h->ev_done);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  h->err = std::string("hipEventQuery: ") + hipGetErrorString(e);
  return -1;
}

int ctr_engine_wait_stream(ctr_handle* h, void* hip_stream) {
  if (!h) return CTR_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipEventRecord(h->ev_order, (hipStream_t)hip_stream));
  HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_order, 0));
  // The head of the next refine call on the own stream is not queued there: it waits for an event
  // recorded on the stream behind this wait and every earlier one (several calls, for several
  // streams, are all honoured).
  h->own_dirty = true;
  return CTR_OK;
}

int ctr_stream_wait_engine(ctr_handle* h, void* hip_stream) {
  if (!h) return CTR_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  // a pending refine call directly: its end is an event of a lane, not of the handle's stream
  if (h->pending) HIP_TRY(h, hipStreamWaitEvent((hipStream_t)hip_stream, h->ev_done, 0));
  HIP_TRY(h, hipEventRecord(h->ev_order, own_stream(h)));
  HIP_TRY(h, hipStreamWaitEvent((hipStream_t)hip_stream, h->ev_order, 0));
  return CTR_OK;
}

int ctr_last_kernel_ms(ctr_handle* h, double* frame_max_ms, double* refine_ms) {
  if (!h) return CTR_ERR_INVALID;
  if (!h->ev_valid) return fail(h, CTR_ERR_INVALID, "no ctr_refine_batch_device call to time");
  HIP_TRY(h, hipEventSynchronize(h->ev[2]));
  float a = 0.f, c = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
  HIP_TRY(h, hipEventElapsedTime(&c, h->ev[1], h->ev[2]));
  if (frame_max_ms) *frame_max_ms = a;
  if (refine_ms) *refine_ms = c;
  return CTR_OK;
}

int ctr_refine_batch(ctr_handle* h, const ctr_problem* p, const ctr_batch* b) {
  if (!h || !p || !b) return CTR_ERR_INVALID;
  std::string msg;
  int rc = validate(p, msg);
  if (rc) return fail(h, rc, msg);
  const size_t isz = host_dtype_size(b->frame_dtype);
  if (!isz) return fail(h, CTR_ERR_INVALID, "unknown frame dtype");
  if (b->n_clusters < 0 || b->n_features < 0 || b->n_frames < 0) return fail(h, CTR_ERR_INVALID, "negative counts");
  if (b->n_clusters == 0) return CTR_OK;
  if (!b->frames || !b->frame_index || !b->feat_offset || !b->params || !b->low || !b->high ||
      !b->params_out || !b->cost || !b->status || !b->n_rounds || !b->n_iter)
    return fail(h, CTR_ERR_INVALID, "null buffer in batch");
  int64_t frame_elems = 1;
  for (int a = 0; a < p->ndim; ++a) {
    if (b->shape[a] < 1) return fail(h, CTR_ERR_INVALID, "frame shape must be positive");
    frame_elems *= b->shape[a];
  }
  const int64_t C = b->n_clusters, N = b->n_features;
  if (b->feat_offset[0] != 0 || b->feat_offset[C] != N) return fail(h, CTR_ERR_INVALID, "feat_offset must run from 0 to n_features");
  for (int64_t c = 0; c < C; ++c) {
    if (b->feat_offset[c + 1] < b->feat_offset[c]) return fail(h, CTR_ERR_INVALID, "feat_offset must be non-decreasing");
    if (b->frame_index[c] < 0 || b->frame_index[c] >= b->n_frames) return fail(h, CTR_ERR_INVALID, "frame_index out of range");
  }
  HIP_TRY(h, hipSetDevice(h->device));

  const size_t np = (size_t)p->n_params;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t sz_frames = al((size_t)b->n_frames * (size_t)frame_elems * isz);
  const size_t sz_fi = al(sizeof(int32_t) * (size_t)C), sz_fo = al(sizeof(int32_t) * (size_t)(C + 1));
  const size_t sz_par = al(sizeof(double) * (size_t)N * np);
  const size_t sz_c = al(sizeof(double) * (size_t)C), sz_ci = al(sizeof(int32_t) * (size_t)C);
  const size_t total = sz_frames + sz_fi + sz_fo + (b->params_std ? 5 : 4) * sz_par + sz_c + 3 * sz_ci;
  rc = reserve(h, h->buf, total, "cannot allocate device memory for the batch");
  if (rc) return rc;
  char* q = (char*)h->buf.ptr;
  ctr_batch d = *b;
  auto take = [&](size_t n) { char* r = q; q += n; return r; };
  char* d_frames = take(sz_frames);
  int32_t* d_fi = (int32_t*)take(sz_fi);
  int32_t* d_fo = (int32_t*)take(sz_fo);
  double* d_par = (double*)take(sz_par);
  double* d_low = (double*)take(sz_par);
  double* d_high = (double*)take(sz_par);
  double* d_out = (double*)take(sz_par);
  double* d_cost = (double*)take(sz_c);
  int32_t* d_status = (int32_t*)take(sz_ci);
  int32_t* d_rounds = (int32_t*)take(sz_ci);
  int32_t* d_iter = (int32_t*)take(sz_ci);
  double* d_std = b->params_std ? (double*)take(sz_par) : nullptr;
  hipStream_t s = own_stream(h);
  HIP_TRY(h, hipMemcpyAsync(d_frames, b->frames, (size_t)b->n_frames * (size_t)frame_elems * isz, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(d_fi, b->frame_index, sizeof(int32_t) * (size_t)C, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(d_fo, b->feat_offset, sizeof(int32_t) * (size_t)(C + 1), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(d_par, b->params, sizeof(double) * (size_t)N * np, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(d_low, b->low, sizeof(double) * (size_t)N * np, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(d_high, b->high, sizeof(double) * (size_t)N * np, hipMemcpyHostToDevice, s));
  d.frames = d_frames; d.frame_index = d_fi; d.feat_offset = d_fo;
  d.params = d_par; d.low = d_low; d.high = d_high; d.params_out = d_out;
  d.cost = d_cost; d.status = d_status; d.n_rounds = d_rounds; d.n_iter = d_iter;
  d.params_std = d_std;
  d.result_rows = nullptr;   // (the host-buffer call returns the tables themselves)
  d.done_flag = nullptr;
  ctr_plan* plan = nullptr;
  rc = ctr_plan_create(h, p, C, b->feat_offset, &plan);
  if (rc) return rc;
  rc = ctr_refine_batch_device(h, plan, &d, s);
  if (rc == CTR_OK) {
    hipError_t e = hipMemcpyAsync(b->params_out, d_out, sizeof(double) * (size_t)N * np, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(b->cost, d_cost, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(b->status, d_status, sizeof(int32_t) * (size_t)C, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(b->n_rounds, d_rounds, sizeof(int32_t) * (size_t)C, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(b->n_iter, d_iter, sizeof(int32_t) * (size_t)C, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && d_std) e = hipMemcpyAsync(b->params_std, d_std, sizeof(double) * (size_t)N * np, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(h, CTR_ERR_DEVICE, std::string("copy back / kernel execution: ") + hipGetErrorString(e));
  } else {
    (void)hipStreamSynchronize(s);
  }
  ctr_plan_destroy(plan);
  return rc;
}

}  // extern "C"
