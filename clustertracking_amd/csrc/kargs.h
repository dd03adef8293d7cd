// kargs.h -- what the translation units of the engine share: kernel arguments and the
// functions through which ctrefine.hip (host runtime) gets at the kernels compiled elsewhere.
// The engine is split into several .hip files only so that they compile in parallel.
// Which launches of a call get which KArgs::split* and TailArgs values is decided on the host, in
// refine_plan.h (LaunchSpec); the sizes both sides share are in engine_dims.h.
#ifndef CTREFINE_KARGS_H
#define CTREFINE_KARGS_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ctrefine.h"
#include "engine_dims.h"

struct KArgs {
  ctr_problem prob;
  const void* frames;
  int32_t frame_dtype;
  int32_t n_bin;
  int64_t shape[3];
  int64_t frame_elems;
  const int32_t* frame_index;
  const int32_t* feat_offset;
  const double* params;
  const double* low;
  const double* high;
  double* params_out;
  double* cost;
  int32_t* status;
  int32_t* n_rounds;
  int32_t* n_iter;
  double* params_std;    // [N, n_params] or nullptr (ctr_batch.params_std)
  const double* fmax;
  const int32_t* order;  // cluster ids of this bin
  // part of the bin a launch takes.  split == nullptr: all of it.  Else, with skip =
  // min(*split, split_cap), the entries that refine_tail_kernel fits: split_cap is 0 without a
  // tail launch and INT32_MAX with one, which takes every close cluster (skip = *split):
  // small kernel, split_part 1: entries [skip, *split) (the likely slow fits, front_load_kernel's
  // count; queued without a tail launch only), split_part 2: entries [*split, n_bin), split_part 3:
  // entries [skip, n_bin) (beside a tail launch, one tier of more pairs than that launch takes whole);
  // block kernel: entries [skip, n_bin)
  const int32_t* split;
  int32_t split_part;
  int32_t split_cap;
  // lowpass of the window (ctr_problem.noise_size): taps of axis a at lp_w[a * LP_STRIDE + 0 ..
  // 2 * lp_half[a]], normalised; an unfiltered axis has lp_half 0 and the single tap 1.
  // nullptr = no lowpass.  Only the LP instantiations of the block kernel read them.
  int32_t lp_half[3];
  const double* lp_w;
  // large-cluster kernel: squared relative residual (preconditioned norm) at which its conjugate
  // gradients stop, far from / near the minimum (large_kernel.h)
  double cg_tol2_far, cg_tol2_near;
};

constexpr int LP_STRIDE = 40;   // >= 2 * 16 + 1 taps (CTR_MAX_NOISE_SIZE = 4)

// refine_tail_kernel (tail_kernel.h): the likely slow clusters of three bins of a call in one
// launch, and all of a bin that is small.  Segment s -- 0: the pairs, 1 / 2: the block bins
// NT = 1 / 2 -- has the workgroups from grid_begin[s] up to the next segment's in the grid, which
// holds the segments in the order 1, 2, 0 (the block clusters, the slowest of a call, are not
// dispatched behind the workgroups of the pairs); grid_begin[TAIL_SEGMENTS] is the grid.  Its
// workgroups share the entries order[ord_off[s] + 0 .. range): range = whole[s] where that is
// positive (the bin's count: the tail launch fits the whole bin), else *close[s], the clusters
// that front_load_kernel has put first and counted.  An empty segment has no workgroup and a null
// count.  (TAIL_SEGMENTS: engine_dims.h)
struct TailArgs {
  const int32_t* close[TAIL_SEGMENTS];
  int32_t ord_off[TAIL_SEGMENTS];
  int32_t grid_begin[TAIL_SEGMENTS + 1];
  int32_t whole[TAIL_SEGMENTS];
};

// a kernel of another translation unit: host-side handle for hipLaunchKernel /
// hipFuncSetAttribute, dynamic LDS bytes and workgroup size
struct KernelInfo {
  const void* fn;
  size_t smem;
  int threads;
};

// ---- workspace of one large cluster (large_kernel.h), in doubles ---------------------------
constexpr int LARGE_MAXNB = 48;   // neighbours (features with overlapping mask ellipsoids) per feature
constexpr int LARGE_AGG = 4;      // features per aggregate of the preconditioner
constexpr int LARGE_AGG_TRI = 416;      // >= (4 * 7) (4 * 7 + 1) / 2 = 406 packed entries of the factor
constexpr int LARGE_AGG_STRIDE = 1280;  // ... + (4 * 7)^2 = 784 of the explicit inverse behind it

struct LargeWs {
  long long nvp, nvp_i;   // variables / features rounded up to a multiple of 8
  long long o_vec, o_cur, o_mco, o_fpar, o_pre, o_uq, o_tile, o_off, o_offc, o_int, o_sync, o_pre2, o_agg, o_pix, o_pixv, cap, total;
};

// n features, npf per-feature and ns shared variables
// cap: pixels of a mask's bounding box, prod(2 radius + 1): room for a feature's list of mask pixels
__host__ __device__ inline LargeWs large_ws(int n, int npf, int ns, long long cap) {
  LargeWs W;
  const long long nn = n, nv = ns + nn * npf;
  W.nvp = (nv + 7) & ~7LL;
  W.nvp_i = (nn + 7) & ~7LL;
  long long o = 0;
  W.o_vec = o;  o += 14 * W.nvp;                 // v vt v0 lo hi g x r z p Ap dl Dm free
  W.o_cur = o;  o += W.nvp_i * CTR_MAX_PARAMS;   // parameter rows
  W.o_mco = o;  o += W.nvp_i * 3 + 8;            // mask centres
  W.o_fpar = o; o += W.nvp_i * 14;               // derived per-feature constants (FP)
  W.o_pre = o;  o += W.nvp_i * 32;               // factors of the diagonal blocks
  W.o_uq = o;   o += W.nvp_i * 16;               // second-order entries + raw sums
  W.o_tile = o; o += 2 * nn * 256;               // accepted / trial 16 x 16 tiles
  W.o_off = o;  o += 2 * nn * LARGE_MAXNB * 64;  // accepted / trial neighbour blocks
  W.o_offc = o; o += nn * LARGE_MAXNB * npf * npf;  // accepted blocks, packed (the CG's copy)
  W.o_int = o;  o += (W.nvp_i + 2 * nn * LARGE_MAXNB + 1) / 2 + 8;   // nbcnt, nbidx, rev (int32)
  // preconditioner aggregates (large_kernel.h): factors of up to n / 2 aggregates of <= 4 features
  // (LARGE_AGG_STRIDE doubles each), and their tables (int32: agg_of[n], parent[n], size[n],
  // members[4 (n / 2 + 1)], n_multi)
  W.o_pre2 = o; o += (nn / 2 + 1) * LARGE_AGG_STRIDE;
  W.o_agg = o;  o += (3 * W.nvp_i + 4 * (nn / 2 + 1) + 8 + 16 * (nn / 2 + 1) + 1) / 2 + 8;   // (+ [n_multi][4][4] neighbour slots)
  // the mask pixels of every feature, compacted (int32: box coordinates, 10 bits per axis), rebuilt
  // every re-window round: [n] counts, then n lists of `cap` entries; their values as doubles
  W.cap = (cap + 63) & ~63LL;
  W.o_pixv = o; o += nn * W.cap;
  // ... and, per feature, the pixels it shares with each neighbour (a pool of 2 `cap` entries of
  // two int32 -- position in the feature's list, packed coordinates -- per feature,
  // [n][LARGE_MAXNB] offsets and counts; a pair that does not fit: count -1)
  W.o_pix = o;  o += (W.nvp_i + 5 * nn * W.cap + 2 * nn * LARGE_MAXNB + 1) / 2 + 8;
  o = (o + 15) & ~15LL;
  W.o_sync = o; o += 64;                         // leader / helper words (large_kernel.h: LSY_*), zero at plan creation
  W.total = (o + 31) & ~31LL;
  return W;
}

// refine_large_kernel<ND, ISO>(KArgs, double* ws, const long long* ws_off_of_cluster, int epoch):
// grid = n_bin leaders + n_bin * (G - 1) helpers (large_kernel.h)
// refine_block_kernel<ND, ISO, NT, W, CONS, LP, FIT> of one cell of a block family
// (CTR_KFAM_*; block_table.h): nt = 1..8; cons != 0: the instantiation for clusters with equality
// constraints (nt = 1, 2 only).  {nullptr} for a cell the unit does not hold.
KernelInfo ctr_block_kernel_2d(int family, int ndim, int iso, int nt, int cons);     // GAUSS, GAUSS_TP; 2D
KernelInfo ctr_block_kernel_3d(int family, int ndim, int iso, int nt, int cons);     // GAUSS; 3D
KernelInfo ctr_block_kernel_lp(int family, int ndim, int iso, int nt, int cons);     // LOWPASS (LP = true)
KernelInfo ctr_block_kernel_fit2d(int family, int ndim, int iso, int nt, int cons);  // RING, DISC; 2D
KernelInfo ctr_block_kernel_fit3d(int family, int ndim, int iso, int nt, int cons);  // RING, DISC; 3D
KernelInfo ctr_block_kernel_inv(int family, int ndim, int iso, int nt, int cons);    // INV_SERIES
// refine_small_kernel<ND, NF, ISO, SG>(KArgs, int* counter); nullptr if not instantiated
const void* ctr_small_kernel(int ndim, int nf, int iso, int sg);
// refine_tail_kernel<ND, ISO>(KArgs, TailArgs, int* counter); 2D only, {nullptr} otherwise
KernelInfo ctr_tail_kernel(int ndim, int iso);
KernelInfo ctr_large_kernel(int ndim, int iso, int lp);   // lp: with the lowpass of the window
// feature location (tu_locate.hip, locate_kernels.h): checks the descriptor and queues the whole
// pipeline on `s`.  CTR_OK or an error code with a static message in *msg.
int ctr_locate_launch(const ctr_locate* l, hipStream_t s, const char** msg);
// The stage units (tu_characterize, tu_preprocess, tu_link, tu_motion, tu_motion_ci, tu_relocate, tu_findlink,
// tu_refine_com, tu_train, tu_cluster_tracks, tu_refine_prepare, tu_drift, tu_msd, tu_pair_corr,
// tu_neighbors, tu_twopoint, tu_shape, tu_residual, tu_contacts, tu_fit_error)
// share one launch signature: ctr_<stage>_launch(descriptor, StageRun*, &msg, extras...).  Each
// checks its descriptor, writes the scratch it needs into stage->scratch_bytes and, for
// STAGE_LAUNCH, queues its whole pipeline on stage->stream.  CTR_OK or an error code with a static
// message in *msg.  Their callers are run_stage (ctrefine.hip), for every ctr_<stage>_device, and
// the two ctr_*_plan queries.  The device and host primitives they share are in stage_common.h.
enum StageMode {
  STAGE_CHECK_SCALARS,   // the scalars alone, no pointer is looked at (ctr_*_plan); a stage whose
                         // launch decision needs no such form checks everything
  STAGE_CHECK,           // the whole descriptor
  STAGE_LAUNCH,          // ... and queue the kernels
};
struct StageRun {
  StageMode mode;
  hipStream_t stream;    // STAGE_LAUNCH
  void* scratch;         // STAGE_LAUNCH: a block of scratch_bytes, for a stage that asked for any
  size_t scratch_bytes;  // out; the caller starts it at 0, a stage without scratch leaves it; 0 from a
                         // stage with scratch: nothing to launch
  unsigned max_grid;     // most workgroups of a grid-stride launch (stage_common.h: stride_grid, frame_grid):
                         // the handle's cap, STAGE_MAX_GRID where there is no handle; never 0
};
int ctr_characterize_launch(const ctr_characterize* c, StageRun* stage, const char** msg);   // characterize_kernels.h
int ctr_preprocess_launch(const ctr_preprocess* p, StageRun* stage, const char** msg);       // preprocess_kernels.h
int ctr_link_launch(const ctr_link* l, StageRun* stage, const char** msg);                   // link_kernels.h; scratch
int ctr_link_adaptive_launch(const ctr_link_adaptive* l, StageRun* stage, const char** msg);   // ... with the adaptive search range
int ctr_link_predict_launch(const ctr_link_predict* l, StageRun* stage, const char** msg);     // ... with prediction (link_predict_kernels.h)
int ctr_orientation_launch(const ctr_orientation* o, StageRun* stage, const char** msg);     // motion_kernels.h
int ctr_diffusion_launch(const ctr_diffusion* d, StageRun* stage, const char** msg);         // ... scratch: its partial sums
// bootstrap interval of the diffusion tensor (motion_ci_kernels.h; scratch): the launch decision
// goes to *plan (may be null), scratch_bytes there without the alignment slack of stage->scratch_bytes
struct ctr_ci_plan {
  int rows_in_lds;
  long long lds_bytes, scratch_bytes, pairs_per_chunk;
};
int ctr_diffusion_ci_launch(const ctr_diffusion_ci* d, StageRun* stage, const char** msg, ctr_ci_plan* plan);
// relocation candidates (relocate_kernels.h): the plan goes to *tile_pixels, *lds_bytes (may be null)
int ctr_relocate_launch(const ctr_relocate* r, StageRun* stage, const char** msg, long long* tile_pixels,
                        long long* lds_bytes);
// find and link with relocation (findlink_kernels.h; scratch): queues ctr_relocate_launch per level
int ctr_find_link_launch(const ctr_find_link* f, StageRun* stage, const char** msg);
// centre-of-mass refinement (refine_com_kernels.h).  level (may be null): instead of the
// descriptor's table, the rows [*start, *start + *cnt) of a level of ctr_find_link_launch's table,
// counted on the device (at most max_rows), all of frame `frame`, refined in place: pos and mass,
// and spos = pos / sr
struct RefineComLevel {
  const long long* start;
  const int* cnt;
  long long max_rows;
  int frame;
  double* pos;
  double* mass;
  double* spos;
  double sr[3];
};
int ctr_refine_com_launch(const ctr_refine_com* c, StageRun* stage, const char** msg, const RefineComLevel* level);
// ctr_find_link_refine_device: ctr_find_link_launch's loop with ctr_refine_com_launch per level
struct FindLinkRefine {
  const ctr_find_link* f;
  const ctr_refine_com* com;
};
int ctr_find_link_refine_launch(const FindLinkRefine* d, StageRun* stage, const char** msg);
// training of shared fit parameters (train_kernels.h; scratch: frame maxima, partials, solver state)
int ctr_train_launch(const ctr_train* t, StageRun* stage, const char** msg);
// shared and per-feature parameters in one problem (global_kernels.h; scratch: frame maxima, a row per
// cluster, the Schur and evaluation tables, solver state, mask centres): the launch decision goes
// to *plan (may be null)
struct ctr_global_launch_plan {
  long long scratch_bytes, row_doubles;
  int launches_per_iteration, tiles;
};
int ctr_refine_global_launch(const ctr_refine_global* t, StageRun* stage, const char** msg, ctr_global_launch_plan* plan);
// cluster tracks (cluster_track_kernels.h; scratch: labels, member counts, the words of the rounds):
// the round bound goes to *plan (may be null)
struct ctr_tracks_plan {
  long long scratch_bytes;
  int max_rounds, jumps_per_round;
};
int ctr_cluster_tracks_launch(const ctr_cluster_tracks* c, StageRun* stage, const char** msg, ctr_tracks_plan* plan);
int ctr_track_positions_launch(const ctr_track_positions* p, StageRun* stage, const char** msg);
// a refine batch from device tables and the scatter of its results (refine_prepare_kernels.h; scratch:
// scaled positions, member counts, ranks, clusters per frame): the scratch goes to *scratch_bytes
// (may be null) without the need of a device
int ctr_refine_prepare_launch(const ctr_refine_prepare* r, StageRun* stage, const char** msg, long long* scratch_bytes);
// drift of a linked video (drift_kernels.h; scratch of the first: the step of every frame)
int ctr_drift_launch(const ctr_drift* d, StageRun* stage, const char** msg);
int ctr_drift_subtract_launch(const ctr_drift_subtract* d, StageRun* stage, const char** msg);
int ctr_filter_stubs_launch(const ctr_filter_stubs* d, StageRun* stage, const char** msg);
// mean squared displacement of linked particles (msd_kernels.h; scratch: the sorted rows, the row
// range of every id and, for the ensemble, a partial per chunk of ids)
int ctr_msd_launch(const ctr_msd* d, StageRun* stage, const char** msg);
int ctr_emsd_launch(const ctr_emsd* d, StageRun* stage, const char** msg);
// van Hove displacement distributions (vanhove_kernels.h, in tu_msd; scratch: the sorted rows as above
// and a partial of the three moments per chunk of ids and lag)
int ctr_vanhove_launch(const ctr_vanhove* d, StageRun* stage, const char** msg);
// pair correlation function of a feature table (pair_corr_kernels.h; scratch: the first work item of
// every frame and, for the arc correction, a partial weight per work item)
int ctr_pair_correlation_launch(const ctr_pair_correlation* d, StageRun* stage, const char** msg);
// nearest neighbours and proximity of a feature table (neighbors_kernels.h; scratch: the first work item
// of every frame and a key per particle)
int ctr_neighbors_launch(const ctr_neighbors* d, StageRun* stage, const char** msg);
// two-point displacement correlations of linked particles (twopoint_kernels.h; scratch: the first work
// item of every frame and the partner's row of every row and lag)
int ctr_twopoint_launch(const ctr_twopoint* d, StageRun* stage, const char** msg);
// shape coordinates of tracked clusters (shape_kernels.h; scratch of the last two: the coordinates of
// every frame, coordinate-major, and for the dynamics the sums per (track, tile, lag, coordinate) and per track):
// the launch decision of the dynamics goes to *plan (may be null)
struct ctr_shape_launch_plan {
  int tile, halo;
  long long lds_bytes, n_tiles, scratch_bytes;
};
int ctr_shape_launch(const ctr_shape* o, StageRun* stage, const char** msg);
int ctr_shape_dynamics_launch(const ctr_shape_dynamics* d, StageRun* stage, const char** msg, ctr_shape_launch_plan* plan);
int ctr_shape_histogram_launch(const ctr_shape_histogram* d, StageRun* stage, const char** msg);
// model and residual frames of a fitted table (residual_kernels.h; scratch: the residual and owner of
// every pixel where the caller does not take them, the frame maxima for the per-cluster cost): the
// launch decision goes to *plan (may be null)
struct ctr_residual_launch_plan {
  int tile[3], chunk;
  long long n_tiles, grids[4], lds_bytes, scratch_bytes;
};
int ctr_residual_launch(const ctr_residual* r, StageRun* stage, const char** msg, ctr_residual_launch_plan* plan);
// contact episodes and bond lifetimes of linked particles (contacts_kernels.h; scratch: the first work
// item of every frame, the sums of the scan tiles, the difference array of `active`, and per entry of
// max_entries the chains, their episodes and the pairs): the launch decision goes to *plan (may be null)
struct ctr_contacts_launch_plan {
  long long scratch_bytes, scan_tiles[2], grids[4];
};
int ctr_contacts_launch(const ctr_contacts* d, StageRun* stage, const char** msg, ctr_contacts_launch_plan* plan);
// standard errors and covariance of a fitted table (fit_error_kernels.h; scratch: the word that says
// whether the tables were taken, the frame maxima): the launch decision goes to *plan (may be null)
struct ctr_fit_error_launch_plan {
  int max_vars[CTR_FITERR_CLASSES], chunk[CTR_FITERR_CLASSES];
  long long lds_bytes[CTR_FITERR_CLASSES], grid, scratch_bytes;
};
int ctr_fit_error_launch(const ctr_fit_error* e, StageRun* stage, const char** msg, ctr_fit_error_launch_plan* plan);

#endif  // CTREFINE_KARGS_H
