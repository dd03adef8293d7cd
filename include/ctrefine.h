/* ctrefine.h -- C-ABI of the MI355X cluster-refinement engine.
 *
 * One batched call replaces the per-cluster Python loop of the reference
 * (clustertracking/refine.py:343-430): for every (frame, cluster) group it
 * cuts the pixel window (masks.py:30-68), builds the per-feature elliptical
 * masks (refine.py:28-58), and minimises the sum-of-Gaussians least-squares
 * objective (fitfunc.py:421-489) under the box bounds (fitfunc.py:535-558) and
 * optional dimer/trimer/tetramer equality constraints (constraints.py:59-137),
 * including the re-window rounds (refine.py:365-388) and the failure rules
 * (refine.py:33-34,356-357,376-377,391-394,408-418).
 *
 * The reference has no FFI of its own: these entry points are
 * what a ctypes binding in its refine.py would call between the host-side
 * setup (refine.py:242-341) and the DataFrame write-back (refine.py:419-430).
 * INTEGRATION.md shows that binding.
 *
 * Plain C types only; every buffer is caller-owned; calls are synchronous
 * unless stated; per-cluster failures are DATA (status + NaN cost), never an
 * error return (mirrors refine.py:408-418).
 */
#ifndef CTREFINE_H
#define CTREFINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTR_ABI_VERSION 8
#define CTR_MAX_NDIM 3
#define CTR_MAX_PARAMS 12 /* background, signal, <=3 positions, <=3 sizes, profile parameters (ring, disc: 1;
                              inv_series_<N>: N + 1, as many as fit: N <= 6 in 2D isotropic, <= 3 in 3D anisotropic) */
#define CTR_MAX_VARS 127 /* optimiser variables per cluster of the on-chip kernels; larger clusters
                            (or more than 64 features) take the large-cluster path: normal matrix
                            block-sparse in HBM, no limit on features or variables */
#define CTR_MAX_NEIGHBOURS 48
#define CTR_MAX_NOISE_SIZE 4.0   /* lowpass sigma: at most 2 * 16 + 1 taps per axis */ /* large-cluster path: features whose mask ellipsoids overlap one feature's */

/* error codes (return values) */
enum {
  CTR_OK = 0,
  CTR_ERR_INVALID = 1,     /* malformed descriptor (reference: ValueError / AssertionError, refine.py:256-262,283) */
  CTR_ERR_UNSUPPORTED = 2, /* recognised but not implemented (mode 'global', a lowpass with a profile other than gauss) */
  CTR_ERR_DEVICE = 3,      /* HIP runtime failure, no MI355X visible, ... */
  CTR_ERR_NOMEM = 4
};

/* pixel types of the frame block */
enum {
  CTR_DTYPE_U8 = 0,
  CTR_DTYPE_U16 = 1,
  CTR_DTYPE_I16 = 2,
  CTR_DTYPE_I32 = 3,
  CTR_DTYPE_F32 = 4,
  CTR_DTYPE_F64 = 5
};

/* radial profile (fitfunc.py:112-154,195-204,334-343): GAUSS, RING ('thickness' column), DISC
 * ('disc_size' column) and INV_SERIES: 'inv_series_<N>' = signal_mult / (r2^N + param_a r2^(N-1) + ... +
 * param_<N>) (what fitfunc.py:148-154 evaluates: np.polyval with the leading coefficient set to 1),
 * N + 1 columns 'signal_mult', 'param_a', ...; N = n_params - (2 + ndim + sizes) - 1 */
enum { CTR_FIT_GAUSS = 0, CTR_FIT_RING = 1, CTR_FIT_DISC = 2, CTR_FIT_INV_SERIES = 3 };

/* parameter modes (fitfunc.py:9-11); 2 ('global') is rejected: it couples all
 * clusters into one problem (refine.py:319-332) and does not shard */
enum { CTR_MODE_CONST = 0, CTR_MODE_VAR = 1, CTR_MODE_GLOBAL = 2, CTR_MODE_CLUSTER = 3 };

/* equality constraints (constraints.py:59-137); applied only to clusters of
 * exactly 2 / 3 / 4 features (constraints.py:32-34) */
enum { CTR_CONS_NONE = 0, CTR_CONS_DIMER = 1, CTR_CONS_TRIMER = 2, CTR_CONS_TETRAMER = 3 };

/* ctr_problem.flags.  The first two are scheduling only: the results do not depend on them.
 * CTR_FLAG_THROUGHPUT: the caller keeps several batches in flight on one device (one handle
 * each); favour machine time per cluster over the latency of one batch -- pairs that are not
 * likely to be slow fits share a wavefront four at a time, larger 2D clusters run on the
 * fewest wavefronts.
 * CTR_FLAG_ISOLATE_TAIL: accepted, without effect.  It used to give the kernel of the likely slow
 * fits a stream of its own; the lanes (below) keep a long kernel out of the way of the others by
 * its measured duration, whichever bin holds it.
 *
 * Lanes.  The kernels of ctr_refine_batch_device calls are queued on streams of the library, the
 * lanes: one per hardware queue of the process, shared by every handle of a device (made with its
 * first handle, released with its last).  Their number is at most the integer in the environment
 * variable GPU_MAX_HW_QUEUES (the HIP runtime's own: hardware queues per process) within 1..32, or
 * 4, HIP's default, where it is not set: the first ctr_create on a device keeps the streams
 * that prove, in a trial with an empty kernel that waits (about 40 ms at 4 queues, 260 ms at 20),
 * to be on queues of their own.  How many it found is what ctr_set_lane_limit with n = 0 returns:
 * fewer than the queue count means a missed queue and a lower rate, never other results.  The library
 * reads the variable once, when it makes the lanes of a device, and never sets it; it decides
 * where a kernel is queued, never what it computes.  Every
 * launch of a call goes, longest first by the duration measured in an earlier call of its plan, to
 * the lane with the least work pending.  A call on the handle's own stream
 * (hip_stream = NULL) is queued on the lanes alone; the stream itself is joined with the call when
 * it is next named: by a *_device call on it, ctr_synchronize, ctr_stream_wait_engine.
 * CTR_FLAG_WINDOW_FILTER (NOT a scheduling flag): `noise_size` was given (refine.py:37 `if
 *   noise_size is not None`): the window goes through the reference's lowpass even where every
 *   sigma is 0 -- then that is its threshold alone, values <= threshold become 0
 *   (preprocessing.py:41-49).  Implied by any noise_size > 0. */
enum { CTR_FLAG_THROUGHPUT = 1, CTR_FLAG_ISOLATE_TAIL = 2, CTR_FLAG_WINDOW_FILTER = 4 };

/* per-cluster status */
enum {
  CTR_STATUS_OK = 0,
  CTR_STATUS_OUT_OF_BOUNDS = 1, /* no coordinate inside the frame (refine.py:33-34) or empty mask */
  CTR_STATUS_NONFINITE = 2,     /* non-finite initial parameters (refine.py:356-357) */
  CTR_STATUS_NO_CONVERGENCE = 3,/* solver failed / iteration limit (refine.py:376-377).  An empty bound
                                   interval on a variable (low > high; the reference's SciPy call raises
                                   on such a box) is this status, with n_rounds 1 and n_iter 0; bounds of
                                   constant columns are not read */
  CTR_STATUS_RMS_DEV = 4,       /* rms deviation above max_rms_dev (refine.py:391-394) */
  CTR_STATUS_TOO_LARGE = 5      /* beyond the engine: a cluster of the large-cluster path in which a feature
                                   has more than CTR_MAX_NEIGHBOURS overlapping neighbours, or whose
                                   parameter modes leave no per-feature variable (reported as data) */
};

/* What is fitted and how (one per call). */
typedef struct ctr_problem {
  int32_t ndim;                    /* 2 or 3 */
  int32_t isotropic;               /* 1: one 'size' column; 0: one per axis */
  int32_t fit_function;            /* CTR_FIT_* */
  int32_t n_params;                /* 2 + ndim + (isotropic ? 1 : ndim) + extras; column order
                                      [background, signal, (z,) y, x, size | size_(z,)y,x, extra]
                                      (fitfunc.py:353-354); extras: 0 for gauss, 1 for ring
                                      ('thickness') and disc ('disc_size'), N + 1 for inv_series_<N> */
  int32_t modes[CTR_MAX_PARAMS];   /* CTR_MODE_* per column (fitfunc.py:394) */
  int32_t radius[CTR_MAX_NDIM];    /* mask radius per axis = diameter // 2 (refine.py:286) */
  int32_t constraint_kind;         /* CTR_CONS_* */
  int32_t max_iter;                /* re-window rounds, >= 1 (refine.py:365; default 10) */
  int32_t solver_maxiter;          /* solver iterations per round (refine.py:243; default 100) */
  int32_t flags;                   /* CTR_FLAG_*; 0 = defaults */
  double constraint_dist[CTR_MAX_NDIM]; /* per-axis distance of the constraint */
  double max_shift;                /* refine.py:384 (default 1) */
  double max_rms_dev;              /* refine.py:391 (default 1) */
  double residual_factor;          /* refine.py:354,379 (default 1e5) */
  double xtol;                     /* relative step tolerance; <= 0 -> 1e-9 */
  double ftol;                     /* relative model-decrease tolerance; <= 0 -> 1e-14 */
  double threshold;                /* lowpass: filtered values <= threshold become 0
                                      (refine.py:38-40, preprocessing.py:47; default 0) */
  double noise_size[CTR_MAX_NDIM]; /* refine.py:37-40: the window of every re-window round is
                                      correlated, axis by axis, with a normalised Gaussian of this
                                      sigma truncated at 4 sigma (preprocessing.py:12-49), zero
                                      beyond the WINDOW edges, before it is fitted; 0 = that axis
                                      is not filtered, all 0 = no lowpass.  At most
                                      CTR_MAX_NOISE_SIZE. */
} ctr_problem;

/* The data of one batch.  All arrays C-contiguous.  For ctr_refine_batch the
 * pointers are HOST pointers; for ctr_refine_batch_device they are DEVICE
 * pointers (hipMalloc'ed memory of the handle's device). */
typedef struct ctr_batch {
  const void* frames;          /* [n_frames, shape...] pixels, dtype frame_dtype */
  int32_t frame_dtype;         /* CTR_DTYPE_* */
  int32_t reserved0;
  int64_t n_frames;
  int64_t shape[CTR_MAX_NDIM]; /* frame shape (z,) y, x; first ndim entries used */
  int64_t n_clusters;          /* C */
  int64_t n_features;          /* N */
  const int32_t* frame_index;  /* [C] index into frames of each cluster */
  const int32_t* feat_offset;  /* [C+1] CSR offsets into the feature table */
  const double* params;        /* [N, n_params] initial parameters (refine.py:345) */
  const double* low;           /* [N, n_params] per-feature lower bounds (fitfunc.py:541-546), -inf = none */
  const double* high;          /* [N, n_params] per-feature upper bounds (fitfunc.py:547-550), +inf = none */
  double* params_out;          /* [N, n_params] refined; equals params for failed clusters */
  double* cost;                /* [C] rms residual / frame max (refine.py:379); NaN on failure */
  int32_t* status;             /* [C] CTR_STATUS_* */
  int32_t* n_rounds;           /* [C] re-window rounds used */
  int32_t* n_iter;             /* [C] solver iterations, summed over rounds */
  double* params_std;          /* [N, n_params] or NULL.  refine.py:400-406 (compute_error):
                                  sqrt(2 diag(inv(H))), H = Hessian of the objective at the
                                  solution over ALL variables of the cluster (bounds and
                                  constraints ignored, as there); here from the exact second
                                  derivatives instead of finite differences.  NaN for constant
                                  parameters, failed clusters and a Hessian that is not positive
                                  definite.  Every parameter mode (second derivatives w.r.t.
                                  signal, centres and sizes).  NaN for clusters of the
                                  large-cluster path (> 64 features) and for the ring / disc /
                                  inv_series profiles: their errors, and the covariance of any
                                  cluster, come from the stage after the fit, ctr_fit_error_device. */
  double* result_rows;         /* [N, n_params + 1] or NULL: params_out and, last column, the cost of
                                  the row's cluster -- the rows of the result table (refine.py:426-427)
                                  in one block, written when the batch is done: what a pipeline sends
                                  on (the multi-GPU gather) without another pass over the outputs.
                                  May be memory of ANOTHER device of the node that this device can
                                  write (peer / IPC-mapped: rank 0's inbox) -- the rows then travel
                                  over xGMI as they are written, no collective per batch */
  int64_t* done_flag;          /* NULL, or where ctr_refine_batch_device stores done_value (one
                                  8-byte store from a kernel of its own, queued last on the call's
                                  stream: after every output above is written); device or peer
                                  memory like result_rows: a consumer polls it per batch.  There is
                                  no flow control: a caller that reuses result_rows / done_flag for a
                                  later batch must have its consumer's acknowledgement first (or one
                                  slot per batch in flight, as bench.py's inbox) */
  int64_t done_value;
} ctr_batch;

typedef struct ctr_handle ctr_handle;
typedef struct ctr_plan ctr_plan;

/* ABI version of the loaded library (== CTR_ABI_VERSION). */
int ctr_abi_version(void);

/* Create / destroy an engine bound to one HIP device.  Owns streams and
 * scratch buffers (frame maxima, work counters).  One caller thread at a time per handle; the
 * *_device calls of one handle are ordered on the device (a call waits for the previous one of
 * the same handle, whatever streams they were given): to overlap batches use one handle each. */
int ctr_create(ctr_handle** out, int device);
void ctr_destroy(ctr_handle* h);

/* Last error text of a failed call on this handle (or of ctr_create when h is NULL). */
const char* ctr_last_error(const ctr_handle* h);

/* Validate a problem descriptor without touching a device. */
int ctr_validate_problem(const ctr_problem* p, char* msg, int msg_len);

/* Number of optimiser variables of a cluster with n features
 * (vect_from_params layout, fitfunc.py:207-263, groups=None). */
int ctr_cluster_n_vars(const ctr_problem* p, int n_features);

/* Which kernel a cluster of n_features goes to (the per-cluster decision of ctr_plan_create,
 * which calls this function); needs no device.  Added in ABI 7 without a version change: it
 * changes no existing struct or call.
 *   bin     CTR_KBIN_*: small kernel (singles / pairs with the default parameter modes), block
 *           kernel by nt, the block kernel's constrained instantiations (dimer / trimer / tetramer
 *           clusters, nt 1..2), large-cluster kernel, or beyond the engine (status 5)
 *   family  CTR_KFAM_*: which table of instantiations the kernel is taken from.  Constrained
 *           clusters take the constrained entry of that table.  GAUSS_TP (CTR_FLAG_THROUGHPUT)
 *           exists in 2D only: a 3D problem with the flag takes the GAUSS table
 *   nt      block and constrained bins: tiles of 16 columns (variables + 1), else 0
 *   lanes   small kernel: lanes per cluster -- singles 8, or 64 when the window of one feature
 *           has more than 600 pixels; pairs 64.  (With CTR_FLAG_THROUGHPUT, a bin of >= 64 pairs
 *           and windows of <= 600 pixels, the pairs that are not closer than a quarter of the mask
 *           radius run 16 lanes each instead: decided on the device per batch.)  Else 0
 *   n_vars  optimiser variables (ctr_cluster_n_vars); -1 when n_features is beyond the engine
 * Returns CTR_ERR_INVALID for a malformed problem or a negative n_features. */
enum { CTR_KBIN_SMALL1 = 1, CTR_KBIN_SMALL2 = 2, CTR_KBIN_BLOCK = 3, CTR_KBIN_CONS = 4,
       CTR_KBIN_LARGE = 5, CTR_KBIN_TOO_LARGE = 6 };
enum { CTR_KFAM_NONE = 0, CTR_KFAM_SMALL = 1, CTR_KFAM_GAUSS = 2, CTR_KFAM_GAUSS_TP = 3,
       CTR_KFAM_LOWPASS = 4, CTR_KFAM_RING = 5, CTR_KFAM_DISC = 6, CTR_KFAM_INV_SERIES = 7,
       CTR_KFAM_LARGE = 8, CTR_KFAM_LARGE_LOWPASS = 9 };
typedef struct ctr_kernel_choice {
  int32_t bin;     /* CTR_KBIN_* */
  int32_t family;  /* CTR_KFAM_*; NONE for CTR_KBIN_TOO_LARGE */
  int32_t nt;
  int32_t lanes;
  int32_t n_vars;
  int32_t reserved0;
} ctr_kernel_choice;
int ctr_cluster_kernel(const ctr_problem* p, int64_t n_features, ctr_kernel_choice* out);

/* Host-pointer entry: copies the batch to the device, runs it, copies the
 * results back.  Synchronous.  Replaces refine.py:343-430. */
int ctr_refine_batch(ctr_handle* h, const ctr_problem* p, const ctr_batch* b);

/* Device-resident path (inputs already in HBM, e.g. frames produced on the
 * GPU): a plan bins the clusters of a batch by problem size on the host once (and owns the
 * HBM workspace of its large clusters: use a plan with the handle it was created on);
 * the run is asynchronous on the given HIP stream (hipStream_t passed as
 * void*; NULL = the handle's own stream). */
int ctr_plan_create(ctr_handle* h, const ctr_problem* p, int64_t n_clusters,
                    const int32_t* feat_offset_host, ctr_plan** out);
void ctr_plan_destroy(ctr_plan* plan);
/* The tail launch of a plan (needs no device beyond the plan's own).  With CTR_FLAG_THROUGHPUT, in
 * 2D, without a lowpass and with the gaussian profile, a plan with at least two non-empty bins
 * among the pairs, the 3-4-feature and the 5-10-feature clusters (block kernel, nt = 1, 2; counts
 * for the default parameter modes) fits the likely slow clusters of those bins -- two features
 * closer than a quarter of the mask radius, or more than 8 features -- in one launch of their own,
 * on at most `cap` workgroups per bin, which share the bin's entries (what else the launch takes:
 * ctr_plan_tail_bins); every cluster is fitted by the same kernel code as without it, the results
 * are the same bits.  fused: 1 if the plan does so; cap: that bound (the same for every plan);
 * tail_grid: workgroups of the launch, the sum over the three bins of min(clusters, cap), 0 if not
 * fused.  Any of the pointers may be null.  Added in ABI 8 without a version change: it changes no
 * existing struct or call. */
int ctr_plan_tail(const ctr_plan* plan, int32_t* fused, int32_t* cap, int32_t* tail_grid);
/* What the tail launch takes of each of its three bins -- [0] the pairs, [1] the 3-4-feature and
 * [2] the 5-10-feature clusters -- beyond the likely slow ones.  The launch lasts as long as the
 * slowest fit of the call on a small part of the machine, and its (at most `cap`) workgroups per
 * bin share the bin's entries through a counter.  In a fused plan:
 *   a block bin of at most max_count clusters (ctr_set_tail_absorb) is fitted whole by the tail
 *     launch and has no launch of its own; of a larger one the tail launch takes the likely slow
 *     clusters, all of them, and the bin's launch the others;
 *   the pairs that would run at 64 lanes -- the likely slow ones where the bin runs in two tiers, all
 *     of them where it runs in one -- are fitted by the tail launch, and the 64-lane launch is not
 *     queued (the 16-lane tier is unchanged).  One tier of more than 8 * cap pairs (windows of more
 *     than 600 pixels) keeps the 64-lane launch for all but the likely slow ones.
 *   absorbed[s]:   1 if the tail launch fits the whole bin s;
 *   own_launch[s]: 1 if the bin's own launch (pairs: the 64-lane one) is queued.
 * A plan that does not fuse, and an empty bin: absorbed 0, own_launch 1 for a non-empty bin.  The
 * results are the same bits whatever the setting.  Either pointer may be null. */
int ctr_plan_tail_bins(const ctr_plan* plan, int32_t absorbed[3], int32_t own_launch[3]);
/* max_count of the rule above for the plans that the handle creates from now on; returns the
 * previous value (-1: null handle).  0: no block bin is fitted whole.  A negative max_count
 * changes nothing (a query).  Default: 32 * cap. */
int32_t ctr_set_tail_absorb(ctr_handle* h, int32_t max_count);
int ctr_refine_batch_device(ctr_handle* h, const ctr_plan* plan,
                            const ctr_batch* b_device, void* hip_stream);

/* Per-frame maximum on the device (the norm of refine.py:354); part of
 * ctr_refine_batch_device, exposed for measurement.  out_max: [n_frames] f64. */
int ctr_frame_max_device(ctr_handle* h, const void* frames, int32_t frame_dtype,
                         int64_t n_frames, int64_t frame_elems, double* out_max,
                         void* hip_stream);

/* Cluster labelling on the device (replaces reference find.py:72-93, the step right
 * before the hot path): rows [frame_offset[f], frame_offset[f+1]) of `pos` are the
 * features of frame f (table sorted by frame); two features of a frame closer than
 * `separation` (per-axis scaled distance <= 1, as cKDTree(pos/separation).query_pairs(1))
 * share a cluster.  label_out[i] = smallest row index of i's cluster (canonical: the
 * reference's own ids depend on Python set order; the partition is the same),
 * size_out[i] = number of features in it.  Host pointers, synchronous. */
int ctr_find_clusters(ctr_handle* h, int32_t ndim, const double* pos, const int32_t* frame_offset,
                      int64_t n_frames, const double* separation, int32_t* label_out, int32_t* size_out);

/* Synthetic frames on the device (the generator next to the hot path):
 * the drawing rule of reference artificial.draw_feature for the Gaussian (artificial.py:131-141:
 * patch [max(floor(c - 4 size), 0), min(ceil(c + 4 size + 1), lim)) per axis,
 * spot = max_value exp(-ndim/2 sum(((idx - c) / size)^2)), TRUNCATED to the pixel type and added
 * with integer wrap-around) and the noise rule of SimulatedImage.noisy_image (:368-378: Poisson
 * noise per pixel, clipped to the pixel type's range).  The noise-free bytes equal the
 * reference rule's; the noise comes from the engine's own counter-based generator (seed, pixel
 * index): same statistics as NumPy's, not the same bytes.  A feature whose centre lies outside
 * its frame is skipped (the reference raises ValueError: check on the host).
 * Device pointers; asynchronous on `hip_stream` (NULL = the handle's stream). */
typedef struct ctr_synth {
  int32_t ndim;                /* 2 or 3 */
  int32_t frame_dtype;         /* CTR_DTYPE_U8 or CTR_DTYPE_U16 */
  int64_t n_frames;
  int64_t shape[CTR_MAX_NDIM]; /* (z,) y, x */
  int64_t n_features;
  const int32_t* frame_of;     /* [N] frame of each feature */
  const double* pos;           /* [N, ndim] centres (z,) y, x */
  const double* size;          /* [N, ndim] radius of gyration per axis (fitfunc.py:112-113) */
  const double* max_value;     /* [N] peak value */
  double noise;                /* Poisson level per pixel, 0 = none */
  uint64_t seed;               /* of the noise */
} ctr_synth;
int ctr_draw_frames_device(ctr_handle* h, const ctr_synth* s, void* frames_out, void* hip_stream);

/* Feature location on the device: the local-maximum rule of reference find.grey_dilation
 * (find.py:166-277) for every frame of a block.  Per frame:
 *   threshold = np.percentile of the non-zero pixels (linear method, NumPy's arithmetic in the
 *     frame's type: float32 for float32 frames, float64 otherwise); NaN (no non-zero pixel, a NaN
 *     pixel) = no features;
 *   box = int(2 separation / sqrt(ndim)) per axis; a pixel is a maximum where it equals the
 *     maximum of its box (scipy.ndimage.grey_dilation, constant border 0: offsets
 *     -((n-1)/2) .. n/2 along an axis of box n) and exceeds the threshold;
 *   maxima closer than `margin` to an edge are dropped;
 *   precise != 0: of two maxima closer than separation (scaled distance <= 1 - 1e-7), the one
 *     lower in the order (pixel value, sum of pos / separation, C-order position) is dropped;
 *     all pairs are decided at once.
 * Positions are written in C order of their frame, frames one after the other.  The total is
 * not known in advance: when *total > capacity only the first `capacity` rows are written (the
 * offsets and the total are complete) and the caller retries with a larger buffer.
 * Device pointers; asynchronous on `hip_stream` (NULL = the handle's stream). */
typedef struct ctr_locate {
  int32_t ndim;                /* 2 or 3 */
  int32_t frame_dtype;         /* CTR_DTYPE_* */
  int64_t n_frames;
  int64_t shape[CTR_MAX_NDIM]; /* (z,) y, x */
  double separation[CTR_MAX_NDIM]; /* per axis, >= 0 */
  double percentile;           /* [0, 100] */
  int64_t margin[CTR_MAX_NDIM];    /* per axis, >= 0 (reference default: int(separation / 2)) */
  int32_t precise;             /* != 0: drop maxima closer than separation to a brighter one */
  int32_t reserved0;
  int64_t capacity;            /* rows of pos_out */
  const void* frames;          /* [n_frames, *shape] */
  int64_t* frame_offset;       /* [n_frames + 1] out: rows of frame t are [off[t], off[t+1]) */
  int32_t* pos_out;            /* [capacity, ndim] out: (z,) y, x */
  int64_t* total;              /* [1] out: rows found (may exceed capacity) */
  double* threshold;           /* [n_frames] out, or NULL: the percentile threshold (NaN: none) */
} ctr_locate;
int ctr_locate_maxima_device(ctr_handle* h, const ctr_locate* l, void* hip_stream);

/* Mass, signal and size of located features on the device: the rule of reference
 * find_link.characterize (find_link.py:44-79), the link between
 * ctr_locate_maxima_device and the start values of a refinement.  Per feature with centre c
 * (any float64; integer when it comes from ctr_locate.pos_out) and integer radius per axis:
 *   window: corner int(round(c - radius)) per axis (half to even), shape 2 radius + 1; pixels
 *     beyond the frame count as 0 (masks.py:9-27);
 *   pixel mask: sum(((idx - (c - corner)) / radius)^2) <= 1 on the unrounded centre, edge
 *     included (masks.py:71-120), evaluated as the refine kernels evaluate it;
 *   mass = sum(window mask) / scale_factor, signal = max(window mask) / scale_factor: masked-out
 *     and padded pixels are zeros that take part in the maximum;
 *   weights over the window offsets k (from the centre of the WINDOW), support
 *     sum((k / radius)^2) <= 1 (trackpy's r_squared_mask / x_squared_masks):
 *     isotropic: size = sqrt(sum(sum_a(k_a^2) window mask) / mass), size[N];
 *     otherwise: size_a = sqrt(ndim sum(k_a^2 window mask) / mass), size[N, ndim].
 *   Integer frames: the sums are exact 64-bit integers, then one float64 division and one
 *   square root.  Float frames: sums in float64.  mass 0 gives size NaN, a negative quotient NaN.
 * Rows [frame_offset[t], frame_offset[t+1]) are the features of frame t (what ctr_locate
 * writes).  Exactly one of pos / pos_i32 is non-NULL.  The descriptor is checked before the
 * handle: with a NULL handle a bad descriptor is reported through the last error of the NULL
 * handle and a good one gives CTR_ERR_INVALID ("null handle").
 * Device pointers; asynchronous on `hip_stream` (NULL = the handle's stream). */
typedef struct ctr_characterize {
  int32_t ndim;                /* 2 or 3 */
  int32_t frame_dtype;         /* CTR_DTYPE_* */
  int64_t n_frames;
  int64_t shape[CTR_MAX_NDIM]; /* (z,) y, x */
  int64_t radius[CTR_MAX_NDIM];    /* per axis, >= 0 */
  int32_t isotropic;           /* != 0: one size per feature */
  int32_t reserved0;
  double scale_factor;         /* divides mass and signal; not 0 (reference default: 1) */
  const void* frames;          /* [n_frames, *shape] */
  int64_t n_features;
  const int64_t* frame_offset; /* [n_frames + 1] */
  const double* pos;           /* [N, ndim] centres (z,) y, x, or NULL */
  const int32_t* pos_i32;      /* [N, ndim] integer centres (ctr_locate.pos_out), or NULL */
  double* mass;                /* [N] out */
  double* signal;              /* [N] out */
  double* size;                /* [N] (isotropic) or [N, ndim] out */
} ctr_characterize;
int ctr_characterize_device(ctr_handle* h, const ctr_characterize* c, void* hip_stream);

/* Preprocessing of whole frames on the device: the reference's lowpass and preprocess
 * (preprocessing.py:13-75) with trackpy's bandpass, scalefactor_to_gamut and scale_to_gamut
 * (DESIGN.md 7b), what runs in front of ctr_locate_maxima_device on raw video.  Per frame:
 *   Gaussian: float64 copy of the frame, then per axis in order correlate1d with the taps of that
 *     axis (n_taps = 2 lw + 1, SciPy's symmetric order: centre tap, then the pairs
 *     (x[i - k] + x[i + k]) * w[lw - k] from k = lw down to 1), zero beyond the frame, every
 *     operation rounded to float64 once.  The taps are the caller's (NumPy's exp, not libm's); a
 *     single tap of 1 leaves the axis as it is.
 *   background: copy of the frame IN THE PIXEL TYPE, then per axis in order a box of box[a] (odd)
 *     over edge-clamped indices: integer pixels trunc(S / box) with S the exact window sum (one
 *     float64 division, C cast), float pixels the float64 window sum divided and rounded to the
 *     pixel type.  A box of 1 leaves the axis as it is.
 *   CTR_PRE_LOWPASS:    out float64 = Gaussian > threshold ? Gaussian : 0
 *   CTR_PRE_BANDPASS:   out float64 = band >= threshold ? band : 0, band = Gaussian - background
 *   CTR_PRE_PREPROCESS: scale_factor = max of the integer type / max of that band over the frame
 *     (one float64 division), out = (integer type)(scale_factor * max(band, 0)), a truncating
 *     cast.  The integer type is the pixel type, uint8 for float frames.  A frame whose band has
 *     no pixel above zero is written as zeros, with scale_factor +inf when its maximum is 0.
 *   CTR_PRE_SCALE:      float frames only, no filter: scale_factor = 255 / max of the frame,
 *     out = (uint8)(scale_factor * max(pixel, 0)).
 * Integer frames: every result equals NumPy / SciPy's bit for bit.  Float frames: the background
 * sums its window in a fixed order, SciPy keeps a running sum, so results agree to rounding.
 * NaN or infinite pixels have no defined result.
 * strategy (CTR_PRE_PREPROCESS): how the maximum is known before the first pixel is written:
 *   CTR_PRE_BAND_PLANE keeps the float64 band in a workspace plane and rescales it,
 *   CTR_PRE_TWICE runs the stencil twice (maximum, then output); CTR_PRE_AUTO picks.  Same result.
 * The halo of a tile lives in LDS: taps or boxes whose tile exceeds 64 KiB give CTR_ERR_UNSUPPORTED.
 * The descriptor is checked before the handle, as for ctr_characterize_device.
 * Device pointers, taps included; asynchronous on `hip_stream` (NULL = the handle's stream). */
enum { CTR_PRE_LOWPASS = 0, CTR_PRE_BANDPASS = 1, CTR_PRE_PREPROCESS = 2, CTR_PRE_SCALE = 3 };
enum { CTR_PRE_AUTO = 0, CTR_PRE_BAND_PLANE = 1, CTR_PRE_TWICE = 2 };
typedef struct ctr_preprocess {
  int32_t ndim;                /* 2 or 3 */
  int32_t frame_dtype;         /* CTR_DTYPE_* */
  int64_t n_frames;
  int64_t shape[CTR_MAX_NDIM]; /* (z,) y, x */
  int32_t mode;                /* CTR_PRE_LOWPASS .. CTR_PRE_SCALE */
  int32_t strategy;            /* CTR_PRE_AUTO .. CTR_PRE_TWICE */
  int32_t n_taps[CTR_MAX_NDIM];    /* per axis, odd, >= 1 */
  int32_t box[CTR_MAX_NDIM];       /* per axis, odd, >= 1 (bandpass, preprocess) */
  const double* taps[CTR_MAX_NDIM];/* per axis [n_taps[a]], on the device */
  double threshold;
  const void* frames;          /* [n_frames, *shape] */
  void* out;                   /* [n_frames, *shape] out: float64, or the integer type */
  double* scale_factor;        /* [n_frames] out (preprocess, scale), else NULL */
} ctr_preprocess;
int ctr_preprocess_device(ctr_handle* h, const ctr_preprocess* p, void* hip_stream);

/* Frame-to-frame linking on the device: the rule of the reference's Linker (Crocker-Grier with
 * sub-network resolution and memory, find_link.py:579-733), what link.link_levels
 * does on the host.  Rows [frame_offset[t], frame_offset[t+1]) of `pos` are the features of level t.
 * Per level t >= 1, sources = the rows of level t - 1 followed by the remembered rows,
 * destinations = the rows of level t, all positions divided per axis by search_range:
 *   candidates: for every destination its up to 10 nearest sources at Euclidean distance
 *     <= 1 + 1e-7 (float64, no contraction); which source is kept when the 10th and 11th are at
 *     exactly the same distance is undefined, as in the reference;
 *   sub-networks: connected components of the candidate graph;
 *   inside a sub-network: the set of links (each source and each destination at most once, along
 *     candidates only) that minimises sum(d^2) + 1 per unlinked source + 1 per missing link, i.e.
 *     maximises sum(2 - d^2); an exact assignment solver, not the reference's order-dependent
 *     recursion.  More than CTR_LINK_MAX_SOURCES sources in a sub-network that is not 1 x 1 is the
 *     reference's SubnetOversizeException: status CTR_LINK_OVERSIZE.  More than
 *     CTR_LINK_MAX_DESTINATIONS destinations is beyond the solver (what CTR_ERR_UNSUPPORTED is for
 *     a synchronous call): status CTR_LINK_CAPACITY;
 *   ids: level 0 gets 0 .. n - 1 in row order; a linked destination takes its source's id; the
 *     unlinked destinations of a level start tracks, numbered from the running count in
 *     lexicographic order of their unscaled position (equal positions in row order);
 *   memory: an unlinked source of level t - 1 is remembered at its last position and stays a
 *     source for `memory` more levels.
 * status[0] = CTR_LINK_*, and for a non-zero one status[1] = the level and status[2] = the size
 * (sources or destinations) it was seen at; status[3] = 0.  With a non-zero status `particle` and
 * `n_tracks` are not a result.  The call zeroes the status itself.
 * The features of a level may be any number that fits in memory (the candidate search of a level
 * costs its destinations times its sources).  Scratch belongs to the handle: calls of one handle
 * are ordered on the device whatever streams they are given.
 * The descriptor is checked before the handle, as for ctr_characterize_device.
 * Device pointers; asynchronous on `hip_stream` (NULL = the handle's stream): read status after
 * synchronising. */
enum { CTR_LINK_OK = 0, CTR_LINK_OVERSIZE = 1, CTR_LINK_CAPACITY = 2 };
#define CTR_LINK_MAX_SOURCES 30
#define CTR_LINK_MAX_DESTINATIONS 64
typedef struct ctr_link {
  int32_t ndim;                /* 2 or 3 */
  int32_t memory;              /* >= 0 */
  int64_t n_levels;
  int64_t n_features;          /* N */
  double search_range[CTR_MAX_NDIM]; /* per axis, > 0 */
  const double* pos;           /* [N, ndim] (z,) y, x; rows sorted by level */
  const int64_t* frame_offset; /* [n_levels + 1] (what ctr_locate writes) */
  int64_t* particle;           /* [N] out: track ids */
  int64_t* n_tracks;           /* [1] out */
  int32_t* status;             /* [4] out */
} ctr_link;
int ctr_link_device(ctr_handle* h, const ctr_link* l, void* hip_stream);

/* ctr_link_device with an adaptive search range (link.py states the same rule): a
 * sub-network beyond the limits does not end the call, its range is shrunk step by step until it
 * falls apart into pieces that can be solved.  A dense restatement of trackpy's published
 * adaptive_link_wrap (adaptive_stop / adaptive_step); parity with trackpy is not pinned.
 * All distances are scaled (position / search_range per axis).  rho_0 = 1, rho_{k+1} = rho_k * step
 * (one double multiplication); stop_rel = max over the axes of adaptive_stop / search_range, formed
 * by the caller; max_rounds = the smallest k with rho_k <= stop_rel, found by that same loop.
 *   round 0: candidates and sub-networks exactly ctr_link_device's.  A 1 x 1 sub-network links; one
 *     of at most CTR_LINK_MAX_SOURCES sources and at most CTR_LINK_MAX_DESTINATIONS destinations is
 *     solved exactly.
 *   an oversize sub-network at round k (more sources or more destinations than that): if
 *     rho_k <= stop_rel the call fails, status CTR_LINK_OVERSIZE for the sources (looked at first),
 *     CTR_LINK_CAPACITY for the destinations, status[1] the level, status[2] the size.  Otherwise
 *     its edges are cut to rho_{k+1}: an edge stays iff d2 <= b * b, b = rho_{k+1} * (1. + 1e-7),
 *     d2 = sum over the axes, in axis order and without contraction, of
 *     (dst_a / sr_a - src_a / sr_a)^2, the number the candidate search stored.  The connected
 *     components of the remaining edges among that sub-network's members are the sub-networks of
 *     round k + 1.  A destination left without an edge starts a track; a source left without an
 *     edge is unlinked and goes to memory as any lost source does.
 *   a sub-network solved at round k maximises sum(2 rho_k^2 - d^2): the cost entry is
 *     d2 - 2. * (rho * rho), trackpy's penalty for a missing link, the current range squared.
 *     k = 0 gives ctr_link_device's bytes.
 *   limits: they stay CTR_LINK_MAX_SOURCES and CTR_LINK_MAX_DESTINATIONS.  trackpy lowers its own
 *     limit to 15 in adaptive mode because its recursion is exponential; the assignment solver here
 *     is not.  So where ctr_link_device succeeds, this call returns the same ids, byte for byte.
 * adaptive_round[i] (may be NULL) is the k of the round in which destination row i was settled: its
 * sub-network was within the limits at rho_k (whether or not the solver linked the row), or the cut
 * to rho_k took its last edge.  0 for the rows of level 0 and for rows without any candidate.
 * Memory, births, ids, status, scratch and streams as ctr_link_device.  The descriptor is checked
 * before the handle: ctr_link's checks, stop_rel and step inside (0, 1), max_rounds in 1..64. */
#define CTR_LINK_MAX_ROUNDS 64
typedef struct ctr_link_adaptive {
  int32_t ndim;                /* the fields of ctr_link */
  int32_t memory;
  int64_t n_levels;
  int64_t n_features;
  double search_range[CTR_MAX_NDIM];
  const double* pos;
  const int64_t* frame_offset;
  int64_t* particle;
  int64_t* n_tracks;
  int32_t* status;
  double stop_rel;             /* in (0, 1) */
  double step;                 /* in (0, 1) */
  int32_t max_rounds;          /* 1 .. CTR_LINK_MAX_ROUNDS */
  int32_t* adaptive_round;     /* [N] out, or NULL */
} ctr_link_adaptive;
int ctr_link_adaptive_device(ctr_handle* h, const ctr_link_adaptive* l, void* hip_stream);

/* ctr_link_device for a sample that moves (link.py states the same rule): a track is
 * looked for where it is expected to be, not where it last was.  The rule is the project's own,
 * after trackpy's nearest-velocity and drift predictors; parity with trackpy is not pinned.
 * Every row i of level t(i) gets a velocity w_i [ndim] in pixels per level once the links of its
 * level are decided.  v0 is initial_velocity.
 *   own velocity of a linked row: for a row i of level t that is linked to source row s of level
 *     t_s, q_i[a] = (p_i[a] - p_s[a]) / (double)(t - t_s): one subtraction and one division.
 *   CTR_LINK_PREDICT_VELOCITY: level 0: w_i = v0.  A linked row: w_i = q_i.  An unlinked row (a
 *     birth) takes w_j of the linked row j of the same level that is nearest in scaled coordinates:
 *     the scaled distance is sum_a (p_i[a] / sr[a] - p_j[a] / sr[a])^2, summed in axis order; a tie
 *     goes to the lower row; there is no distance limit.  If the level has no linked row, the birth
 *     takes v0.
 *   CTR_LINK_PREDICT_DRIFT: one vector per level, u_0 = v0.  For level t >= 1 with M linked rows:
 *     u_t[a] = S_a / M if M > 0, otherwise u_t = u_{t-1}.  S_a is summed in this fixed order:
 *     partial sum l of 256 starts at 0. and adds q_i[a] of the linked rows among rows
 *     r0 + l, r0 + l + 256, .. of the level (r0: its first row), in ascending order; then for
 *     h = 128, 64, .., 1: part[l] += part[l + h] for l < h; S_a = part[0].
 *     w_i = u_t for every row of level t.
 *   prediction: source s (a row of level t_s, the previous level or a remembered one) is offered to
 *     level t at the predicted position P_s.  VELOCITY: P_s[a] = p_s[a] + w_s[a] * (double)(t - t_s);
 *     DRIFT: the same with u_{t-1}[a] in place of w_s[a].  One multiplication, then one addition,
 *     with no contraction.  P_s[a] / sr[a] takes the place of p_s[a] / sr[a] in the candidate
 *     search, and so in the d2 that is stored.
 *   everything else is unchanged: the ten nearest candidates, the 1 + 1e-7 bound, sub-networks, the
 *     exact solver, the limits CTR_LINK_MAX_SOURCES and CTR_LINK_MAX_DESTINATIONS, birth order, ids
 *     and memory.  A remembered source still leaves after `memory` levels; what changes is that it
 *     is predicted forward by its age.
 *   the adaptive range (max_rounds >= 1: the fields and the rule of ctr_link_adaptive;
 *     max_rounds == 0: none, stop_rel, step and adaptive_round are not looked at) composes with
 *     prediction: the rounds work on the d2 of the predicted positions.
 *   limits of the rule: time is counted in levels, and a level without rows is a level.  Without
 *     an initial_velocity, a sample that already moves beyond the range at level 1 never acquires a
 *     velocity: nothing links, and a level without linked rows passes v0 on.
 * velocity (may be NULL) receives w, [N, ndim].  The call is always queued level by level, as
 * ctr_link_device with memory > 0; the host waits for nothing in between.  Status, scratch and
 * streams as ctr_link_device.  The descriptor is checked before the handle: ctr_link's checks, the
 * adaptive fields as above, predictor one of the two, initial_velocity finite. */
enum { CTR_LINK_PREDICT_VELOCITY = 1, CTR_LINK_PREDICT_DRIFT = 2 };
typedef struct ctr_link_predict {
  int32_t ndim;                /* the fields of ctr_link_adaptive */
  int32_t memory;
  int64_t n_levels;
  int64_t n_features;
  double search_range[CTR_MAX_NDIM];
  const double* pos;
  const int64_t* frame_offset;
  int64_t* particle;
  int64_t* n_tracks;
  int32_t* status;
  double stop_rel;
  double step;
  int32_t max_rounds;          /* 0: no adaptive range; else 1 .. CTR_LINK_MAX_ROUNDS */
  int32_t* adaptive_round;     /* [N] out, or NULL */
  int32_t predictor;           /* CTR_LINK_PREDICT_* */
  double initial_velocity[CTR_MAX_NDIM]; /* v0, pixels per level */
  double* velocity;            /* [N, ndim] out, or NULL */
} ctr_link_predict;
int ctr_link_predict_device(ctr_handle* h, const ctr_link_predict* l, void* hip_stream);

/* Relocation candidates of lost features on the device: the rule of the reference's
 * FindLinker.get_relocate_candidates (find_link.py:811-867), the look-again step that
 * makes find_link more than locate followed by link.  The loop around it (shortage per sub-network,
 * merging, the sub-network solved with the claimed candidates) is ctr_find_link_device, below.
 * Derived once per call, as FindLinker.__init__ derives them: box = int(2 separation / sqrt(ndim))
 * per axis (0 filters like 1), slice_radius = int(search_range + radius + 1),
 * bg_radius = slice_radius + radius + 1, max_dist = max(bg_radius / search_range).
 * A query q is a frame t = query_frame[q] and the sources source_pos[source_offset[q] ..
 * source_offset[q + 1]) (any float64, also beyond the frame); the known features of frame t are
 * rows [known_offset[t], known_offset[t + 1]) of known_pos.  Per query:
 *   box: the sources rounded half to even; those beyond the frame by more than slice_radius on an
 *     axis are dropped (masks._in_bounds); origin = max(0, min - slice_radius), end =
 *     min(shape, max + slice_radius + 1); none left = no candidates.  Below, a source is
 *     rel = s - origin and a known feature k - origin (one float64 subtraction each), a pixel its
 *     integer index p in the box;
 *   visible: sum(((p - rel) / slice_radius)^2) <= 1 for any source, the dropped ones included
 *     (masks.py:89; axis order, no contraction);
 *   background: the known features with sum((k / search_range - s / search_range)^2) <=
 *     max_dist * max_dist for any source (frame coordinates, the division first); a visible pixel is
 *     hidden where sum(((p - (k - origin)) / separation)^2) < 1 for any of them (strict);
 *   m(p) = the pixel, in its own type, where visible and not hidden, else 0 -- also beyond the box;
 *   maxima: m(p) equals the maximum of m over the dilation box around p (offsets
 *     -((n-1)/2) .. n/2, 0 beyond the box) and m(p) > threshold[t], both as ctr_locate compares
 *     (float32 frames against the float32 threshold); a NaN threshold = no candidates;
 *   reach: all search_range equal: sum((p - rel)^2) <= search_range^2 for any source, otherwise
 *     sum((p / search_range - rel / search_range)^2) <= 1 (find_link.py:25-41);
 *   drop close: as ctr_locate's `precise` on the maxima within reach, positions in box coordinates:
 *     of two closer than separation (scaled distance <= 1 - 1e-7) the one lower in the order (m,
 *     sum of p / separation, C-order position) goes, all pairs decided at once;
 *   mass, signal, size of every survivor by the rule of ctr_characterize_device ON m (radius,
 *     isotropic, scale_factor; the window is padded with 0 beyond the box, not beyond the frame);
 *   the rows with mass >= minmass, by mass descending; equal masses in C order of position (the
 *     reference: an unstable sort of a set's iteration order).  Positions in frame coordinates.
 * The reference's three early exits (box sums to 0 before or after masking, every m below the
 * threshold) change nothing for frames without negative pixels, where a sum of 0 means all zeros and
 * the threshold of ctr_locate is positive; for frames with negative pixels the result is the rule
 * above WITHOUT the two sum exits (not compared with the reference).
 * Ties: every `<=` above on exact float64 equality decides as written.  They equal cKDTree's
 * decisions on the constructed ties of tests/test_relocate_rule.py.
 * Outputs per query: n_found = rows after the minmass cut (may exceed max_candidates = K); rows
 * [0, min(n_found, K)) of cand_pos / mass / signal / size; the rows behind them are -1 / NaN.
 * status[q]: CTR_RELOCATE_OK; CTR_RELOCATE_CAPACITY for more than CTR_LINK_MAX_SOURCES sources, more
 * than CTR_RELOCATE_MAX_MAXIMA raw maxima in the box (before reach; a saturated plateau) or more than
 * CTR_RELOCATE_MAX_BACKGROUND background features; CTR_RELOCATE_BAD_FRAME for a query_frame outside
 * [0, n_frames) -- reported by the device, not clamped (the host cannot read it).  With a non-zero
 * status n_found[q] is 0 and the rows of q are -1 / NaN; other queries are unaffected.
 * One workgroup per query; m is staged in an LDS tile that holds a one-source box or the thinnest
 * slab of a frame-wide box, whichever is larger, up to CTR_RELOCATE_TILE_BYTES (an untuned choice);
 * a larger box is walked in slabs along axis 0 with the dilation box as halo, and a box so wide that
 * not even one slab fits (box[0] x its other axes > tile: sources spread over a wide frame or a 3D
 * stack) is not staged at all: m is recomputed from the frame in global memory, slower, same result.
 * The frame's size never refuses a call.  No scratch, no floating-point atomics: a query gives the
 * same bytes alone and in any batch.
 * source_offset and known_offset are the caller's and are trusted, like every other offset table of
 * this header: they must rise within [0, S] and [0, n_known] (S is not passed; the known range is
 * kept inside the table, nothing else is checked).
 * ctr_relocate_plan reports the tile (pixels) and the LDS bytes of a launch without a device; it
 * checks the scalars of the descriptor only.
 * The descriptor is checked before the handle, as for ctr_characterize_device.
 * Device pointers; asynchronous on `hip_stream` (NULL = the handle's stream): read status after
 * synchronising. */
enum { CTR_RELOCATE_OK = 0, CTR_RELOCATE_CAPACITY = 1, CTR_RELOCATE_BAD_FRAME = 2 };
#define CTR_RELOCATE_MAX_MAXIMA 256
#define CTR_RELOCATE_MAX_BACKGROUND 512
#define CTR_RELOCATE_TILE_BYTES 32768
typedef struct ctr_relocate {
  int32_t ndim;                /* 2 or 3 */
  int32_t frame_dtype;         /* CTR_DTYPE_* */
  int64_t n_frames;
  int64_t shape[CTR_MAX_NDIM]; /* (z,) y, x */
  int64_t radius[CTR_MAX_NDIM];        /* per axis, >= 0: diameter // 2 */
  double separation[CTR_MAX_NDIM];     /* per axis, > 0 */
  double search_range[CTR_MAX_NDIM];   /* per axis, > 0 */
  int32_t isotropic;           /* != 0: one size per candidate */
  int32_t max_candidates;      /* K >= 1: rows per query */
  double minmass;
  double scale_factor;         /* divides mass and signal; not 0 */
  const void* frames;          /* [n_frames, *shape] */
  const double* threshold;     /* [n_frames]: what ctr_locate.threshold holds; NaN = no candidates */
  int64_t n_known;             /* M */
  const double* known_pos;     /* [M, ndim] (z,) y, x */
  const int64_t* known_offset; /* [n_frames + 1] */
  int64_t n_queries;           /* Q */
  const int64_t* query_frame;  /* [Q] */
  const int64_t* source_offset;/* [Q + 1] */
  const double* source_pos;    /* [S, ndim] */
  int32_t* n_found;            /* [Q] out */
  int32_t* cand_pos;           /* [Q, K, ndim] out */
  double* mass;                /* [Q, K] out */
  double* signal;              /* [Q, K] out */
  double* size;                /* [Q, K] (isotropic) or [Q, K, ndim] out */
  int32_t* status;             /* [Q] out: CTR_RELOCATE_* */
} ctr_relocate;
int ctr_relocate_device(ctr_handle* h, const ctr_relocate* r, void* hip_stream);
int ctr_relocate_plan(const ctr_relocate* r, int64_t* tile_pixels, int64_t* lds_bytes);

/* Find and link with relocation on the device: the loop of the reference's find_link
 * (FindLinker.assign_links, find_link.py:869-911, with Subnets.merge_lost_subnets, :329-370;
 * DESIGN.md 7b) around ctr_link_device's rule and ctr_relocate_device's.  The caller has located
 * the features of every frame (ctr_locate_maxima_device, ctr_characterize_device, mass >= minmass):
 * rows [frame_offset[t], frame_offset[t+1]) of pos / mass / signal / size are the located rows of
 * frame t.  `frames` is what the relocation looks at (the preprocessed frames where there are any),
 * threshold[t] what ctr_locate wrote for them.
 * Level 0: the located rows of frame 0 start tracks in row order.
 * Level t >= 1: destinations = the located rows of frame t; sources = all rows of level t - 1, the
 * relocated ones included, and the rows remembered by ctr_link_device's memory rule.
 *   1. candidates and sub-networks as ctr_link_device forms them; a source without candidate is a
 *      sub-network of its own, without destination;
 *   2. merging: shortage = sources - destinations per sub-network, before any merging; for every
 *      source of a sub-network with a positive one its up to 10 nearest sources (itself and the
 *      remembered ones included) at scaled distance <= 2 + 1e-7; the sub-networks of those sources
 *      unite (a union: the order decides nothing);
 *   3. relocation: every sub-network whose shortage after merging is positive issues one query by the
 *      rule of ctr_relocate_device: its sources, the located rows of frame t as known features,
 *      threshold[t].  Its first min(shortage, n_found) candidates by mass join the destinations, each
 *      a link candidate of every source of the sub-network at scaled distance <= 1 + 1e-7
 *      (sum((c / search_range - s / search_range)^2), axis order);
 *   4. solve: inside a sub-network the links that maximise sum(2 - d^2), from the exact solver of
 *      ctr_link_device (the reference's FindLinker sorts its candidates before the recursion, so its
 *      recursion is exact too: the two differ at ties only).  A claimed candidate becomes a row of
 *      level t with relocated = 1 and the mass, signal and size ctr_relocate_device gave it; an
 *      unclaimed one is dropped; an unlinked located destination starts a track;
 *   5. ids, births and memory as ctr_link_device; a relocated row is never a birth.
 * The short sub-networks of a level do not see each other's claimed candidates (the reference adds
 * them to the background of the queries it issues later, in dict order): coupled[t] = 1 where a
 * claimed candidate lies at scaled distance <= max_dist (ctr_relocate_device) of a source of another
 * query of the level -- only there could the reference's result differ.
 * Output: the rows of all levels packed in level order, the located rows of a level in their order,
 * then its relocated rows in C order of position; frame_offset_out[T] is their number (at most
 * n_located + (n_frames - 1) * max_relocated, the rows the output arrays must hold).
 * status[0] = CTR_FIND_LINK_*, for a non-zero one status[1] = the level and status[2] = a size:
 * OVERSIZE more than CTR_LINK_MAX_SOURCES sources in a sub-network after merging; CAPACITY more than
 * CTR_LINK_MAX_DESTINATIONS destinations, relocated included; RELOCATE a query ended with a
 * non-zero status (status[2]); QUERIES more than max_queries short sub-networks in the level; ROWS
 * more than max_relocated claimed candidates.  The first level that fails is reported; no kernel
 * stops, and with a non-zero status no output is a result.  The call zeroes status and coupled.
 * Levels are queued one after the other on the stream (candidates, merge, relocation with
 * max_queries workgroups -- one without sources ends at once --, solve); nothing crosses to the host
 * in between.  Scratch belongs to the handle (the block of ctr_link_device); no floating-point
 * atomics: the same bytes on any stream.
 * The descriptor is checked before the handle, as for ctr_characterize_device.
 * Device pointers; asynchronous on `hip_stream` (NULL = the handle's stream): read status after
 * synchronising. */
enum { CTR_FIND_LINK_OK = 0, CTR_FIND_LINK_OVERSIZE = 1, CTR_FIND_LINK_CAPACITY = 2, CTR_FIND_LINK_RELOCATE = 3,
       CTR_FIND_LINK_QUERIES = 4, CTR_FIND_LINK_ROWS = 5 };
typedef struct ctr_find_link {
  int32_t ndim;                /* 2 or 3 */
  int32_t frame_dtype;         /* CTR_DTYPE_* */
  int64_t n_frames;            /* T */
  int64_t shape[CTR_MAX_NDIM]; /* (z,) y, x */
  int64_t radius[CTR_MAX_NDIM];        /* per axis, >= 0: diameter // 2 */
  double separation[CTR_MAX_NDIM];     /* per axis, > 0 */
  double search_range[CTR_MAX_NDIM];   /* per axis, > 0 */
  int32_t isotropic;           /* != 0: one size per row */
  int32_t memory;              /* >= 0 */
  int32_t max_queries;         /* 1 .. 1024: relocation queries per level */
  int32_t max_relocated;       /* 1 .. 1024: relocated rows per level */
  double minmass;              /* of a relocation candidate */
  double scale_factor;         /* of a relocation candidate's mass and signal; not 0 */
  const void* frames;          /* [T, *shape] */
  const double* threshold;     /* [T] */
  int64_t n_located;           /* M */
  const double* pos;           /* [M, ndim] located rows, sorted by frame */
  const int64_t* frame_offset; /* [T + 1] */
  const double* mass;          /* [M] */
  const double* signal;        /* [M] */
  const double* size;          /* [M] (isotropic) or [M, ndim] */
  int64_t capacity;            /* rows of the outputs: >= M + (T - 1) * max_relocated */
  double* pos_out;             /* [capacity, ndim] out */
  int64_t* frame_offset_out;   /* [T + 1] out */
  int64_t* particle;           /* [capacity] out */
  double* mass_out;            /* [capacity] out */
  double* signal_out;          /* [capacity] out */
  double* size_out;            /* [capacity] or [capacity, ndim] out */
  uint8_t* relocated;          /* [capacity] out */
  int64_t* n_tracks;           /* [1] out */
  int32_t* coupled;            /* [T] out */
  int32_t* status;             /* [4] out */
} ctr_find_link;
int ctr_find_link_device(ctr_handle* h, const ctr_find_link* f, void* hip_stream);

/* Centre-of-mass refinement of features on the device: what the reference's find_link(refine=True)
 * asks of trackpy.refine(image, image, radius, coords, separation=0, characterize=False)
 * (find_link.py:436-465).  trackpy is not part of the reference's tree: the rule
 * below is its refine_com loop RESTATED from the published source and made total (step 1); parity
 * with trackpy itself is not pinned.
 * Inputs of one feature: a frame of `shape`; a start c, each axis rounded half to even to an
 * integer; an integer radius r, at least 1 per axis, with 2 r[a] + 1 <= shape[a]; max_iterations
 * (1 .. 100; trackpy's default 10); shift_thresh (> 0; trackpy's default 0.6).
 * Mask: the window offsets k with -r[a] <= k[a] <= r[a] and sum((k[a] / r[a])^2) <= 1, the support
 * of ctr_characterize_device's weights.
 *   1. clip c to [r, shape - 1 - r] per axis (trackpy does not, and would slice out of the frame: a
 *      relocated row can lie closer to the edge than r);
 *   2. evaluate the window at c: m = the sum of the masked pixels, cm[a] = the sum of the masked
 *      pixels times j[a], divided by m, with j = k + r (the window index from 0);
 *      off[a] = cm[a] - r[a]; if any cm[a] is NaN (m == 0; trackpy's _safe_center_of_mass): off = 0.
 *      Integer frames: both sums are exact in int64 and each is converted to float64 once.  Float
 *      frames: float64 sums (pixels outside the mask are multiplied by 0, as NumPy's mask * image);
 *   3. if abs(off[a]) < shift_thresh on every axis: stop;
 *   4. otherwise c[a] += 1 where off[a] > shift_thresh, c[a] -= 1 where off[a] < -shift_thresh, clip as
 *      in step 1 and, if fewer than max_iterations windows have been evaluated, go to step 2.
 * Result, all of it from the last evaluated window and the c it was evaluated at, not from a move
 * made after it: pos[a] = (cm[a] - r[a]) + c[a] in that order (float64, no contraction); mass = m
 * as float64, not divided by any scale factor; n_iter = the number of windows evaluated.  An off
 * exactly equal to the threshold neither stops nor moves: the same window is evaluated until
 * max_iterations.
 * Rows [frame_offset[t], frame_offset[t+1]) of pos are the features of frame t (what ctr_locate and
 * ctr_find_link write).  pos_out may be pos.  A NaN start has no defined result (the Python layer
 * refuses it).  No scratch, no atomics: the same bytes in any launch.
 * The descriptor is checked before the handle, as for ctr_characterize_device.
 * Device pointers; asynchronous on `hip_stream` (NULL = the handle's stream). */
typedef struct ctr_refine_com {
  int32_t ndim;                /* 2 or 3 */
  int32_t frame_dtype;         /* CTR_DTYPE_* */
  int64_t n_frames;
  int64_t shape[CTR_MAX_NDIM]; /* (z,) y, x */
  int64_t radius[CTR_MAX_NDIM];    /* per axis, >= 1, 2 radius + 1 <= shape */
  int32_t max_iterations;      /* 1 .. 100 */
  int32_t reserved0;
  double shift_thresh;         /* > 0 */
  const void* frames;          /* [n_frames, *shape] */
  int64_t n_features;          /* N */
  const int64_t* frame_offset; /* [n_frames + 1] */
  const double* pos;           /* [N, ndim] starts (z,) y, x */
  double* pos_out;             /* [N, ndim] out */
  double* mass;                /* [N] out */
  int32_t* n_iter;             /* [N] out */
} ctr_refine_com;
int ctr_refine_com_device(ctr_handle* h, const ctr_refine_com* c, void* hip_stream);

/* ctr_find_link_device with the refinement above after every level: the reference's
 * find_link(refine=True), whose after_link callback refines the features of a level and whose
 * linker.set_dataframe writes the positions back into the points (find_link.py:651-654, 1001-1007).
 * `com` supplies the raw frames ([T, *shape]), their dtype, max_iterations and shift_thresh; its
 * ndim, n_frames, shape and radius must equal f's (else CTR_ERR_INVALID naming the field); its
 * table pointers (n_features, frame_offset, pos, pos_out, mass, n_iter) are ignored.
 * The rows of level 0 are refined before the first level is linked; the rows of level t >= 1, its
 * claimed relocated rows included, after step 4 of that level.  The refinement is in place in the
 * linker's table: position and mass of the row become pos and mass of ctr_refine_com.  So the
 * sources of level t + 1 (the remembered ones keep what they had), the sources of the relocation
 * queries, the coupled test (whose claimed candidates are still whole pixels when it runs) and the
 * emitted table see refined values; the destinations of a level are linked from where they were
 * located; the known features that the relocation masks with stay the located ones
 * (find_link.py:827); signal and size stay from the unrefined position.  The relocated rows of a
 * level are emitted in C order of their refined position.
 * Everything else, the status words included, as ctr_find_link_device. */
int ctr_find_link_refine_device(ctr_handle* h, const ctr_find_link* f, const ctr_refine_com* com, void* hip_stream);

/* Orientation of tracked clusters on the device: the rule of the reference's motion.orientation_df
 * (motion.py:40-162), the step behind ctr_link_device.  `pos` holds, per track and
 * frame, the features of the cluster in the order of their `particle`; a frame in which the cluster
 * is not complete is NaN (any non-finite coordinate marks the frame as missing).  Per frame:
 *   coordinates: pos * mpp, reversed to x, y(, z);
 *   permutations: P = 2, 6, 12 for cluster_size 2, 3, 4, the reference's tables in its order
 *     (motion.py:137-145).  The weights are NOT permuted with the coordinates: permutation p has the
 *     centre of mass com_p = sum_i(weights[i] c[perm_p[i]]) / sum(weights);
 *   2D (sizes 2, 3): x = unit(c[perm_p[0]] - com_p) padded with 0, z = (0, 0, 1), y = unit(z x x);
 *   3D: z = unit(c[perm_p[0]] - com_p);
 *     size 3: x = unit(z x (c[perm_p[1]] - com_p));  size 4: x = unit(z x (c[perm_p[2]] - c[perm_p[1]]));
 *     size 2: x = unit(R(z, angle) ([1, 0, 0] x z)) with R the rotation matrix of motion.py:3-16 and
 *       angle = angles[t, p, f], in radians (the reference draws 2 pi np.random.random() here);
 *     y = unit(z x x);
 *   bases[t, p, f] = rows x, y, z; a basis with a non-finite entry (coincident features, a collinear
 *     trimer, a dimer along [1, 0, 0]) is written as nine NaN; the reference's check_orthonormality
 *     is not reproduced;
 *   com[t, f] = the centre of mass of the LAST permutation, padded with 0 in 2D.
 * A missing frame gives NaN com and bases.  cluster_size 1 and the 2D tetramer are CTR_ERR_UNSUPPORTED,
 * a 3D dimer without angles CTR_ERR_INVALID.
 * The descriptor is checked before the handle, as for ctr_characterize_device.
 * Device pointers; asynchronous on `hip_stream` (NULL = the handle's stream). */
typedef struct ctr_orientation {
  int32_t ndim;            /* 2 or 3 */
  int32_t cluster_size;    /* 2..4 as allowed above */
  int64_t n_tracks, n_frames;
  double  mpp;
  double  weights[4];      /* sizes**ndim, computed by the caller */
  const double* pos;       /* [T, F, cluster_size, ndim] (z,) y, x in px; NaN = missing */
  const double* angles;    /* [T, P, F] or NULL (required for 3D dimers) */
  double* com;             /* [T, F, 3] out */
  double* bases;           /* [T, P, F, 3, 3] out */
} ctr_orientation;
int ctr_orientation_device(ctr_handle* h, const ctr_orientation* o, void* hip_stream);

/* Diffusion tensor of tracked clusters on the device: the rule of the reference's
 * motion.diffusion_tensor (motion.py:165-198) for every track and every lag of a sweep
 * in one call.  Per track t, lag k, permutation p and frame b with b + k < n_frames:
 *   translation = bases[t, p, b] (positions[t, b + k] - positions[t, b]),
 *   rotation    = 0.5 sum_i e_i x (bases[t, p, b] bases[t, p, b + k, i]),
 *   x = (translation, rotation); a row with a non-finite component is dropped; the rows of all
 *   permutations are pooled:
 *   tensor[t, k] = mean(x x^T) * 0.5 / (k / fps); ndim 2 keeps the components [0, 1, 5] (3 x 3), ndim
 *   3 all six (6 x 6); n_samples[t, k] = rows that entered the mean; none (also k >= n_frames or
 *   k < 1): a NaN tensor and 0.
 * The frames of a (track, permutation) are cut into tiles of 256 whatever the lags are; a workgroup
 * stages its tile and the halo behind it in LDS (as many frames as 64 KiB hold), loops
 * over the lags and writes one partial sum per (track, lag, permutation, tile); a later frame beyond
 * the staged halo is read from global memory.  A second kernel adds the partials of a (track, lag)
 * in the order permutation, tile.  No floating-point atomics: the result of a (track, lag) is the
 * same bytes whatever else the call holds.
 * Scratch (the partials) belongs to the handle: calls of one handle are ordered on the device
 * whatever streams they are given.
 * The descriptor is checked before the handle, as for ctr_characterize_device.
 * Device pointers, lags included; asynchronous on `hip_stream` (NULL = the handle's stream). */
typedef struct ctr_diffusion {
  int32_t ndim;            /* 2 -> 3x3, 3 -> 6x6 */
  int32_t n_perm;
  int64_t n_tracks, n_frames, n_lags;
  double  fps;
  const int64_t* lags;     /* [n_lags], each >= 1 (validated on the host side of the wrapper) */
  const double* positions; /* [T, F, 3] */
  const double* bases;     /* [T, P, F, 3, 3] */
  double*  tensor;         /* [T, n_lags, D, D] out */
  int64_t* n_samples;      /* [T, n_lags] out: rows that entered the mean */
} ctr_diffusion;
int ctr_diffusion_device(ctr_handle* h, const ctr_diffusion* d, void* hip_stream);

/* Bootstrap confidence interval of the diffusion tensor on the device: the reference's
 * motion.diffusion_tensor_ci (motion.py:201-216), which calls scikits.bootstrap.ci on the pooled
 * displacement rows.  That package's ci is restated here from its published source; parity with the
 * package itself is not pinned.  For every pair = (track, lag) -- with pool_tracks every
 * lag, over the rows of all tracks -- of a call:
 *   rows: x[n, D], the rows of ctr_diffusion_device in the order (track,) permutation, frame, those
 *     with a non-finite component dropped; ndim 2 keeps the components [0, 1, 5] (D = 3), ndim 3 all
 *     six (D = 6);
 *   statistic: stat(x) = mean_k(x_k x_k^T) * 0.5 / (lag / fps), D x D; ostat = stat(x) (`tensor`);
 *   resamples b = 0 .. B - 1 (B = n_samples): s_b = stat(x[idx[b, :]]), idx[b, k] for k = 0 .. n - 1
 *     drawn with replacement by a counter-based generator that depends on (seed, b, k, n) alone:
 *       r = mix64(mix64(seed) + ((b << 32) + k + 1) * 0x9E3779B97F4A7C15 mod 2^64),
 *       idx[b, k] = floor(r n / 2^64)   (the high half of the 128-bit product),
 *     mix64 the finaliser of splitmix64: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *     z *= 0x94D049BB133111EB; z ^= z >> 31.  The products of a resample are added in the order of k;
 *   sort: every entry (i, j) of s is sorted over b, ascending;
 *   method CTR_CI_PI (percentile): avals = alphas;
 *   method CTR_CI_BCA: z0 = Phi^-1(#{b: s_b < ostat} / B) (-inf / +inf where no / every resample lies
 *     below); the acceleration a = sum(d^3) / (6 sum(d^2)^1.5) with d_k = p_k - mean(p), p_k =
 *     x_ki x_kj -- the jackknife form sum((jm - j_k)^3) / (6 sum((jm - j_k)^2)^1.5) of the package,
 *     j_k = stat(x without row k), of which jm - j_k is a positive multiple of d_k;
 *     zs = z0 + z_alpha; avals = Phi(z0 + zs / (1 - a zs)); z_alpha = Phi^-1(alphas) is the caller's;
 *   rank = round_half_even((B - 1) avals), 0 where avals is NaN (0 / 0 in a, z0 infinite), as the
 *     package's nan_to_num; interval[q, i, j] = sorted s[rank[q, i, j], i, j].
 * z0 and a are written for both methods.  A pair without rows (also lag >= n_frames or lag < 1) gives
 * a NaN interval, tensor, z0 and a, ranks 0 and n_rows 0.
 * The launch decision (ctr_diffusion_ci_plan reports it without a handle or a device; it checks the
 * scalars of the descriptor only) follows n_max = n_perm n_frames (times n_tracks when pooled), the
 * host-known bound on n, never n itself:
 *   rows_in_lds: n_max rows fit into CTR_DIFFUSION_CI_LDS_BYTES (8 D n_max <= it): a workgroup of 512
 *     resamples stages the rows of its pair in LDS once (lds_bytes = 8 D n_max) and gathers from there;
 *     otherwise (lds_bytes 0) the rows are gathered from the scratch in global memory;
 *   the scratch of a pair: 8 (D n_max + D (D + 1) / 2 B + 1) bytes -- rows, the distinct entries of
 *     the statistics, n; pairs_per_chunk = min(pairs, CTR_DIFFUSION_CI_SCRATCH_BYTES / that), and
 *     scratch_bytes = pairs_per_chunk times that.  A call with more pairs is processed in chunks on
 *     the stream, without a host synchronisation; a single pair that does not fit is
 *     CTR_ERR_UNSUPPORTED, and so is n_samples > CTR_DIFFUSION_CI_MAX_SAMPLES (an entry's statistics
 *     are sorted in the LDS of one workgroup: 128 KiB).
 * No floating-point atomics, no sum across lanes in a resample: a pair gives the same bytes alone, in
 * a batch, in a sweep and in any chunking.  The scratch is ctr_diffusion_device's and belongs to the
 * handle: calls of one handle are ordered on the device whatever streams they are given.
 * tensor, n_rows, z0, accel and ranks may be NULL.  The descriptor is checked before the handle, as
 * for ctr_characterize_device.  Device pointers, lags included; asynchronous on `hip_stream`
 * (NULL = the handle's stream). */
enum { CTR_CI_BCA = 0, CTR_CI_PI = 1 };
#define CTR_DIFFUSION_CI_MAX_SAMPLES 16384
#define CTR_DIFFUSION_CI_MAX_ALPHA 8
#define CTR_DIFFUSION_CI_LDS_BYTES 65536
#define CTR_DIFFUSION_CI_SCRATCH_BYTES 268435456
typedef struct ctr_diffusion_ci {
  int32_t ndim;            /* 2 -> 3x3, 3 -> 6x6 */
  int32_t n_perm;
  int64_t n_tracks, n_frames, n_lags;
  double  fps;
  const int64_t* lags;     /* [n_lags] */
  const double* positions; /* [T, F, 3] */
  const double* bases;     /* [T, P, F, 3, 3] */
  int64_t  n_samples;      /* B in [1, CTR_DIFFUSION_CI_MAX_SAMPLES] */
  uint64_t seed;
  int32_t  method;         /* CTR_CI_BCA or CTR_CI_PI */
  int32_t  n_alpha;        /* K in [1, CTR_DIFFUSION_CI_MAX_ALPHA] */
  double   z_alpha[CTR_DIFFUSION_CI_MAX_ALPHA];  /* Phi^-1(alphas), taken on the host (CTR_CI_BCA) */
  double   alphas[CTR_DIFFUSION_CI_MAX_ALPHA];   /* probabilities */
  int32_t  pool_tracks;    /* != 0: one interval per lag over the rows of all tracks (Np = n_lags, else T n_lags) */
  double*  interval;       /* [Np, K, D, D] out */
  double*  tensor;         /* [Np, D, D] out: ostat */
  int64_t* n_rows;         /* [Np] out: n */
  double*  z0;             /* [Np, D, D] out */
  double*  accel;          /* [Np, D, D] out: a */
  int64_t* ranks;          /* [Np, K, D, D] out */
} ctr_diffusion_ci;
int ctr_diffusion_ci_device(ctr_handle* h, const ctr_diffusion_ci* d, void* hip_stream);
int ctr_diffusion_ci_plan(const ctr_diffusion_ci* d, int32_t* rows_in_lds, int64_t* lds_bytes, int64_t* scratch_bytes,
                          int64_t* pairs_per_chunk);

/* Training of shared fit parameters on the device: what the reference's train_leastsq
 * (refine.py:455-515) asks of refine_leastsq -- positions, signal and background constant, the
 * size column(s) and the profile's own parameters fitted as ONE value shared by all features
 * (param_mode 'global').  With every other parameter constant the unknowns of a
 * problem are its G shared values alone (1 to 8), the windows never move, and the objective is a
 * sum over clusters.  General global mode (per-feature variables beside shared ones: an arrowhead
 * system over all clusters) is ctr_refine_global_device, below; ctr_validate_problem, and with it
 * ctr_refine_batch, and this call still refuse it.
 * A call holds P independent problems; problem p owns the clusters [problem_offset[p],
 * problem_offset[p + 1]), cluster c the features [feat_offset[c], feat_offset[c + 1]) of `params`
 * and the frame frame_index[c].  For one problem:
 *   objective: F(g) = (1 / norm) sum_c (1 / P_c) sum_{pixels of c} (I - bg_c - sum_{i in c, pixel in
 *     mask_i} s_i f(r2_i(g), g))^2 (fitfunc.py:436-450): bg_c the background of the cluster's first
 *     feature; a pixel whose residual is NaN (a NaN pixel; ring and disc within one pixel of a
 *     centre, fitfunc.py:20-26) is left out of the sum and still counts in P_c (np.nansum);
 *   windows and masks: those of ctr_refine_batch to the letter -- the union window of the cluster
 *     from the centres rounded half to even, the centres beyond the frame by more than the radius
 *     left out, clipped to the frame (masks.py:42-68); a feature counts only inside its own mask
 *     sum(((idx - (c - origin)) / radius)^2) <= 1 on the unrounded centre, evaluated without
 *     contraction at the boundary; P_c = the pixels of the window inside any mask;
 *   norm = (max over the frames of the problem's clusters of frame.max())^2 / residual_factor
 *     (refine.py:325-331): ONE maximum for the problem, not one per frame; a NaN maximum is passed
 *     over, as Python's max(norm, nan) does;
 *   variables, in the order of the columns: every column with mode CTR_MODE_GLOBAL.  Only the size
 *     column(s) and the profile's columns may be global, every other mode must be CTR_MODE_CONST
 *     (else CTR_ERR_UNSUPPORTED), and at least one column is global;
 *   start, low, high [P, G] are the caller's: the mean of the column over the problem's features
 *     (refine.py:361), the minimum of the per-feature lower and the maximum of the per-feature upper
 *     bounds of fitfunc.py:535-558; the start is clipped into the box; low > high fails the problem;
 *   one window round: the positions are constant (refine.py:384 breaks at once);
 *   minimiser: the engine's bounded Levenberg-Marquardt on the G variables with the
 *     Gauss-Newton matrix: active set on the box, (J^T J + mu diag(J^T J)) d = -g on the free
 *     variables, projection, predicted decrease, trial evaluation, Nielsen's update; mu0 = 1 (a size
 *     is always among the variables); converged at a relative step <= xtol after an accepted step or
 *     |predicted decrease| <= ftol F / 2; at most solver_maxiter iterations, where a last accepted
 *     step that lowered F by less than 1e-9 (relative) still counts as converged; an evaluation
 *     with a size of 0 is not valid and is rejected; a trial whose F equals the accepted point's to
 *     within 16 units in the last place is accepted where its projected gradient is the smaller
 *     (the decrease of F drops below the rounding of its sum before the gradient does);
 *   result: globals[p, :] the G values, cost[p] = sqrt(F / residual_factor), n_iter[p] the
 *     iterations, status[p] a CTR_STATUS_*: NONFINITE a non-finite entry in the parameters of the
 *     problem's features, OUT_OF_BOUNDS a cluster without a pixel (no centre near the frame; also a
 *     problem without clusters and a frame_index beyond the frames), NO_CONVERGENCE, RMS_DEV
 *     cost > max_rms_dev, TOO_LARGE a cluster of more than 64 features.  A failed problem has NaN
 *     globals and cost; it never stops a kernel and leaves the other problems' bytes as they are.
 * Per iteration two kernels run on the stream: one workgroup per cluster sums the weighted J^T J,
 * J^T r and r^2 of its pixels at the trial point in float64 and reduces them, lanes then wavefronts in
 * a fixed order, into its row of a table; one workgroup per problem adds the rows of its clusters
 * in a fixed order and does the bookkeeping of the iteration.  No floating-point atomics, no
 * workgroup waits for another: the same bytes on any stream, alone and in any batch.  The
 * workgroups of a finished problem return at once.
 * check_every = 0: solver_maxiter + 1 iterations are queued blind and the call is asynchronous.
 * check_every = K > 0: the host reads one word every K iterations and stops queueing when every
 * problem has finished; the call then returns with the stream synchronised.  Same results.
 * problem_offset must rise from 0 to C (problem_offset[p] <= problem_offset[p + 1]): the device checks
 * each problem's own range, not that the ranges of different problems are disjoint; overlapping
 * ranges give undefined globals with a status of OK.
 * max_features is the caller's statement of the largest cluster (the host cannot read
 * feat_offset): more than 64 is CTR_ERR_UNSUPPORTED; the device checks every cluster again.
 * Scratch (the table, the solver state, the frame maxima) belongs to the handle: calls of one
 * handle are ordered on the device whatever streams they are given.
 * The descriptor is checked before the handle, as for ctr_characterize_device.
 * Device pointers; asynchronous on `hip_stream` (NULL = the handle's stream) unless check_every. */
#define CTR_TRAIN_MAX_GLOBALS 8
#define CTR_TRAIN_MAX_FEATURES 64
typedef struct ctr_train {
  int32_t ndim;                    /* 2 or 3 */
  int32_t isotropic;               /* 1: one 'size' column; 0: one per axis */
  int32_t fit_function;            /* CTR_FIT_* */
  int32_t n_params;                /* as ctr_problem.n_params */
  int32_t modes[CTR_MAX_PARAMS];   /* CTR_MODE_CONST or CTR_MODE_GLOBAL per column */
  int32_t radius[CTR_MAX_NDIM];    /* mask radius per axis, >= 1 */
  int32_t frame_dtype;             /* CTR_DTYPE_* */
  int32_t solver_maxiter;          /* 1 .. 10000 (refine.py:243; default 100) */
  int32_t max_features;            /* features of the largest cluster, <= CTR_TRAIN_MAX_FEATURES */
  int32_t check_every;             /* 0, or iterations between two looks at the finished count */
  int64_t n_frames;
  int64_t shape[CTR_MAX_NDIM];     /* (z,) y, x */
  int64_t n_problems;              /* P */
  int64_t n_clusters;              /* C */
  int64_t n_features;              /* N */
  double residual_factor;          /* > 0 (default 1e5) */
  double max_rms_dev;              /* refine.py:391 (default 1) */
  double xtol;                     /* <= 0 -> 1e-9 */
  double ftol;                     /* <= 0 -> 1e-14 */
  const void* frames;              /* [n_frames, *shape] */
  const double* params;            /* [N, n_params] */
  const int32_t* feat_offset;      /* [C + 1] */
  const int32_t* frame_index;      /* [C] */
  const int32_t* problem_offset;   /* [P + 1] offsets into the clusters */
  const double* start;             /* [P, G] */
  const double* low;               /* [P, G], -inf = none */
  const double* high;              /* [P, G], +inf = none */
  double* globals;                 /* [P, G] out */
  double* cost;                    /* [P] out */
  int32_t* status;                 /* [P] out */
  int32_t* n_iter;                 /* [P] out */
} ctr_train;
int ctr_train_device(ctr_handle* h, const ctr_train* t, void* hip_stream);

/* ---- shared and per-feature parameters in one problem: general global mode (ABI 8, additions) ----
 * What the reference's refine_leastsq does with a param_mode 'global' (refine.py:317-332): the G
 * global columns are ONE value for all features of a problem, fitted together with whatever varies
 * per feature ('var') or per cluster ('cluster').  Training (above) is the case without locals.
 * A call holds P independent problems laid out as ctr_train lays them out (problem_offset,
 * feat_offset, frame_index, params [N, n_params]).  For one problem:
 *   objective: windows, union boxes, masks, P_c, the NaN-pixel rule, bg_c (the background of the
 *     cluster's first feature) and the ONE norm per problem are those of the training rule to the
 *     letter; the masks are built on the mask centres of the round, the model on the trial positions;
 *   modes per column: CTR_MODE_CONST, _VAR, _CLUSTER, _GLOBAL.  At least one column is global
 *     (else CTR_ERR_INVALID); background, signal, the size column(s) and the profile's columns may
 *     be; a global position is CTR_ERR_UNSUPPORTED; the background is never VAR (fitfunc.py:389-392);
 *   variables: the G <= 8 global columns, in column order, are the shared variables.  The locals of
 *     cluster c, L_c of them, in column order: a CLUSTER column one entry, a VAR column one entry per
 *     feature of the cluster in row order.  L_c = 0 is allowed; a problem whose clusters all have
 *     L_c = 0 is a training problem;
 *   start and bounds are the caller's (refine.py:361-364, fitfunc.py:535-558): start, low, high
 *     [P, G] as in training; local_start, local_low, local_high [C, max_locals], row c holding the
 *     L_c locals of cluster c in the order above (a VAR entry its own value and bounds, a CLUSTER
 *     entry the mean over the cluster's rows, the min of the lows and the max of the highs).  The
 *     start is clipped into the box; low > high anywhere fails the problem (NO_CONVERGENCE);
 *   rounds (refine.py:365-388): up to max_iter window rounds.  Every round minimises from the
 *     call's start vector with the call's bounds; only the mask centres move, to the last round's
 *     positions.  The rounds end when every feature of the problem is less than max_shift from
 *     its mask centre (squared distance < max_shift^2), as ctr_refine_batch does per cluster; after
 *     the last round cost = sqrt(F / residual_factor);
 *   minimiser: the training's bounded Levenberg-Marquardt on the whole vector, everything as written
 *     there: Gauss-Newton matrix, Marquardt scaling by its diagonal, active set on the box,
 *     projection, predicted decrease of the full model at the projected step, Nielsen's update,
 *     mu0 = 1, the stopping tests and the flat-trial rule (the projected gradient over locals and
 *     globals).  The damped matrix is an arrowhead -- a block A_c + mu D_c per cluster, its coupling
 *     B_c to the G shared columns, the G x G corner -- and the step is solved in four stages: the
 *     free locals of every cluster are eliminated with a Cholesky in the cluster's workgroup; the
 *     Schur rows G_c - B_c^T (A_c + mu D_c)^-1 B_c and the reduced gradients are summed per problem
 *     in a fixed order; the G x G system is solved in the problem's workgroup; every cluster
 *     back-substitutes and projects.  A block or a corner that is not positive definite rejects the
 *     step (more damping) without a pixel pass;
 *   result: params_out [N, n_params] (the fitted columns of the problem's rows, every other entry
 *     as in params), globals [P, G], cost [P], status [P], n_rounds [P], n_iter [P] (iterations of
 *     all rounds).  A failed problem leaves its rows as they came in and has NaN cost and globals
 *     (refine.py:408-412); statuses as in training; TOO_LARGE: a cluster of more than 64 features,
 *     of more than max_locals locals or of more than 48 columns (L_c + G + 1).  A failed problem
 *     never stops a kernel and leaves the other problems' bytes alone.
 * Per iteration four kernels run on the stream (global_kernels.h): one workgroup per cluster
 * back-substitutes and builds the rows [J_local | J_global | r] of its window in LDS row tiles,
 * contracted with v_mfma_f64_16x16x4_f64 (A_c, B_c, the cluster's part of the corner, both gradients
 * and F_c out of one contraction); one workgroup per problem judges the trial; one wavefront per
 * cluster factors and forms its Schur row; one workgroup per problem solves the corner.  A cluster
 * keeps A_c, B_c, g_c of the accepted point in a row of the handle's scratch sized by max_locals, so
 * a rejected trial costs no second pixel pass.  The kernel boundary is the only synchronisation; no
 * floating-point atomics; every sum in an order fixed by the cluster alone (its pixels go in tiles of
 * 64 to four virtual waves, tile k to k mod 4, whose partial sums are added in their order, however
 * many wavefronts and column tiles the call's largest cluster makes the kernel use): the same bytes
 * alone, in a batch with any other problems, on any stream and for any check_every.  The workgroups of a finished problem return
 * at once.
 * The host queues iterations and reads one word every check_every >= 1 iterations (the count of
 * finished problems; a problem re-windows on the device); the call returns with the stream
 * synchronised.  There is no blind queue.
 * max_features and max_locals are the caller's statement; the device checks every cluster again.
 * problem_offset must rise from 0 to C, as for ctr_train: the device checks each problem's own
 * range, not that the ranges of different problems are disjoint; overlapping ranges are memory-safe
 * and give undefined results with a status of OK.
 * ctr_refine_global_plan (no device needed) gives the scratch bytes, the launches per iteration
 * (4), the 16-column tiles of a row (1 .. 3) and the doubles of a cluster's scratch row.
 * The descriptor is checked before the handle.  Device pointers. */
#define CTR_REFINE_GLOBAL_MAX_GLOBALS 8
#define CTR_REFINE_GLOBAL_MAX_COLUMNS 48
typedef struct ctr_refine_global {
  int32_t ndim;                    /* 2 or 3 */
  int32_t isotropic;               /* 1: one 'size' column; 0: one per axis */
  int32_t fit_function;            /* CTR_FIT_* */
  int32_t n_params;                /* as ctr_problem.n_params */
  int32_t modes[CTR_MAX_PARAMS];   /* CTR_MODE_* per column */
  int32_t radius[CTR_MAX_NDIM];    /* mask radius per axis, >= 1 */
  int32_t frame_dtype;             /* CTR_DTYPE_* */
  int32_t solver_maxiter;          /* 1 .. 10000: iterations of one round (default 100) */
  int32_t max_iter;                /* 1 .. 1000: window rounds (refine.py:365; default 10) */
  int32_t max_features;            /* features of the largest cluster, <= 64 */
  int32_t max_locals;              /* locals of the largest cluster; max_locals + G + 1 <= 48 */
  int32_t check_every;             /* >= 1: iterations between two looks at the finished count */
  int32_t reserved0;
  int64_t n_frames;
  int64_t shape[CTR_MAX_NDIM];     /* (z,) y, x */
  int64_t n_problems;              /* P */
  int64_t n_clusters;              /* C */
  int64_t n_features;              /* N */
  double residual_factor;          /* > 0 (default 1e5) */
  double max_rms_dev;              /* refine.py:391 (default 1) */
  double max_shift;                /* refine.py:384 (default 1) */
  double xtol;                     /* <= 0 -> 1e-9 */
  double ftol;                     /* <= 0 -> 1e-14 */
  const void* frames;              /* [n_frames, *shape] */
  const double* params;            /* [N, n_params] */
  const int32_t* feat_offset;      /* [C + 1] */
  const int32_t* frame_index;      /* [C] */
  const int32_t* problem_offset;   /* [P + 1] offsets into the clusters */
  const double* start;             /* [P, G] */
  const double* low;               /* [P, G], -inf = none */
  const double* high;              /* [P, G], +inf = none */
  const double* local_start;       /* [C, max_locals] */
  const double* local_low;
  const double* local_high;
  double* params_out;              /* [N, n_params] out */
  double* globals;                 /* [P, G] out */
  double* cost;                    /* [P] out */
  int32_t* status;                 /* [P] out */
  int32_t* n_rounds;               /* [P] out */
  int32_t* n_iter;                 /* [P] out */
} ctr_refine_global;
int ctr_refine_global_device(ctr_handle* h, const ctr_refine_global* d, void* hip_stream);
int ctr_refine_global_plan(const ctr_refine_global* d, int64_t* scratch_bytes, int32_t* launches_per_iteration,
                           int32_t* tiles, int64_t* row_doubles);

/* ---- cluster tracks: which particles form one cluster over time (ABI 8, additions) ----
 * The step between the linker and the motion stage: ctr_link_device / ctr_find_link_device give every
 * feature a `particle`, ctr_find_clusters labels the clusters of each frame, ctr_orientation_device
 * takes a dense block of tracked clusters.  The rule is this project's own (the reference's
 * orientation_df assumes one cluster per table, motion.py:146-162); tests/_cluster_tracks.py restates
 * it in NumPy / SciPy.
 * Input: N rows sorted by frame; frame_offset [T + 1] (0 <= off[t] <= off[t + 1] <= N, rows [off[t],
 * off[t + 1]) are frame t; a row in no frame is passed over); particle [N], dense ids 0 .. P - 1, a
 * negative id is an unlinked row; cluster [N], any integers: equal within a frame means the same
 * cluster, the values need not be unique across frames; pos [N, ndim]; cluster_size in {2, 3, 4};
 * min_frames >= 1.
 *   1. complete group: the rows of one frame with the same `cluster` value form a complete group when
 *      there are exactly cluster_size of them, all with particle >= 0 and pairwise different
 *      particles.  A group of any other size is no evidence (two dimers that touch in a frame form a
 *      group of four and bond nothing).
 *   2. bond: b(p, q) = the number of frames in which p and q share a complete group; p and q are
 *      bonded iff b(p, q) >= min_frames.
 *   3. track: the connected components of the bond graph with at least two particles, numbered
 *      0 .. n_tracks - 1 by ascending smallest particle id.  track_of_particle [P] is that number, -1
 *      for every other particle; n_members [n_tracks] the size of the component (it can exceed
 *      cluster_size where the linker lost a feature and gave it a new id: A-B, later A-B', is one
 *      track of three members).
 *   4. positions: for track k and frame t take the rows of frame t whose particle is a member of k,
 *      whatever their `cluster` value.  present [n_tracks, T] is their count.  Where it equals
 *      cluster_size, pos_out[k, t, j, :] is the position of the j-th of them in ascending order of
 *      (particle, row); anywhere else all of pos_out[k, t] is NaN.  present < cluster_size is an
 *      incomplete frame, present > cluster_size a conflict; nothing is chosen at random.
 * Integers and copies of doubles: the same bytes on every run and stream.
 *
 * ctr_cluster_tracks_device has two phases with the caller's sort between them:
 *   CTR_TRACKS_PAIRS: a kernel checks the tables (frame_offset as above, particle < P) before any
 *     other follows an index; a failed check gives status[0] = CTR_TRACKS_BAD_TABLE and no key.  One
 *     workgroup per frame: every row finds its group's size, whether it is complete and its rank by
 *     particle, and writes into keys[row (cluster_size - 1) ...] one key (lo << 32 | hi), lo < hi, per
 *     member of higher rank -- cluster_size (cluster_size - 1) / 2 per complete group -- and
 *     CTR_TRACKS_NO_KEY into every other slot.
 *   The caller sorts keys [N (cluster_size - 1)] ascending (any device sort; equal keys must be
 *     adjacent, nothing more is used).
 *   CTR_TRACKS_COMPONENTS: slot e is an edge where it starts a run of equal keys (keys[e - 1] differs),
 *     keys[e + min_frames - 1] == keys[e] and both ids are below P.  Components by hooking to the smaller label and pointer jumping: a round is one hook
 *     kernel (every edge between two trees hangs the root with the larger id under the smaller, by
 *     atomicMin, reading the labels of the round's start) and up to J = ceil(log2 P) + 1 jump kernels
 *     (label = label of label) that flatten every tree to a star.  A tree with an edge to another
 *     tree is merged with one within two rounds, so R = 2 ceil(log2 P) + 2 rounds suffice
 *     (ctr_cluster_tracks_plan gives R and J).  Kernel boundaries are the only synchronisation
 *     between workgroups; a kernel that has nothing left to do returns at its first load.
 *     check_every = 0: the R rounds are queued blind and the call is asynchronous; K > 0: the host
 *     reads one word every K rounds and stops queueing after a round that hooked nothing; the call
 *     then returns with the stream synchronised.  Same bytes.  A last kernel verifies that a further
 *     round would change nothing; if it would, status[0] = CTR_TRACKS_ROUNDS and no track is given.
 *     Then the roots with at least two members are numbered in ascending order (block counts, their
 *     scan, ranks) and track_of_particle, n_tracks, n_members and n_rounds (the rounds that hooked
 *     anything; may be null) are written.  status[0] is the PAIRS phase's and is not reset: a refused
 *     table gives n_tracks = 0 and -1 everywhere.
 * ctr_track_positions_device: a kernel checks the tables again (and track_of_particle < n_tracks);
 * status[0] = CTR_TRACKS_BAD_TABLE leaves present 0 and pos_out NaN.  present by one integer
 * atomicAdd per member row; pos_out by a NaN fill and a scatter by rank, one workgroup per frame.
 * n_tracks is the only number the host needs between the two calls.
 * Scratch of ctr_cluster_tracks_device belongs to the handle: calls of one handle are ordered on
 * the device whatever streams they are given.  Descriptors are checked before the handle, as for
 * ctr_characterize_device.  Device pointers; asynchronous on `hip_stream` unless check_every. */
#define CTR_TRACKS_PAIRS 0
#define CTR_TRACKS_COMPONENTS 1
#define CTR_TRACKS_OK 0
#define CTR_TRACKS_BAD_TABLE 1
#define CTR_TRACKS_ROUNDS 2
#define CTR_TRACKS_NO_KEY 0x7fffffffffffffffLL
typedef struct ctr_cluster_tracks {
  int32_t phase;                   /* CTR_TRACKS_PAIRS or CTR_TRACKS_COMPONENTS */
  int32_t cluster_size;            /* 2, 3 or 4 */
  int32_t check_every;             /* COMPONENTS: 0, or rounds between two looks at the hook word */
  int32_t reserved0;
  int64_t min_frames;              /* >= 1 */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  int64_t n_particles;             /* P <= 2^31 - 2 */
  const int64_t* frame_offset;     /* [T + 1]  (PAIRS) */
  const int64_t* particle;         /* [N]      (PAIRS) */
  const int64_t* cluster;          /* [N]      (PAIRS) */
  int64_t* keys;                   /* [N (cluster_size - 1)]: PAIRS out; COMPONENTS in, sorted */
  int32_t* track_of_particle;      /* [P] out          (COMPONENTS) */
  int32_t* n_tracks;               /* [1] out          (COMPONENTS) */
  int32_t* n_members;              /* [P / 2] out, the first n_tracks entries (COMPONENTS) */
  int32_t* status;                 /* [1]: PAIRS out; COMPONENTS in and out */
  int32_t* n_rounds;               /* [1] out or NULL  (COMPONENTS) */
} ctr_cluster_tracks;
int ctr_cluster_tracks_device(ctr_handle* h, const ctr_cluster_tracks* c, void* hip_stream);
/* No device needed: the scratch of the call, its round bound R and the jump kernels per round J. */
int ctr_cluster_tracks_plan(const ctr_cluster_tracks* c, int64_t* scratch_bytes, int32_t* max_rounds,
                            int32_t* jumps_per_round);

typedef struct ctr_track_positions {
  int32_t ndim;                    /* 2 or 3 */
  int32_t cluster_size;            /* 2, 3 or 4 */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  int64_t n_particles;             /* P */
  int64_t n_tracks;                /* n_tracks[0] of ctr_cluster_tracks_device */
  const int64_t* frame_offset;     /* [T + 1] */
  const int64_t* particle;         /* [N] */
  const int32_t* track_of_particle;/* [P] */
  const double* pos;               /* [N, ndim] */
  int32_t* present;                /* [n_tracks, T] out */
  double* pos_out;                 /* [n_tracks, T, cluster_size, ndim] out */
  int32_t* status;                 /* [1] out */
} ctr_track_positions;
int ctr_track_positions_device(ctr_handle* h, const ctr_track_positions* p, void* hip_stream);

/* ---- drift of a linked video: compute, subtract, drop stubs (ABI 8, additions) ----
 * The step between the linker and the cluster tracks / the motion stage: ctr_diffusion_device takes a
 * second moment, mean(x x^T) / (2 dt), not a covariance, so a common drift of v px per frame adds
 * v^2 lag^2 / (2 dt) to its translational entries.  The reference leaves the step to trackpy
 * (compute_drift, subtract_drift, filter_stubs on the linked table); the rule here is this project's
 * dense restatement of trackpy's published rule, tests/_drift.py restates it in NumPy.
 * Input: N rows sorted by frame; frame_offset [T + 1] (0 <= off[t] <= off[t + 1] <= N, rows [off[t],
 * off[t + 1]) are frame t); particle [N], dense ids 0 .. P - 1, a negative id is an unlinked row and
 * is ignored; pos [N, ndim], ndim 2 or 3.
 *   1. pairs: row i of frame t >= 1 and row j of frame t - 1 form a pair of frame t when
 *      particle[i] == particle[j] >= 0.  Where several rows of frame t - 1 carry that id, j is the
 *      lowest such row (the linker never makes such a table; the clause makes the result defined).
 *      Every row i of frame t that has a match counts.
 *   2. step: n_pairs[t] is the number of pairs of frame t, n_pairs[0] = 0; dx[t] the mean of
 *      pos[i] - pos[j] over the pairs of frame t.
 *   3. smoothing s >= 0: 0 and 1 mean none, sm[t] = dx[t] where n_pairs[t] > 0, else 0.  Otherwise
 *      sm[t] is the mean of dx[u] over the frames u in [max(1, t - s + 1), t] with n_pairs[u] > 0,
 *      and 0 where there is none.
 *   4. drift: drift[0] = 0, drift[t] = drift[t - 1] + sm[t].  Out: drift [T, ndim], n_pairs [T].
 *   5. subtraction: pos_out[i] = pos[i] - drift[frame of i], one subtraction per coordinate: NumPy's
 *      bytes for the same drift.  A row in no frame (before off[0], from off[T] on) is copied.
 *   6. stubs: count[p] is the number of rows with particle == p; a row whose particle has
 *      count < threshold gets particle -1.  No row is removed and no id renumbered, so the result
 *      goes into ctr_cluster_tracks_device and into 1, which ignore negative ids.  Out:
 *      particle_out [N], count [P], exact integers.
 * Against trackpy: its drift table has no row for the first frame nor for a frame without pairs, its
 * subtract_drift leaves the rows of such frames unshifted, and its rolling window counts table rows,
 * not frames.  Here the drift is carried forward through a frame without pairs and n_pairs says
 * which frames those are; on a table where every frame t >= 1 has a pair the values of the frames
 * t >= 1 are trackpy's.
 * A table is refused when frame_offset is not as above or a particle >= P: a kernel checks that
 * before any other follows an index, status[0] = CTR_DRIFT_BAD_TABLE, and then drift and pos_out
 * are NaN, n_pairs and count 0, particle_out -1.
 * Launches of ctr_drift_device: the check; one workgroup of 256 threads per frame t for 1 and 2 -- the
 * rows of frame t - 1 pass through LDS in tiles of 2048 rows, ascending, each an open-addressing
 * table of 4096 slots (particle << 32 | row, 32 KiB) in which a repeated particle keeps its lowest
 * row; a row of frame t without a match yet probes the tile, so the first tile that answers gives
 * the lowest row and a frame of any row count costs rows x tiles.  A thread adds the displacements
 * of its rows in ascending row order, the workgroup adds the threads' sums in a binary tree: no
 * float atomics, the same bytes on every run.  Then one workgroup for 3 and 4: sm[t] in ascending u,
 * the running sum per coordinate by a workgroup scan in chunks of 256 frames.  Scratch of the
 * handle: dx, 8 ndim T bytes.  ctr_drift_subtract_device: the check, then one grid-stride kernel
 * over the rows, the frame of a row by bisection of frame_offset; pos_out may be pos.
 * ctr_filter_stubs_device: the check, an int32 histogram by atomicAdd, an apply pass; particle_out
 * may be particle.  Descriptors are checked before the handle, as for ctr_characterize_device.
 * Device pointers; asynchronous on `hip_stream`. */
#define CTR_DRIFT_OK 0
#define CTR_DRIFT_BAD_TABLE 1
typedef struct ctr_drift {
  int32_t ndim;                    /* 2 or 3 */
  int32_t smoothing;               /* s >= 0 */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  int64_t n_particles;             /* P <= 2^31 - 2 */
  const double* pos;               /* [N, ndim] */
  const int64_t* frame_offset;     /* [T + 1] */
  const int64_t* particle;         /* [N] */
  double* drift;                   /* [T, ndim] out */
  int32_t* n_pairs;                /* [T] out */
  int32_t* status;                 /* [1] out */
} ctr_drift;
int ctr_drift_device(ctr_handle* h, const ctr_drift* d, void* hip_stream);

typedef struct ctr_drift_subtract {
  int32_t ndim;                    /* 2 or 3 */
  int32_t reserved0;
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  const double* pos;               /* [N, ndim] */
  const int64_t* frame_offset;     /* [T + 1] */
  const double* drift;             /* [T, ndim] */
  double* pos_out;                 /* [N, ndim] out; may be pos */
  int32_t* status;                 /* [1] out */
} ctr_drift_subtract;
int ctr_drift_subtract_device(ctr_handle* h, const ctr_drift_subtract* d, void* hip_stream);

typedef struct ctr_filter_stubs {
  int64_t threshold;               /* >= 1 */
  int64_t n_features;              /* N */
  int64_t n_particles;             /* P <= 2^31 - 2 */
  const int64_t* particle;         /* [N] */
  int64_t* particle_out;           /* [N] out; may be particle */
  int32_t* count;                  /* [P] out */
  int32_t* status;                 /* [1] out */
} ctr_filter_stubs;
int ctr_filter_stubs_device(ctr_handle* h, const ctr_filter_stubs* d, void* hip_stream);

/* ---- mean squared displacement of linked particles (ABI 8, additions) ----
 * The squared displacement of a linked table against lag time, of every particle and of the
 * ensemble: what the reference's users compute with trackpy (msd, imsd, emsd) before they trust a
 * diffusion tensor; it calibrates D, it shows a residual drift v as |v|^2 k^2 at lag k, and it tells
 * stuck particles from free ones.  The rule is this project's dense restatement of trackpy's
 * published rule with gaps; tests/_msd.py restates it with plain loops.
 * Input: the tables of the drift calls above -- N rows sorted by frame, frame_offset [T + 1], particle
 * [N] with dense ids 0 .. P - 1 and negative = unlinked, pos [N, ndim], ndim 2 or 3 -- and
 * max_lagtime L >= 1 (the lags k = 1 .. L, in frames), mpp per axis.  A row before off[0] or from
 * off[T] on is in no frame and does not exist for this rule.
 *   1. of several rows of one frame with the same id >= 0 only the lowest row exists (clause 1 of the
 *      drift rule);
 *   2. rows i (frame t) and j (frame t + k) with particle[i] == particle[j] == p >= 0 are a pair of
 *      (p, k); a frame in between that p misses makes no difference;
 *   3. d = (pos[j] - pos[i]) * mpp, per coordinate: the subtraction first;
 *   4. n[p, k] is the number of pairs of (p, k);
 *   5. mean_d[p, k, a] is the mean of d_a over them;
 *   6. mean_d2[p, k, a] is the mean of d_a^2, the square rounded before it is added;
 *   7. msd[p, k] = mean_d2[p, k, 0] + mean_d2[p, k, 1] (+ mean_d2[p, k, 2]), added in that order;
 *   8. lagt[k] = k / fps (the Python layer's: the device works in frames);
 *   9. where n == 0 the means and msd are NaN: k beyond the track's span, a particle with one row,
 *      an id without rows;
 *  10. ensemble: the same four quantities over the pairs of all particles pooled (trackpy's emsd:
 *      the mean of the per-particle values weighted by n); its n[k] is int64.
 * Against trackpy: its msd reindexes a track by frame and takes NaN where a frame is missing, which
 * is clause 2; its imsd returns msd alone and drops nothing else; its emsd pools with the weights n
 * as clause 10 does.  trackpy's 'N' column of msd is an effective number of independent
 * measurements, not a pair count; n here is the pair count.  Clause 1 has no counterpart (the
 * linker never makes such a table; the clause makes the result defined).
 * `order` [N] is the caller's stable ascending sort of the rows by particle (torch's or any other):
 * rows are in frame order, so that is (particle, frame, row) order.  A table is refused
 * (status[0] = CTR_MSD_BAD_TABLE; then the means and msd are NaN and every n is 0, and no kernel
 * follows an index of the table) when frame_offset is not monotone within [0, N], a particle >= P,
 * or `order` is not that sort (an entry outside [0, N), ids not ascending, rows of an id not
 * ascending).  `select`: the M ids to report, or null for 0 .. M - 1; an id outside [0, P) is an id
 * without rows.
 * Launches, 256 threads each.  The check.  msd_rows: one thread per sorted row -- the frame of the
 * row by bisection of frame_offset, into a code (the frame, or a negative word for a row that does
 * not exist: repeated, or in no frame), the positions gathered into sorted order, and the first and
 * last sorted row of every id where the id changes: no histogram and no scan.
 * ctr_msd_device then runs msd_particle, one workgroup per reported id: a track whose span (last -
 * first + 1 frames) is at most CTR_MSD_TILE = 2048 is staged in LDS dense by frame, coordinates
 * and a presence byte, and for lag k a thread visits frames f, f + 256, ... and adds where f and
 * f + k are both present; a longer span is read from the sorted rows in global memory, where the
 * partner of row i at lag k is row i + k when the track has no gap there and else is found by
 * bisection of the codes.  No track is refused for its length.  A thread adds its terms in frame
 * order; the workgroup adds the threads' sums in a fixed tree (shuffles in the wavefront, then the
 * four wavefronts): no float atomics, the same bytes on every call; lags beyond the span are
 * written without a reduction.  ctr_emsd_device runs msd_chunk, one workgroup per CTR_MSD_CHUNK =
 * 256 consecutive ids: their rows are consecutive sorted rows, which it walks as the long-span
 * path does, and writes one partial (sums and a count per lag) per chunk; then msd_pool adds the
 * partials in chunk order.  The chunk is a constant, not a function of the grid; where the chunks
 * are few the launch lets several workgroups share the lags of a chunk, each lag still summed by
 * one workgroup in the same order, so the bytes do not depend on that either.  Scratch of the
 * handle: 4 N (codes) + 4 N (ids) + 8 ndim N (positions) + 8 P (row ranges) bytes, and for the
 * ensemble 8 (2 ndim + 1) L ceil(P / 256) more; nothing proportional to P L.
 * Descriptors are checked before the handle.  Device pointers; asynchronous on `hip_stream`. */
#define CTR_MSD_OK 0
#define CTR_MSD_BAD_TABLE 1
#define CTR_MSD_TILE 2048            /* frames of a track's span that msd_particle stages in LDS */
#define CTR_MSD_CHUNK 256            /* particle ids per partial of the ensemble */
typedef struct ctr_msd {
  int32_t ndim;                    /* 2 or 3 */
  int32_t reserved0;
  int64_t max_lagtime;             /* L >= 1 */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  int64_t n_particles;             /* P <= 2^31 - 2 */
  int64_t n_select;                /* M: the ids reported */
  double mpp[CTR_MAX_NDIM];        /* per axis, finite */
  const double* pos;               /* [N, ndim] */
  const int64_t* frame_offset;     /* [T + 1] */
  const int64_t* particle;         /* [N] */
  const int64_t* order;            /* [N]: the rows in a stable ascending sort by particle */
  const int64_t* select;           /* [M] ids, or null: 0 .. M - 1 */
  double* msd;                     /* [M, L] out */
  double* mean_d;                  /* [M, L, ndim] out */
  double* mean_d2;                 /* [M, L, ndim] out */
  int32_t* n;                      /* [M, L] out */
  int32_t* status;                 /* [1] out */
} ctr_msd;
int ctr_msd_device(ctr_handle* h, const ctr_msd* d, void* hip_stream);

typedef struct ctr_emsd {
  int32_t ndim;                    /* 2 or 3 */
  int32_t reserved0;
  int64_t max_lagtime;             /* L >= 1 */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  int64_t n_particles;             /* P <= 2^31 - 2 */
  double mpp[CTR_MAX_NDIM];        /* per axis, finite */
  const double* pos;               /* [N, ndim] */
  const int64_t* frame_offset;     /* [T + 1] */
  const int64_t* particle;         /* [N] */
  const int64_t* order;            /* [N]: as in ctr_msd */
  double* msd;                     /* [L] out */
  double* mean_d;                  /* [L, ndim] out */
  double* mean_d2;                 /* [L, ndim] out */
  int64_t* n;                      /* [L] out */
  int32_t* status;                 /* [1] out */
} ctr_emsd;
int ctr_emsd_device(ctr_handle* h, const ctr_emsd* d, void* hip_stream);

/* ---- van Hove displacement distributions of linked particles (ABI 8, an addition) ----
 * The histogram of the displacements at a lag, per coordinate and radial, pooled over all
 * particles: what the reference's users take from trackpy's motion.vanhove to see whether the
 * displacements are Gaussian, which every diffusion coefficient of this library assumes (the D of
 * the ensemble's MSD, the tensor of ctr_diffusion_device).  Stuck particles and wrong links put
 * weight in the tails, a residual drift shifts the centre, clusters near a wall give heavy tails
 * long before the MSD bends.  The rule is this project's own dense rule; tests/_vanhove.py restates
 * it with plain loops.  Input: the tables of the MSD calls above, `order` included, and K lags.
 *   1. - 3. are clauses 1 to 3 of the MSD rule, unchanged: of several rows of one frame with the same
 *      id >= 0 only the lowest exists; rows i (frame t) and j (frame t + k) of one id >= 0 are a pair
 *      of lag k whatever is missing in between; d_a = (pos[j, a] - pos[i, a]) * mpp_a, one
 *      subtraction and one product: the same double as there;
 *   4. lags: lag[0 .. K - 1], ascending distinct integers >= 1 and <= 2^31 - 3, 1 <= K <=
 *      CTR_VANHOVE_MAX_LAGS = 64; host values, inline in the descriptor, checked by the launch;
 *   5. bins per coordinate: H = half_bins = ceil(max_disp / bin_width), 1 <= H <=
 *      CTR_VANHOVE_MAX_HALF_BINS = 1024, B = 2 H bins; edges[b] = (b - H) * bin_width for b = 0 .. 2 H,
 *      computed by the caller in float64 with one rounding each (so they are symmetric and edges[H]
 *      is 0.0) and handed over; d_a is in bin b iff edges[b] <= d_a < edges[b + 1]; d_a < edges[0]
 *      counts in below[k, a], d_a >= edges[2 H] in above[k, a]; a NaN compares false everywhere: it is
 *      in no bin and in neither tail.  The device guesses the bin by a product with 1 / bin_width;
 *      the comparison with the edges decides;
 *   6. radial bins: r_edges[b] = b * bin_width for b = 0 .. H, edge2 = r_edges * r_edges (the
 *      caller's, handed over); d2 is the sum over the axes, in axis order, of d_a * d_a, every product
 *      and every sum rounded on its own; the pair is in radial bin b iff edge2[b] <= d2 < edge2[b + 1];
 *      d2 >= edge2[H] counts in above_r[k]; a NaN d2 nowhere;
 *   7. counts: n[k] is the number of pairs of lag k over all ids; count[k, a, b], below, above,
 *      count_r and above_r are int64 and exact.  On finite positions count[k, a].sum() + below[k, a]
 *      + above[k, a] == n[k] for every a, and count_r[k].sum() + above_r[k] == n[k];
 *   8. moments: mean_d[k, a], mean_d2[k, a], mean_d4[k, a] are the means over the pairs of d_a, of
 *      rn(d_a d_a) and of rn(rn(d_a^2) rn(d_a^2)).  They are summed as the ensemble's MSD sums: per
 *      chunk of CTR_MSD_CHUNK consecutive ids, the chunk's sorted rows strided over the workgroup of
 *      256, the wavefront's tree, (0 + 1) + (2 + 3) over the wavefronts, then the chunks in chunk
 *      order.  A thread adds a term of d and of d^2 to its running sum as msd_chunk_kernel is compiled
 *      to add it, the product and the addition in one fused operation (fma(mpp, diff, sum), fma(d,
 *      d, sum): one rounding where the plain sum has two); d^4 is rounded, then added.  So mean_d and
 *      mean_d2 are bit for bit those of ctr_emsd_device at the same lag;
 *   9. alpha2[k, a] = mean_d4 / (3 * (mean_d2 * mean_d2)) - 1, every operation rounded on its own:
 *      the one-dimensional non-Gaussian parameter, 0 for a Gaussian, -2/3 for a single value;
 *  10. density[k, a, b] = count / (n[k] * bin_width); density_r[k, b] = count_r / (n[k] * bin_width),
 *      per unit r, not divided by the shell.  Where n[k] == 0 (a lag beyond every span, an empty
 *      table, unlinked rows only) the densities, the means and alpha2 are NaN and the counts 0;
 *  11. a refused table (status[0] = CTR_VANHOVE_BAD_TABLE: what ctr_emsd_device refuses): the
 *      floats NaN, the counts and n 0, and no kernel follows an index of the table.
 * Against trackpy's vanhove: bins are given by a width and a reach, not by a count over the data's
 * range; the tails are counted rather than dropped; the ensemble only (a histogram per particle is
 * P B numbers); all coordinates and the radial part in one call; several lags in one call.
 * Launches, 256 threads each.  The check and the sorted rows of the MSD calls; vanhove_clear zeroes
 * the int64 tables; vanhove_bin, one workgroup per (chunk, lag): uint32 counters in LDS, ndim (2 H +
 * 2) + H + 1 of them (a chunk has fewer than 2^31 rows), integer LDS atomics, the moments in
 * registers; one partial per (chunk, lag) and the non-zero counters added to the int64 tables with
 * integer atomics: any order gives the same bytes; vanhove_finish, one workgroup per lag: the
 * partials in chunk order, clauses 8 to 10.  No float atomics.  Scratch of the handle (the block of
 * the MSD calls): the sorted rows as there and 8 (3 ndim + 1) K ceil(P / 256) bytes of partials.
 * Descriptors are checked before the handle.  Device pointers; asynchronous on `hip_stream`. */
#define CTR_VANHOVE_OK 0
#define CTR_VANHOVE_BAD_TABLE 1
#define CTR_VANHOVE_MAX_LAGS 64
#define CTR_VANHOVE_MAX_HALF_BINS 1024
typedef struct ctr_vanhove {
  int32_t ndim;                    /* 2 or 3 */
  int32_t n_lags;                  /* K, 1 .. CTR_VANHOVE_MAX_LAGS */
  int64_t half_bins;               /* H, 1 .. CTR_VANHOVE_MAX_HALF_BINS */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  int64_t n_particles;             /* P <= 2^31 - 2 */
  double bin_width;                /* finite, > 0 */
  double mpp[CTR_MAX_NDIM];        /* per axis, finite */
  int64_t lag[CTR_VANHOVE_MAX_LAGS];   /* the first K: ascending, >= 1, <= 2^31 - 3 */
  const double* pos;               /* [N, ndim] */
  const int64_t* frame_offset;     /* [T + 1] */
  const int64_t* particle;         /* [N] */
  const int64_t* order;            /* [N]: as in ctr_msd */
  const double* edges;             /* [2 H + 1]: clause 5 */
  const double* edge2;             /* [H + 1]: clause 6 */
  int64_t* count;                  /* [K, ndim, 2 H] out */
  int64_t* below;                  /* [K, ndim] out */
  int64_t* above;                  /* [K, ndim] out */
  double* density;                 /* [K, ndim, 2 H] out */
  int64_t* count_r;                /* [K, H] out */
  int64_t* above_r;                /* [K] out */
  double* density_r;               /* [K, H] out */
  int64_t* n;                      /* [K] out */
  double* mean_d;                  /* [K, ndim] out */
  double* mean_d2;                 /* [K, ndim] out */
  double* mean_d4;                 /* [K, ndim] out */
  double* alpha2;                  /* [K, ndim] out */
  int32_t* status;                 /* [1] out */
} ctr_vanhove;
int ctr_vanhove_device(ctr_handle* h, const ctr_vanhove* d, void* hip_stream);

/* ---- pair correlation function g(r) of a feature table (ABI 8, additions) ----
 * The structure of a frame, where the calls above describe dynamics: the bond length inside a
 * cluster is the first peak of g(r) over the pairs of one cluster, `separation` is the gap behind
 * it, and crowding is g(r) between clusters.  The reference's users take it from trackpy
 * (static.pair_correlation_2d / _3d), one kd-tree query per particle and frame; this is an all-pairs
 * distance histogram per frame and an edge correction per reference row.  The rule is the project's
 * own dense rule; tests/_pair_correlation.py restates it in NumPy.  Parity with trackpy is not
 * pinned; it differs in: a ratio estimator (the pooled g is a ratio of sums over the frames, not a
 * mean of per-particle ratios), the radius of the correction (the middle of the bin), one box for all
 * frames, coincident rows counted, and a result per frame.
 * Input: pos [N, ndim], ndim 2 or 3, rows sorted by frame; frame_offset [T + 1]; group [N] or null;
 * B bins of width dr; mpp per axis, > 0; box [2, ndim] (lo, then hi) in scaled units; edge2 [B + 1]
 * and shell [B], which the host computes once (clause 1) so that the kernel and the yardstick
 * compare with the same doubles.
 *   1. Bins.  B = ceil(cutoff / dr) (the Python layer's); r_edges[b] = b * dr for b = 0 .. B;
 *      edge2 = r_edges * r_edges; shell[b] = pi * (edge2[b + 1] - edge2[b]) for ndim 2 and
 *      4/3 * pi * (r_edges[b + 1]^3 - r_edges[b]^3) for ndim 3.
 *   2. Scaling.  q = pos * mpp per axis, one rounding; everything below is in these units.
 *   3. Box.  `boundary` of the Python layer, [[lo...], [hi...]] in pixels, times mpp; by default the
 *      minimum and the maximum of q over all rows of the call, NaN ignored (+inf and -inf where there
 *      is none): one box for all frames.  V = the product over the axes, in axis order, of hi_a - lo_a.
 *   4. A row exists when every coordinate is finite and within [lo_a, hi_a].  n_rows[t] counts the
 *      existing rows of frame t; rho_t = (n_rows[t] - 1) / V.
 *   5. Reference rows.  CTR_PCF_EDGE_NONE and _ARC: every existing row.  _INTERIOR: the existing
 *      rows with q_a - lo_a >= r_edges[B] and hi_a - q_a >= r_edges[B] on every axis.  n_ref[t]
 *      counts them.
 *   6. Pairs.  A reference row i and an existing row j != i of the same frame are a pair, ordered:
 *      two reference rows count each other.  CTR_PCF_PAIRS_SAME: also group[i] == group[j] >= 0;
 *      _OTHER: the pairs that fail that; so count_all == count_same + count_other in every bin.
 *   7. Binning.  d2 = the sum over the axes, in axis order, of (q_j - q_i)_a squared, every
 *      product and sum rounded on its own.  The pair falls in bin b iff edge2[b] <= d2 < edge2[b + 1];
 *      with d2 >= edge2[B] in none; coincident distinct rows (d2 == 0) in bin 0.  count[t, b], int64.
 *   8. Weight.  weight[t, b] = the sum over the reference rows of frame t, in row order, of phi_i(b).
 *      _NONE and _INTERIOR: phi = 1, weight[t, b] = n_ref[t].  _ARC (ndim 2): phi_i(b) is the
 *      fraction of the circle of radius R = r_edges[b] + dr / 2 around row i that lies inside the
 *      box: the quadrant angles of the four quadrants -- wall distance a along axis 0 in (hi_0 - q_0,
 *      q_0 - lo_0), b' along axis 1 in (hi_1 - q_1, q_1 - lo_1), added in the order (a, b') = (first,
 *      first), (first, second), (second, first), (second, second) -- divided by 2 pi.  The quadrant
 *      angle is pi / 2 when a >= R and b' >= R and max(0, asin(min(b' / R, 1)) - acos(min(a / R, 1)))
 *      otherwise.  A row further than R from every wall gets exactly 1.0 without trigonometry.
 *   9. g_frame[t, b] = count[t, b] / ((rho_t * shell[b]) * weight[t, b]); NaN where the denominator
 *      is not positive and finite: an empty or one-row frame, a degenerate box (V = 0 makes it
 *      infinite), no reference row.
 *  10. g[b] = the sum of count[t, b] over t divided by the sum over t, in frame order, of the
 *      positive finite denominators of clause 9; NaN where no frame has one.
 * A frame_offset that is not monotone within [0, N] is refused: status[0] = CTR_PCF_BAD_TABLE, g,
 * g_frame and weight NaN, count, n_ref and n_rows 0, and no kernel follows an offset.
 * Launches, 256 threads each.  pcf_check.  pcf_frames, one workgroup per frame: n_rows, n_ref, the
 * counts zeroed.  pcf_items, one workgroup: the exclusive scan of ceil(rows / 256) over the frames.
 * pcf_pairs: a work item is a frame and a tile of 256 of its rows; their number is known on the
 * device alone, so T + N / 256 workgroups (its upper bound) are launched, each finds its item in the
 * scan by bisection and the surplus leaves.  A thread keeps its reference row in registers and walks
 * the frame's rows, staged 256 at a time in LDS with their group ids; the bin is guessed from
 * sqrt(d2) / dr and corrected against edge2 (in LDS); the workgroup's histogram, 32-bit LDS atomics,
 * is added to count[t, :] with 64-bit atomics.  _ARC: one thread per bin then walks the tile's
 * reference rows in row order and writes the partial weight of the work item to scratch.
 * pcf_finish, one thread per (t, b): the frame's partials added in item order, g_frame.  pcf_pool,
 * one thread per bin walking the frames in order: g.  Sums of doubles in a fixed order, integer
 * atomics only: the same bytes on every call.  (_ARC: weight is the sum of the tiles' sums, each in
 * row order.)  All pairs of a frame are visited; there is no cell list.
 * Scratch of the handle: 8 (T + 1) bytes and for _ARC 8 B (T + N / 256) more.
 * Descriptors are checked before the handle.  Device pointers; asynchronous on `hip_stream`. */
#define CTR_PCF_OK 0
#define CTR_PCF_BAD_TABLE 1
#define CTR_PCF_MAX_BINS 2048        /* edge2 and the histogram of a workgroup are in LDS */
#define CTR_PCF_EDGE_NONE 0
#define CTR_PCF_EDGE_INTERIOR 1
#define CTR_PCF_EDGE_ARC 2
#define CTR_PCF_PAIRS_ALL 0
#define CTR_PCF_PAIRS_SAME 1
#define CTR_PCF_PAIRS_OTHER 2
typedef struct ctr_pair_correlation {
  int32_t ndim;                    /* 2 or 3 */
  int32_t edge;                    /* CTR_PCF_EDGE_*; _ARC with ndim 2 only */
  int32_t pairs;                   /* CTR_PCF_PAIRS_* */
  int32_t reserved0;
  int64_t n_bins;                  /* B, 1 .. CTR_PCF_MAX_BINS */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  double dr;                       /* > 0 */
  double mpp[CTR_MAX_NDIM];        /* per axis, > 0 */
  const double* pos;               /* [N, ndim] */
  const int64_t* frame_offset;     /* [T + 1] */
  const int64_t* group;            /* [N], or null with CTR_PCF_PAIRS_ALL */
  const double* box;               /* [2, ndim]: lo, hi */
  const double* edge2;             /* [B + 1] */
  const double* shell;             /* [B] */
  double* g;                       /* [B] out */
  double* g_frame;                 /* [T, B] out */
  int64_t* count;                  /* [T, B] out */
  double* weight;                  /* [T, B] out */
  int64_t* n_ref;                  /* [T] out */
  int64_t* n_rows;                 /* [T] out */
  int32_t* status;                 /* [1] out */
} ctr_pair_correlation;
int ctr_pair_correlation_device(ctr_handle* h, const ctr_pair_correlation* d, void* hip_stream);

/* ---- nearest neighbours and proximity of a feature table (ABI 8, additions) ----
 * The structure per feature, where g(r) above is pooled: how far every row is from its nearest
 * rows, which rows those are, and how many rows lie within a distance.  Within a frame (lag 0) it
 * is the upper bound of `search_range`, the coordination number and, over the rows of one group,
 * the bond length; from frame t into frame t + 1 (lag 1) the displacement that `search_range` must
 * exceed; to the rows of other groups the filter that keeps cluster_tracks and motion to free
 * clusters.  The reference's users take it from trackpy (static.proximity) and a cKDTree per frame;
 * this visits all rows of the candidate frame.  The rule is the project's own dense rule;
 * tests/_neighbors.py restates it in NumPy.  Parity with trackpy is not pinned.
 * Input: pos [N, ndim], ndim 2 or 3, rows sorted by frame; frame_offset [T + 1]; group [N] or null;
 * particle [N] or null; k in 1 .. CTR_NBR_MAX_K; lag >= 0; mpp per axis, > 0; limit2 > 0 or +inf.
 *   1. Scaling.  q = pos * mpp per axis, one rounding; everything below is in these units.
 *   2. A row exists when every coordinate of q is finite.  There is no box.
 *   3. Candidates.  The candidates of row i of frame t are the existing rows j of frame t + lag;
 *      with lag == 0, j == i is excluded; a row of a frame with t + lag >= T has no candidate.
 *      CTR_PCF_PAIRS_SAME: also group[i] == group[j] >= 0; _OTHER: the candidates that fail that.
 *   4. Distance.  d2 = the sum over the axes, in axis order, of (q_j - q_i)_a squared, every
 *      product and sum rounded on its own.  A candidate qualifies when d2 < limit2, strictly;
 *      limit2 = max_dist * max_dist, which the host computes once, or +inf without a max_dist.
 *   5. count[i] = the number of qualifying candidates: exact, int64.
 *   6. Neighbours.  The qualifying candidates sorted by (d2, j) ascending; the first k are the
 *      neighbours: dist2[i, m] their d2, index[i, m] their global row j, dist[i, m] =
 *      sqrt(dist2[i, m]).  Coincident rows (d2 == 0) are neighbours like any other.  Where fewer
 *      than k qualify the remaining entries are NaN, NaN and -1.
 *   7. Rows with no result: a row that does not exist, a row of a frame without a candidate frame
 *      and a row outside [frame_offset[0], frame_offset[T]) get NaN, -1 and count 0, and are
 *      nobody's neighbour.
 *   8. Per particle (n_particles = P > 0).  particle_min2[p] = the minimum of dist2[i, 0] over the
 *      rows with particle[i] == p that have a neighbour; particle_min[p] its square root; NaN where
 *      there is none.  Rows with an id outside [0, P) contribute nowhere.
 *   9. A refused table.  A frame_offset that is not monotone within [0, N] is refused: status[0] =
 *      CTR_NBR_BAD_TABLE, every float output NaN, index -1, count 0, and no kernel follows an
 *      offset before nbr_check has passed it.
 * Launches, 256 threads each.  nbr_check.  nbr_defaults: the outputs of a refused table and of the
 * rows outside the frames, and the per-particle keys.  nbr_items, one workgroup: the exclusive scan
 * of ceil(rows / 256) over the frames.  nbr_pairs: a work item is a frame and a tile of 256 of its
 * rows, T + N / 256 workgroups of which the surplus leaves; a thread owns one row and every output
 * element of it, keeps the row and its best (d2, j) in registers -- a sorted list of compile-time
 * capacity 1, 4 or 16, the smallest that holds k, as an unrolled compare-and-shift chain -- and walks
 * the candidate frame's rows, staged 256 at a time in LDS with their group ids.  Candidates arrive
 * in ascending j and enter only on a strict d2 < kept, behind equal entries: the (d2, j) order
 * without a comparison of indices.  nbr_particles: the per-particle minimum, taken by nbr_pairs with
 * 64-bit integer atomics on the ordered key of the non-negative double, and its square root.  No
 * float atomic and no sum of doubles whose order could matter: the same bytes on every call.
 * Scratch of the handle: 8 (T + 1) bytes and 8 P for the keys.
 * Descriptors are checked before the handle.  Device pointers; asynchronous on `hip_stream`. */
#define CTR_NBR_OK 0
#define CTR_NBR_BAD_TABLE 1
#define CTR_NBR_MAX_K 16             /* the largest list a thread keeps in registers */
typedef struct ctr_neighbors {
  int32_t ndim;                    /* 2 or 3 */
  int32_t pairs;                   /* CTR_PCF_PAIRS_* */
  int32_t k;                       /* 1 .. CTR_NBR_MAX_K */
  int32_t lag;                     /* >= 0: the candidates of frame t are in frame t + lag */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  int64_t n_particles;             /* P, 0: no per-particle result */
  double limit2;                   /* > 0 or +inf */
  double mpp[CTR_MAX_NDIM];        /* per axis, > 0 */
  const double* pos;               /* [N, ndim] */
  const int64_t* frame_offset;     /* [T + 1] */
  const int64_t* group;            /* [N], or null with CTR_PCF_PAIRS_ALL */
  const int64_t* particle;         /* [N], with P > 0 */
  double* dist;                    /* [N, k] out */
  double* dist2;                   /* [N, k] out */
  int64_t* index;                  /* [N, k] out */
  int64_t* count;                  /* [N] out */
  double* particle_min;            /* [P] out, with P > 0 */
  double* particle_min2;           /* [P] out, with P > 0 */
  int32_t* status;                 /* [1] out */
} ctr_neighbors;
int ctr_neighbors_device(ctr_handle* h, const ctr_neighbors* d, void* hip_stream);

/* ---- two-point displacement correlations of linked particles (ABI 8, additions) ----
 * Whether particles move together, as a function of their separation: the mean over the pairs of a
 * frame, binned by distance, of the product of their displacements over a lag -- its trace (dot), its
 * part along the line between the two (longitudinal, D_rr of two-point microrheology), its part across
 * that line (transverse) and the cosine of the angle between the two displacements.  Where the
 * reference's users take trackpy's motion.velocity_corr / direction_corr; g(r) and the neighbours above
 * say how close rows come, this says whether their motion is coupled.  A residual drift shows as a
 * constant |v|^2 lag^2 at every r, wrong links in the first bins.  The rule is the project's own
 * dense rule; tests/_twopoint.py restates it in NumPy.  Parity with trackpy is not pinned; it differs
 * in: bins and a pool over all frames, ordered pairs, any lag, and max_disp.
 * Input: pos [N, ndim], ndim 2 or 3, rows sorted by frame; frame_offset [T + 1]; particle [N], ids
 * below P, negative = unlinked; group [N] or null; K lags; B bins of width dr; mpp per axis, > 0;
 * edge2 [B + 1] and max2, which the host computes once.
 *   1. Bins.  Clause 1 of g(r): B = ceil(cutoff / dr), at most CTR_TP_MAX_BINS; r_edges[b] = b * dr;
 *      edge2 = r_edges * r_edges, computed on the host.
 *   2. Scaling and existence.  q = pos * mpp per axis, one rounding.  A row exists when every
 *      coordinate of q is finite.  There is no box.
 *   3. Lags.  An ascending list of distinct integers >= 1, at most CTR_TP_MAX_LAGS of them.
 *   4. Partner.  The partner of row i of frame t at lag k is the lowest row j of frame t + k with
 *      particle[j] == particle[i] >= 0; there is none when t + k >= T or particle[i] < 0: drift's rule
 *      for a repeated particle.
 *   5. Displacement.  u_a = q_partner,a - q_i,a; u2 = the sum over the axes, in axis order, of u_a *
 *      u_a, every product and sum rounded on its own.  Row i has moved at lag k when it exists, its
 *      partner exists and u2 <= max2; max2 = max_disp * max_disp, computed once on the host.
 *      n_moved[k] counts the moved rows, beyond[k] the rows with a finite u and u2 > max2.  Rows
 *      outside [frame_offset[0], frame_offset[T]) take no part.
 *   6. Pairs.  A pair is an ordered pair (i, j), j != i, of rows of one frame that have both moved at
 *      lag k, with 0 < d2 < edge2[B]; d2 and the bin as in clause 7 of g(r): edge2[b] <= d2 <
 *      edge2[b + 1].  Coincident rows are not pairs, because L below divides by d2.
 *      CTR_PCF_PAIRS_SAME / _OTHER with group as in clause 6 of g(r).
 *   7. Per pair, every product and sum rounded on its own: R_a = q_j,a - q_i,a, the differences that
 *      d2 squares; dot = the sum over the axes, in axis order, of u_i,a * u_j,a; a_i = that sum of
 *      u_i,a * R_a and a_j = of u_j,a * R_a; L = (a_i * a_j) / d2; c = dot / sqrt(u2_i * u2_j) where
 *      that product is > 0, else 0.
 *   8. Fixed point.  e = the smallest integer with 2^e >= max2; unit = 2^(e - 40) and unit_cos =
 *      2^-40.  A value x enters as the integer rint(x / unit), ties to even; the scaling is exact.
 *   9. Sums.  n[k, b] counts the pairs, exact int64.  sums[k, b, s], s = dot, L, c, are the exact
 *      integer sums, each a 128-bit two's-complement number in two int64 words (hi, lo).  Integer
 *      addition commutes: the order of the pairs cannot matter, and there is no float sum at all.
 *  10. Means.  A sum that fits int64 (hi is the sign extension of lo) is converted from that int64
 *      with one rounding; a larger one is (double)hi * 2^64 + (double)(uint64)lo.  Then dot[k, b] =
 *      (x * unit) / (double)n, and likewise longitudinal (from the L sum) and cos (with unit_cos).
 *      transverse comes from the exact integer difference S_dot - S_L the same way, divided also by
 *      ndim - 1: ((x * unit) / (double)n) / (double)(ndim - 1), the mean per transverse axis.  NaN
 *      where n == 0.
 *  11. A refused table.  A frame_offset that does not rise within [0, N] or a particle[i] >= P is
 *      refused: status[0] = CTR_TP_BAD_TABLE, float outputs NaN, integers 0, and no kernel follows an
 *      index of a refused table.
 * Consequences: (i, j) and (j, i) give the same three integers (a_i and a_j swap and change sign
 * exactly), so n and every sum are even; S_all == S_same + S_other as integers.
 * Launches, 256 threads each.  twopt_check.  twopt_defaults zeroes the integer outputs.
 * twopt_partner, one workgroup per (lag, frame), striding: the partner's row of every moved row, or
 * -1, into scratch, 4 bytes per row and lag; the rows of frame t + k go through an LDS open-addressing
 * table in tiles of 2048, lowest row kept (drift's); n_moved and beyond by integer atomics.
 * twopt_items: the exclusive scan of ceil(rows / 256) over the frames.  twopt_pairs, one workgroup
 * per (lag, frame, tile of 256 rows), striding: a thread keeps q, u and u2 of its row in registers
 * and walks the frame's rows, staged 256 at a time in LDS with their u and u2 (the walk of g(r));
 * 32-bit counts and 64-bit sums per bin in LDS, added to the global (hi, lo) words at the end of a
 * work item and every 32 tiles (|integer| <= 2^41 per pair, 2^16 pairs per tile: below 2^62); the
 * carry into hi is the old low word against the new one, plus the sign extension.  twopt_finish, one
 * thread per (k, b): clause 10.  Integer atomics only: the same bytes on every call.
 * Scratch of the handle: 8 (T + 1) + 4 K N bytes.
 * Descriptors are checked before the handle.  Device pointers; asynchronous on `hip_stream`. */
#define CTR_TP_OK 0
#define CTR_TP_BAD_TABLE 1
#define CTR_TP_MAX_BINS 512          /* edge2, the counts and the sums of a workgroup are in LDS */
#define CTR_TP_MAX_LAGS 16
typedef struct ctr_twopoint {
  int32_t ndim;                    /* 2 or 3 */
  int32_t pairs;                   /* CTR_PCF_PAIRS_* */
  int32_t n_lags;                  /* K, 1 .. CTR_TP_MAX_LAGS */
  int32_t reserved0;
  int64_t n_bins;                  /* B, 1 .. CTR_TP_MAX_BINS */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  int64_t n_particles;             /* P */
  double dr;                       /* > 0 */
  double max2;                     /* max_disp squared, within [2^-500, 2^500]; (n_bins dr)^2 max2 <= 2^1000 */
  double mpp[CTR_MAX_NDIM];        /* per axis, > 0 */
  int64_t lag[CTR_TP_MAX_LAGS];    /* ascending, distinct, >= 1 */
  const double* pos;               /* [N, ndim] */
  const int64_t* frame_offset;     /* [T + 1] */
  const int64_t* particle;         /* [N] */
  const int64_t* group;            /* [N], or null with CTR_PCF_PAIRS_ALL */
  const double* edge2;             /* [B + 1] */
  int64_t* n;                      /* [K, B] out */
  double* dot;                     /* [K, B] out */
  double* longitudinal;            /* [K, B] out */
  double* transverse;              /* [K, B] out */
  double* cos;                     /* [K, B] out */
  int64_t* sums;                   /* [K, B, 3, 2] out: dot, L, c; each (hi, lo) */
  int64_t* n_moved;                /* [K] out */
  int64_t* beyond;                 /* [K] out */
  int32_t* status;                 /* [1] out */
} ctr_twopoint;
int ctr_twopoint_device(ctr_handle* h, const ctr_twopoint* d, void* hip_stream);

/* ---- contact episodes and bond lifetimes of linked particles (ABI 8, additions) ----
 * How long two particles stay together: g(r) above gives the bond length, the neighbours say how
 * close rows come, the two-point correlations whether they move together; this is the quantity that
 * separates a bonded cluster from a collision, the number that min_frames of
 * ctr_cluster_tracks_device is compared with, and for self-assembling clusters the physics itself
 * (association and dissociation rates, the survival curve of a bond).  Two knobs keep a lifetime
 * from measuring the localisation noise and the dropout rate: a contact switches on below r_on and
 * off at r_off >= r_on (a Schmitt trigger), and up to `gap` frames without the pair are bridged.
 * The rule is the project's own; tests/_contacts.py restates it in NumPy.  Every output is an
 * integer or a minimum / maximum of doubles: it equals the restatement exactly.
 * Input: pos [N, ndim], ndim 2 or 3, rows sorted by frame; frame_offset [T + 1]; particle [N], ids
 * below P, negative = unlinked; group [N] or null; mpp per axis, > 0; on2, off2, gap.
 *   1. Inputs.  q = pos * mpp per axis, one rounding.  A row takes part when every coordinate of q is
 *      finite and particle >= 0.
 *   2. Thresholds.  r_on > 0, r_off >= r_on, in the units of pos * mpp; on2 = r_on * r_on and off2 =
 *      r_off * r_off are computed once on the host.  gap is an integer >= 0.
 *   3. Entries.  For every frame t and every ordered pair of rows (i, j) of that frame that take part,
 *      with particle[i] < particle[j] and d2 < off2, there is an entry (a = particle[i], b =
 *      particle[j], t, d2); d2 = the sum over the axes, in axis order, of (q_j - q_i)_a squared,
 *      every product and sum rounded on its own.  CTR_PCF_PAIRS_SAME / _OTHER with group filter the
 *      entries as in clause 6 of g(r).  The entries of row i are emitted in ascending j; entries lie
 *      in (frame, i, j) order.  n_entries counts them.
 *   4. Pair order.  The entries are sorted stably by key = a * P + b (P <= 2^31 - 1: below 2^62);
 *      within a pair they stay in frame order.
 *   5. Duplicates.  An entry with the key and the frame of the entry before it -- a particle repeated
 *      in a frame -- is a duplicate: counted in `duplicates` and otherwise ignored; the first in
 *      (frame, i, j) order counts.
 *   6. Chains.  An entry that is no duplicate heads a chain when it is the first of its pair, or when
 *      its frame exceeds the frame of the entry before it by more than gap + 1.  So up to `gap`
 *      frames without an entry are bridged, whether one of the two was missing in them or the two
 *      were r_off or more apart.
 *   7. Episodes.  A chain holds at most one episode: it begins at the chain's first entry with d2 <
 *      on2 and ends at the chain's last entry; a chain without such an entry has none.  Its fields:
 *      a, b; first, last (frames); lifetime = last - first + 1; n_seen, the entries that are no
 *      duplicates from the first on-entry on; min_d2, max_d2 over those.
 *   8. Censoring.  first_seen[p], last_seen[p]: the first and last frame with a row of p that takes
 *      part; T and -1 for a particle that never does.  An episode is left_open when its first
 *      on-entry heads the chain and first - max(first_seen[a], first_seen[b]) <= gap; right_open when
 *      min(last_seen[a], last_seen[b]) - last <= gap; complete when neither.
 *   9. Series, int64 [T].  formed[first] += 1 for the episodes that are not left_open;
 *      broken[last + 1] += 1 for those not right_open (last + 1 <= T - 1 by clause 8); active[t] =
 *      the episodes with first <= t <= last.
 *  10. Lifetimes.  lifetime_count [2, L]: row 0 the complete episodes, row 1 the open ones (either
 *      side), at index lifetime - 1; lifetime_above [2]: those with lifetime > L.
 *      count.sum() + above.sum() == n_episodes.
 *  11. Pairs.  Episodes lie in (a, b, first) order.  Every pair with an episode has a row: pair_a,
 *      pair_b, pair_episodes, pair_frames (the sum of its lifetimes), pair_first, pair_last; n_pairs
 *      counts the rows.
 *  12. A refused table.  A frame_offset that does not rise within [0, N] or a particle[i] >= P:
 *      status[0] = CTR_CON_BAD_TABLE; counts, series and histogram 0, every column and first_seen /
 *      last_seen -1, the doubles NaN; no kernel follows an index of a refused table.
 *  13. Capacity.  Every per-entry, per-episode and per-pair buffer has max_entries rows.  n_entries >
 *      max_entries: status[0] = CTR_CON_OVERFLOW, n_entries as counted, everything else as in 12.
 *      Rows of the columns beyond n_episodes / n_pairs hold -1 and NaN.
 * Three phases, each a call; the caller owns everything that passes from one to the next.
 * CTR_CON_COUNT: cont_check; cont_count_defaults; cont_items (the scan of ceil(rows / 256) over the
 * frames); cont_count: a work item is a frame and a tile of 256 of its rows, a thread owns a row, walks
 * the frame's rows staged 256 at a time in LDS (the walk of g(r)), counts its entries into
 * entry_start[i] and notes its frame in first_seen / last_seen with 64-bit integer atomic minima and
 * maxima; then the exclusive scan of the N counts in place, entry_start[N] = n_entries.  A caller
 * without a capacity reads that word here.  CTR_CON_FILL: cont_fill_defaults (the overflow, the key
 * 2^63 - 1 in every slot without an entry); cont_items; cont_fill repeats the walk and writes key,
 * frame and d2 of row i from entry_start[i] on: no atomic append.  Between FILL and EPISODES the
 * caller sorts key stably and gathers frame and d2 by the permutation.  CTR_CON_EPISODES:
 * cont_episode_defaults; the scan of the chain heads, which places the first entry of every chain;
 * cont_chains, one chain per wavefront, the 64 lanes striding its entries, with shuffle reductions
 * for the first on-entry, n_seen, the minimum and the maximum; the scan of the chains with an
 * episode; cont_episodes, a thread per episode: its row, and integer atomics into formed, broken,
 * the difference array of active and the histogram, one per distinct address among the lanes of a
 * wavefront (the episodes of one lifetime share a bin); the scan of the pair heads; cont_pairs, one pair
 * per wavefront; cont_active, one workgroup: the running sum of the difference array.  Every scan is
 * three launches (cont_scan_sums: a sum per tile of 256 values; cont_scan_top: one workgroup over
 * those; cont_scan_apply), so no workgroup waits on another.  256 threads each; integer atomics
 * only: the same bytes on every call.
 * Bytes that a call allocates per entry of max_entries: 20 for key, frame and d2 and 28 for their
 * sorted copies and the permutation, 72 for the episode columns, 48 for the pair columns, 56 of the
 * handle's scratch (the chains, their episodes, the pairs): 224 in all; besides, 8 (N + 1) for
 * entry_start, 16 P, 24 T + 16 L, and of the scratch 16 (T + 1) + max(N, max_entries) / 32.
 * Descriptors are checked before the handle.  Device pointers; asynchronous on `hip_stream`. */
#define CTR_CON_COUNT 0              /* phase */
#define CTR_CON_FILL 1
#define CTR_CON_EPISODES 2
#define CTR_CON_OK 0
#define CTR_CON_BAD_TABLE 1
#define CTR_CON_OVERFLOW 2
#define CTR_CON_MAX_LIFETIME 1048576 /* 2^20: L at most */
typedef struct ctr_contacts {
  int32_t phase;                   /* CTR_CON_COUNT, _FILL, _EPISODES */
  int32_t ndim;                    /* 2 or 3 */
  int32_t pairs;                   /* CTR_PCF_PAIRS_* */
  int32_t reserved0;
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N */
  int64_t n_particles;             /* P */
  int64_t gap;                     /* 0 .. 2^31 - 1 */
  int64_t max_lifetime;            /* L, 1 .. CTR_CON_MAX_LIFETIME (EPISODES) */
  int64_t max_entries;             /* M >= 0: rows of every per-entry buffer (FILL, EPISODES) */
  double on2;                      /* r_on squared, > 0 */
  double off2;                     /* r_off squared, >= on2 */
  double mpp[CTR_MAX_NDIM];        /* per axis, > 0 */
  const double* pos;               /* [N, ndim] (COUNT, FILL) */
  const int64_t* frame_offset;     /* [T + 1] (COUNT, FILL) */
  const int64_t* particle;         /* [N] (COUNT, FILL) */
  const int64_t* group;            /* [N], or null with CTR_PCF_PAIRS_ALL (COUNT, FILL) */
  int64_t* entry_start;            /* [N + 1] COUNT out, FILL in */
  int64_t* n_entries;              /* [1] COUNT out, FILL and EPISODES in */
  int64_t* first_seen;             /* [P] COUNT out, EPISODES in */
  int64_t* last_seen;              /* [P] COUNT out, EPISODES in */
  int64_t* key;                    /* [M] FILL out; EPISODES in, sorted */
  int32_t* frame;                  /* [M] FILL out; EPISODES in, in the order of key */
  double* d2;                      /* [M] FILL out; EPISODES in, in the order of key */
  int64_t* a;                      /* [M] episode columns, EPISODES out */
  int64_t* b;
  int64_t* first;
  int64_t* last;
  int64_t* lifetime;
  int64_t* n_seen;
  int32_t* left_open;              /* [M] 0 / 1 */
  int32_t* right_open;
  double* min_d2;
  double* max_d2;
  int64_t* pair_a;                 /* [M] pair columns, EPISODES out */
  int64_t* pair_b;
  int64_t* pair_episodes;
  int64_t* pair_frames;
  int64_t* pair_first;
  int64_t* pair_last;
  int64_t* formed;                 /* [T] EPISODES out */
  int64_t* broken;                 /* [T] */
  int64_t* active;                 /* [T] */
  int64_t* lifetime_count;         /* [2, L] */
  int64_t* lifetime_above;         /* [2] */
  int64_t* duplicates;             /* [1] */
  int64_t* n_episodes;             /* [1] */
  int64_t* n_pairs;                /* [1] */
  int32_t* status;                 /* [1] COUNT out; FILL in / out; EPISODES in */
} ctr_contacts;
int ctr_contacts_device(ctr_handle* h, const ctr_contacts* d, void* hip_stream);
/* The launch decision of a call without a device: scratch_bytes of the handle; scan_tiles [2], the
 * tiles of the scan over the N rows and over the max_entries entries; grids [4], the workgroups of
 * cont_check, of the walks, of a kernel over the entries and of cont_chains, at the default cap of
 * a grid.  Any of the pointers may be null. */
int ctr_contacts_plan(const ctr_contacts* d, int64_t* scratch_bytes, int64_t* scan_tiles, int64_t* grids);

/* ---- shape coordinates of tracked clusters: bonds, angles, flexibility (ABI 8, additions) ----
 * Everything ctr_orientation_device and ctr_diffusion_device report assumes that a tracked cluster is
 * a rigid body: a basis is built from the features' positions, and every change of it is read as
 * rotation.  These calls are the check of that assumption, and the plain measurement that comes with
 * it (the bond length that constraints.dimer / trimer / tetramer need): the internal coordinates of
 * every cluster in every frame, their distributions, and their displacement statistics over a sweep
 * of lags.  The rule is this project's own; tests/_shape.py restates it with plain loops.  Input: the
 * block `pos` [T, F, n, ndim] of ctr_track_positions_device, (z,) y, x, NaN where the cluster is not
 * complete; n = cluster_size in {2, 3, 4}, ndim in {2, 3}; the 2D tetramer is accepted (no basis is
 * needed).  No operation below is contracted to a fused multiply-add.
 *   Rule 1, the coordinates of one (track, frame): C = NB + NA + 1 of them, in this order (C = 2, 7,
 *     19 for n = 2, 3, 4).  x[i, a] = pos[i, a] * mpp[a], the product rounded on its own.
 *     Bonds: NB = n (n - 1) / 2, the pairs a < b in lexicographic order (bond_ab): d = x[b] - x[a],
 *       bond2 = sum over the axes, in axis order, of d * d, every product and sum rounded on its own;
 *       bond = sqrt(bond2), correctly rounded.
 *     Angles: NA = n (n - 1) (n - 2) / 2 (0, 3, 12): for the vertex a ascending, the pairs b < c of the
 *       other features in lexicographic order (angle_a_bc): u = x[b] - x[a], v = x[c] - x[a], dot = sum
 *       u_k v_k in axis order; in 2D cr = |u_0 v_1 - u_1 v_0|; in 3D cr = sqrt(c_0 c_0 + c_1 c_1 + c_2
 *       c_2) with c = (u_1 v_2 - u_2 v_1, u_2 v_0 - u_0 v_2, u_0 v_1 - u_1 v_0), each component and each
 *       square rounded on its own; angle = atan2(cr, dot) in [0, pi].  Coincident features give what
 *       IEEE atan2 gives (0): no error.
 *     Radius of gyration (rg, last): c_k = (sum_i x[i, k]) / n, features in order; rg = sqrt((sum_i
 *       sum_k (x[i, k] - c_k)^2) / n), features outer, axes inner, correctly rounded.
 *     Missing data: a frame with a non-finite x among its n ndim gives NaN in all C coordinates.
 *   Rule 2, dynamics, per track t, coordinate c (value q) and lag k of lags[0 .. L - 1] (any integers;
 *     k < 1 or k >= F has no row): the rows are the frames b with q[b] and q[b + k] both finite, d =
 *     q[b + k] - q[b]; n[t, c, l] counts them (exact); mean_d, mean_d2, mean_d4 are the means of d, of
 *     rn(d d) and of rn(rn(d d) rn(d d)); flex = ((mean_d2 * 0.5) * fps) / k, the scaling of
 *     ctr_diffusion_device: the joint flexibility of an angle, the breathing diffusivity of a bond.
 *     Where n == 0 the four are NaN.  Pooled over the tracks: pooled_n [C, L] and pooled_mean_d,
 *     pooled_mean_d2, pooled_mean_d4, pooled_flex from the sums of the tracks added in track order.
 *     (Slots follow the order of `particle`, so between tracks they are arbitrary: the counts and the
 *     means are returned so that a caller can pool slots.)  Static moments per (t, c) over the frames
 *     with a finite q: count, mean, var = mean((q - mean)^2) in two passes, min, max; NaN where count is 0.
 *     Order of the sums: a workgroup per (track, tile of CTR_SHAPE_TILE = 256 frames) stages its tile
 *     and a halo of frames behind it in LDS; the halo depends on F and C alone, never on the lags:
 *     halo = min(max(F - 256, 0), min(CTR_SHAPE_HALO_CAP = 768, (8192 - 320) / C - 256)) (ctr_shape_plan);
 *     a later frame beyond it is read from global memory: the same double.  Lane = frame of the tile; per
 *     (coordinate, lag) the four sums go through one fixed wavefront tree, the four wavefronts are added
 *     in their order, one partial per (track, tile, lag, coordinate); a second kernel adds the tiles in
 *     tile order, a third the sums of the tracks in track order.  No float atomics: a (track, coordinate, lag) is
 *     the same bytes alone, inside a batch of tracks, inside a sweep of lags, and on any stream.
 *   Rule 3, distributions: bond bins B = bond_bins = ceil(bond_max / bond_dr), 1 <= B <=
 *     CTR_SHAPE_MAX_BOND_BINS; bond_edges[b] = b * bond_dr, b = 0 .. B; angle bins A = angle_bins, 1 <=
 *     A <= CTR_SHAPE_MAX_ANGLE_BINS, angle_edges = A + 1 equal steps from 0 to pi, angle_edges[A] the
 *     double nearest pi; both computed by the caller and handed over.  A value v is in bin b iff
 *     edges[b] <= v < edges[b + 1], decided by comparison with the edges (the device guesses with a
 *     product); the last angle bin is closed at pi; bonds and rg at or above the last edge count in
 *     `above`; a NaN is nowhere.  count_bond [NB + 1, B] (rg last), above [NB + 1], count_angle [NA, A],
 *     n [1] = frames that entered (bond_01 is not NaN); with per_track a leading T on all four.  Counts
 *     are int64 and exact; on every row count.sum() + above == n for finite coordinates.  density_bond =
 *     count_bond / (n * bond_dr), density_angle = count_angle / (n * angle_width), angle_width = pi / A
 *     as the caller rounds it; NaN where n == 0.
 * Launches, 256 threads each.  shape_coords_kernel<ndim, n>: one lane per (track, frame), lanes along
 * the frames; for ctr_shape_device it writes coords [T, F, C]; for the other two it writes the handle's
 * scratch coordinate-major, [C][T F], so that every later read of a coordinate is contiguous along the
 * frames, and trigonometry is done once per frame however many tiles stage it.  Dynamics:
 * shape_partial_kernel, shape_final_kernel, shape_pool_kernel as above and shape_moments_kernel, a
 * workgroup per (track, coordinate).  Histogram: shape_hist_kernel, a workgroup per (track or all,
 * coordinate, chunk of 4096 frames) with uint32 counters in LDS and integer atomics on the int64
 * tables, then shape_density_kernel.  Scratch of the handle: 8 C T F bytes, and for the dynamics 32 C L
 * T (ceil(F / 256) + 1) bytes behind it: the partials, and the sums of every track that the pooling reads.  Calls of one handle that use it are ordered on the device.
 * Descriptors are checked before the handle.  Device pointers, lags included; asynchronous. */
#define CTR_SHAPE_MAX_COORDS 19
#define CTR_SHAPE_TILE 256
#define CTR_SHAPE_HALO_CAP 768
#define CTR_SHAPE_MAX_BOND_BINS 4096
#define CTR_SHAPE_MAX_ANGLE_BINS 1024
typedef struct ctr_shape {
  int32_t ndim;                    /* 2 or 3 */
  int32_t cluster_size;            /* n: 2, 3 or 4 */
  int64_t n_tracks;                /* T */
  int64_t n_frames;                /* F */
  double mpp[CTR_MAX_NDIM];        /* per axis, finite */
  const double* pos;               /* [T, F, n, ndim] */
  double* coords;                  /* [T, F, C] out */
} ctr_shape;
int ctr_shape_device(ctr_handle* h, const ctr_shape* s, void* hip_stream);

typedef struct ctr_shape_dynamics {
  int32_t ndim;                    /* 2 or 3 */
  int32_t cluster_size;            /* n: 2, 3 or 4 */
  int64_t n_tracks;                /* T */
  int64_t n_frames;                /* F */
  int64_t n_lags;                  /* L */
  double fps;                      /* finite, > 0 */
  double mpp[CTR_MAX_NDIM];        /* per axis, finite */
  const int64_t* lags;             /* [L], device memory */
  const double* pos;               /* [T, F, n, ndim] */
  int64_t* n;                      /* [T, C, L] out */
  double* mean_d;                  /* [T, C, L] out */
  double* mean_d2;                 /* [T, C, L] out */
  double* mean_d4;                 /* [T, C, L] out */
  double* flex;                    /* [T, C, L] out */
  int64_t* pooled_n;               /* [C, L] out */
  double* pooled_mean_d;           /* [C, L] out */
  double* pooled_mean_d2;          /* [C, L] out */
  double* pooled_mean_d4;          /* [C, L] out */
  double* pooled_flex;             /* [C, L] out */
  int64_t* count;                  /* [T, C] out: frames with a finite coordinate */
  double* mean;                    /* [T, C] out */
  double* var;                     /* [T, C] out */
  double* min;                     /* [T, C] out */
  double* max;                     /* [T, C] out */
} ctr_shape_dynamics;
int ctr_shape_dynamics_device(ctr_handle* h, const ctr_shape_dynamics* d, void* hip_stream);
/* No device needed: the launch decision of ctr_shape_dynamics_device from the scalars of d (its
 * pointers are not looked at): the frames of a tile, the halo staged behind it, the dynamic LDS of a
 * workgroup, the tiles of a track and the scratch of the call. */
int ctr_shape_plan(const ctr_shape_dynamics* d, int32_t* tile, int32_t* halo, int64_t* lds_bytes, int64_t* n_tiles,
                   int64_t* scratch_bytes);

typedef struct ctr_shape_histogram {
  int32_t ndim;                    /* 2 or 3 */
  int32_t cluster_size;            /* n: 2, 3 or 4 */
  int32_t per_track;               /* 0: all tracks in one table; 1: a leading T on the outputs */
  int32_t reserved0;
  int64_t n_tracks;                /* T */
  int64_t n_frames;                /* F */
  int64_t bond_bins;               /* B, 1 .. CTR_SHAPE_MAX_BOND_BINS */
  int64_t angle_bins;              /* A, 1 .. CTR_SHAPE_MAX_ANGLE_BINS */
  double bond_dr;                  /* finite, > 0 */
  double angle_width;              /* pi / A as the caller rounds it */
  double mpp[CTR_MAX_NDIM];        /* per axis, finite */
  const double* pos;               /* [T, F, n, ndim] */
  const double* bond_edges;        /* [B + 1] */
  const double* angle_edges;       /* [A + 1] */
  int64_t* count_bond;             /* [(T,) NB + 1, B] out */
  int64_t* above;                  /* [(T,) NB + 1] out */
  int64_t* count_angle;            /* [(T,) NA, A] out */
  int64_t* n;                      /* [1] or [T] out */
  double* density_bond;            /* [(T,) NB + 1, B] out */
  double* density_angle;           /* [(T,) NA, A] out */
} ctr_shape_histogram;
int ctr_shape_histogram_device(ctr_handle* h, const ctr_shape_histogram* d, void* hip_stream);

/* ---- model and residual frames of a fitted table (ABI 8, additions) ----
 * The step after ctr_refine_batch_device: the fitted model drawn back into the frames, the frames
 * minus the model, and the goodness-of-fit sums per feature and per cluster by the rule of the
 * reference's FitFunctions.get_residual (fitfunc.py:421-450).  Input: the frames [T, (z,) y, x] in
 * any CTR_DTYPE_*, params [N, n_params] in the column order of a ctr_problem -- background, signal,
 * <pos>, <size...>, <profile parameters> -- with the rows sorted by frame, frame_offset [T + 1], mask_pos
 * [N, ndim] (the centres of the elliptical masks; NULL: the positions in params), cluster [N] (the
 * smallest row of the row's cluster; NULL: no per-cluster output).  The residual is against the
 * raw frame; constraints do not enter the model.  The rule is the project's own
 * (tests/_residual.py restates it in NumPy with plain loops over the rows); no operation is
 * contracted to a fused multiply-add.
 *
 * For pixel x of frame t and the rows i of that frame in ascending row order:
 *   Covering.  Row i covers x when sum(((x - mask_pos_i) / radius)**2) <= 1, evaluated as NumPy
 *     does: per axis a division, a product and a sum, in axis order, each rounded once; the edge is
 *     included.  The box of a mask is clipped to the frame: a centre outside the frame covers
 *     whatever part of its ellipse lies inside, a non-finite centre covers nothing.
 *   Per-pixel maps.  coverage(x) is the number of covering rows (int32), owner(x) the lowest
 *     covering row, or -1.
 *   Term of a row.  term_i(x) = signal_i * g(r2_i(x)), with r2 and g as the refine kernels evaluate
 *     them: d_a = x_a - pos_a, r2 = the sum over the axes, in axis order, of (d_a * d_a) * (1 / (size_a
 *     * size_a)), every operation rounded on its own.  gauss: g = exp(-0.5 ndim r2).  ring (e =
 *     thickness): r = sqrt(r2), num = r - 1 + e, g = exp(-0.5 ndim ((num / e) * (num / e))).  disc (e =
 *     disc_size): e <= 0 the Gaussian; else ds = e, or 0.999 where e >= 1; g = 1 unless r2 > ds ds,
 *     where u = (sqrt(r2) - ds) / (1 - ds), g = exp(u u ndim / -2).  inv_series_<N> (e[0 .. N]): g = e[0] / y,
 *     y = polyval([1, e[1], ..., e[N]], r2) in Horner's order.  For ring and disc these are the
 *     reference's r2_*_safe forms: where q = the sum of d_a d_a over the axes, last axis first, is
 *     below 1, g is NaN (the disc with disc_size > 0 has the value 1 there, as the reference's
 *     disc_func leaves it).
 *   Residual.  residual(x) = ((image(x) - background_owner) - term_i1) - term_i2 ... over the covering
 *     rows in ascending row order (fitfunc.py:443-448).
 *   Model.  model(x) = background_owner + s, where s starts from 0 and takes the terms of the
 *     covering rows in the same order.
 *   Outside every mask.  outside decides the residual: 0.0 (CTR_RESID_ZERO), NaN (CTR_RESID_NAN) or
 *     float64(image(x)) (CTR_RESID_IMAGE); model is 0.0, NaN or 0.0 respectively.
 *   Per feature [N].  n_pix: covered pixels; n_own: pixels with owner == i; n_nan: covered pixels
 *     whose residual is NaN; sum, sum_sq, max_abs: over its covered pixels whose residual is not NaN
 *     (the reference's nansum; 0 where there is none); own_sum_sq: the same over its owned pixels;
 *     rms = sqrt(sum_sq / n_pix), the divisor counting the NaN pixels as len(image) does there, NaN
 *     for n_pix == 0.  Order of the sums: the pixels of the clipped box of the mask (every axis from
 *     floor(max(c - radius - 1, 0)) to ceil(min(c + radius + 1, shape - 1))) are numbered in
 *     row-major order; lane l of the feature's wavefront adds the pixels l, l + 64, ... in that order,
 *     and the 64 lane sums are added by the butterfly x += x[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.
 *   Per cluster, only when cluster is given; per row [N], every row carrying its cluster's value.
 *     cluster_n_pix = the sum of n_own over the rows of the cluster, cluster_sum_sq = the sum of
 *     own_sum_sq, in ascending row order; cost = sqrt(cluster_sum_sq / cluster_n_pix) / max(frame_t),
 *     the frame maximum of ctr_frame_max_device.  Where the masks of different clusters do not
 *     overlap (always for separation >= diameter), cluster_sum_sq / cluster_n_pix is what
 *     get_residual(..., norm=1.) returns for that cluster, and with mask_pos the last round's
 *     centres cost is ctr_batch.cost.
 * No float atomics; every output is the same bytes on every call, on every stream, and a frame's
 * outputs do not depend on which other frames are in the call.
 *
 * status[0]: CTR_RESID_OK; CTR_RESID_BAD_TABLE for a frame_offset that does not rise from 0 to N
 * (found by the first kernel; no other output is then written); CTR_RESID_BAD_CLUSTER for a cluster
 * entry that is not a row c <= i of the row's frame with cluster[c] == c (those rows get 0, 0 and NaN).
 *
 * Launch (ctr_residual_plan).  Frame pass: a workgroup of 256 owns a tile of 8 x 32
 * (2D) or 2 x 8 x 16 (3D) pixels of one frame, walks the rows of the frame in chunks of
 * CTR_RESID_CHUNK through LDS in ascending row order, compacted to those whose clipped box meets
 * the tile, and every pixel accumulates its terms in row order; a frame of any number of rows takes
 * as many chunks as it needs.  Feature pass: one wavefront per row walks its clipped box and reads
 * the residual and owner just written.  Cluster pass: a thread per row adds the rows of its cluster
 * in its frame.  Every grid is capped (the handle's cap, ctr_set_stage_max_grid; max_grid > 0 lowers
 * it further) and strides.  Scratch: the residual (8 B a pixel) and owner (4 B a pixel) where
 * want_frames is 0, and 16 B a frame for the frame maxima where has_cluster is set. */
#define CTR_RESID_CHUNK 256
enum { CTR_RESID_ZERO = 0, CTR_RESID_NAN = 1, CTR_RESID_IMAGE = 2 };
enum { CTR_RESID_OK = 0, CTR_RESID_BAD_TABLE = 1, CTR_RESID_BAD_CLUSTER = 2 };
typedef struct ctr_residual {
  int32_t ndim;                    /* 2 or 3 */
  int32_t frame_dtype;             /* CTR_DTYPE_* */
  int32_t fit_function;            /* CTR_FIT_* */
  int32_t isotropic;               /* 1: one size column; 0: one per axis */
  int32_t n_profile;               /* profile parameters: gauss 0, ring and disc 1, inv_series_<N> N + 1 */
  int32_t outside;                 /* CTR_RESID_ZERO, _NAN or _IMAGE */
  int32_t want_frames;             /* 1: residual, coverage and owner are outputs; 0: all three NULL */
  int32_t want_model;              /* 1: model is an output; 0: NULL */
  int32_t has_cluster;             /* 1: cluster and the three per-cluster outputs are given; 0: all NULL */
  int32_t max_grid;                /* > 0: a cap on every grid below the handle's; 0: the handle's */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N < 2^31 - 1 */
  int64_t shape[CTR_MAX_NDIM];     /* (z,) y, x of a frame */
  int64_t radius[CTR_MAX_NDIM];    /* of the masks, 1 .. 1024 */
  const void* frames;              /* [T, (z,) y, x] */
  const int64_t* frame_offset;     /* [T + 1] */
  const double* params;            /* [N, 2 + ndim + (isotropic ? 1 : ndim) + n_profile] */
  const double* mask_pos;          /* [N, ndim] or NULL */
  const int64_t* cluster;          /* [N] or NULL */
  double* residual;                /* [T, (z,) y, x] out or NULL */
  double* model;                   /* [T, (z,) y, x] out or NULL */
  int32_t* coverage;               /* [T, (z,) y, x] out or NULL */
  int32_t* owner;                  /* [T, (z,) y, x] out or NULL */
  int64_t* n_pix;                  /* [N] out */
  int64_t* n_own;                  /* [N] out */
  int64_t* n_nan;                  /* [N] out */
  double* sum;                     /* [N] out */
  double* sum_sq;                  /* [N] out */
  double* own_sum_sq;              /* [N] out */
  double* max_abs;                 /* [N] out */
  double* rms;                     /* [N] out */
  int64_t* cluster_n_pix;          /* [N] out or NULL */
  double* cluster_sum_sq;          /* [N] out or NULL */
  double* cost;                    /* [N] out or NULL */
  int32_t* status;                 /* [1] out */
} ctr_residual;
int ctr_residual_device(ctr_handle* h, const ctr_residual* r, void* hip_stream);
/* No device needed: the launch decision of ctr_residual_device from the scalars of r (its pointers
 * are not looked at) and the default cap of a handle: tile [3] the pixels of a tile per axis (1
 * beyond ndim), chunk the rows of a chunk, n_tiles the tiles of the call, grids [4] the workgroups of
 * the check, frame, feature and cluster kernels (0: not launched), lds_bytes the LDS of a workgroup
 * of the frame pass, scratch_bytes the scratch of the call. */
int ctr_residual_plan(const ctr_residual* r, int32_t* tile, int32_t* chunk, int64_t* n_tiles, int64_t* grids,
                      int64_t* lds_bytes, int64_t* scratch_bytes);

/* ---- standard errors and covariance of a fitted table (ABI 8, additions) ----
 * The other step after ctr_refine_batch_device: how well every parameter is determined.  The exact
 * Hessian of the reference's objective (FitFunctions.get_residual, fitfunc.py:421-450) at a fitted
 * table, per cluster, for every profile, parameter mode and pixel type; from it the reference's
 * sqrt(2 diag(inv H)) (refine.py:400-406) and, on request, the covariance of the cluster's
 * variables.  Input: frames, params, frame_offset and mask_pos as ctr_residual takes them; order [N],
 * the rows sorted by (frame, cluster label) with a stable sort; cluster_offset [C + 1], the ranges of
 * the clusters in order.  The rule is the project's own (tests/_fit_error.py restates it in NumPy
 * with plain loops); bounds and constraints do not enter, as in the reference.
 *
 *   Clusters.  A cluster is the set of rows of one frame with one value of `cluster`; the rows need
 *     not be contiguous in the table; within a cluster the rows are taken in ascending row order.
 *   Variables.  The layout is that of vect_from_params (fitfunc.py:207-263) for the modes of the
 *     columns, in column order: a CTR_MODE_VAR column gives one variable per row, a
 *     CTR_MODE_CLUSTER column one variable per cluster, a CTR_MODE_CONST column none;
 *     CTR_MODE_GLOBAL is refused.  The background is CONST or CLUSTER.  The value of a cluster
 *     variable is that of the cluster's first row where all its rows are equal (as
 *     ctr_batch.params_out has them), else their sum in row order divided by their number; the
 *     model reads that value for every row.  A constant background is that of the first row.
 *   Pixels.  Covering, box clipping, r2, g and the NaN rule of the ring and disc "safe" forms are
 *     ctr_residual's "Covering" and "Term of a row", with the values of the variables as above.
 *     P is the number of pixels covered by at least one row of the cluster, NaN pixels included,
 *     whatever other clusters cover.  A pixel whose residual is NaN enters no sum (the reference's
 *     nansum).
 *   Residual and Hessian.  res(x) = image(x) - background - sum_i signal_i g(r2_i(x), e_i) over the
 *     covering rows of the cluster in row order.  F = sum res^2 / (P norm), norm = max(frame)^2 /
 *     residual_factor (refine.py:354), the frame maximum of ctr_frame_max_device.  The Hessian of F
 *     is 2 (J^T J + Q) / (P norm): J the Jacobian of res in the variables, Q = sum_x res(x)
 *     d2res(x), exact in all variables -- signal, centres, sizes and every profile parameter.  With
 *     m = s g(r2(c, size), e): m_ss = 0, m_sp = g' r2_p, m_se = g_e, m_pq = s (g'' r2_p r2_q + g'
 *     r2_pq), m_pe = s g'_e r2_p, m_ee' = s g_ee' (p, q over centres and sizes, ' the derivative in
 *     r2), and d2res = -d2m.  r2_c = -2 d / size^2, r2_size = -2 d^2 / size^3 (isotropic: -2 q /
 *     size^3, q the sum of d^2), r2_cc = 2 / size^2, r2_c,size = 4 d / size^3, r2_size,size = 6 d^2
 *     / size^4 (isotropic: 6 q / size^4), all others 0.  gauss (k = ndim / 2): g' = -k g, g'' = k^2 g.
 *     ring and disc through r = sqrt(r2): g' = g_r / (2 r), g'' = g_rr / (4 r2) - g_r / (4 r^3), g'_e
 *     = g_re / (2 r), with g = exp(phi), g_a = g phi_a, g_ab = g (phi_a phi_b + phi_ab); ring: phi =
 *     -k w^2, w = (r - 1 + e) / e; disc: phi = -k u^2, u = (r - ds) / (1 - ds), in the region r2 <=
 *     ds^2 g = 1 with all derivatives 0, the clamp disc_size >= 1 -> 0.999 has derivative 0 in
 *     disc_size, disc_size <= 0 is the Gaussian.  inv_series: g = e0 / y, y the polynomial in r2; g'
 *     = -e0 y' / y^2, g'' = e0 (2 y'^2 / y^3 - y'' / y^2), g_e0 = 1 / y, g_ek = -e0 r2^(N - k) / y^2,
 *     g_e0,ek = -r2^(N - k) / y^2, g_ek,el = 2 e0 r2^(N - k) r2^(N - l) / y^3, g'_e0 = -y' / y^2, g'_ek
 *     = -e0 ((N - k) r2^(N - k - 1) / y^2 - 2 y' r2^(N - k) / y^3).  Where the safe form makes the
 *     disc's g 1 (q < 1, disc_size > 0) all derivatives are 0.  A feature's block in parameter space
 *     is added to the rows and columns of the variables its parameters map to; a shared variable
 *     collects every feature's block.
 *   Result.  A = J^T J + Q is factored by Cholesky; a pivot that is not a positive finite number
 *     makes the cluster CTR_FITERR_NOT_POSITIVE_DEFINITE.  Otherwise cov = P norm A^-1 and std_v =
 *     sqrt(cov_vv).  params_std [N, n_params] is vect_to_params of std: a cluster variable's value
 *     goes on every row of the cluster, a constant column is NaN, a failed cluster is all NaN.
 *   Statuses, per cluster (every row carries its cluster's), as data and never as errors:
 *     CTR_FITERR_OK; CTR_FITERR_NOT_POSITIVE_DEFINITE; CTR_FITERR_NONFINITE, a non-finite
 *     parameter in a variable or in a value the model reads (a mask centre included);
 *     CTR_FITERR_EMPTY, P == 0; CTR_FITERR_TOO_LARGE, more than 64 rows or more than CTR_MAX_VARS
 *     variables (n_pix is then 0 and the cluster has no covariance block); CTR_FITERR_BAD_TABLE
 *     on every row, when frame_offset, order, cluster_offset or the offsets of the covariance do
 *     not fit together or a cluster's rows lie in more than one frame.
 *   Order of the sums.  The covered pixels of a cluster are numbered by owner (the lowest covering
 *     row of the cluster, in row order) and, within an owner, in row-major order of the clipped box
 *     of its mask; every entry of J^T J adds the pixels in that order.  The block of a feature adds
 *     the pixels of its box as ctr_residual's per-feature sums do (lane l the pixels l, l + 64, ...,
 *     then the butterfly), and the blocks are added to A after J^T J in row order.  Cholesky and
 *     the inverse take their terms in index order.
 * No float atomics; every output is the same bytes on every call, on every stream, whatever else is
 * in the batch.
 *
 * Launch (ctr_fit_error_plan).  One workgroup of 256 per cluster; the matrix lives in
 * LDS as a packed triangle, and a cluster is taken by the launch of its size class (at most 16, 48
 * or CTR_MAX_VARS variables), which sizes the LDS request.  Scratch: 16 B a frame for the frame
 * maxima. */
enum { CTR_FITERR_OK = 0, CTR_FITERR_NOT_POSITIVE_DEFINITE = 1, CTR_FITERR_NONFINITE = 2, CTR_FITERR_EMPTY = 3,
       CTR_FITERR_TOO_LARGE = 4, CTR_FITERR_BAD_TABLE = 5 };
#define CTR_FITERR_MAX_ROWS 64
#define CTR_FITERR_CLASSES 3
typedef struct ctr_fit_error {
  int32_t ndim;                    /* 2 or 3 */
  int32_t frame_dtype;             /* CTR_DTYPE_* */
  int32_t fit_function;            /* CTR_FIT_* */
  int32_t isotropic;               /* 1: one size column; 0: one per axis */
  int32_t n_profile;               /* profile parameters: gauss 0, ring and disc 1, inv_series_<N> N + 1 */
  int32_t want_cov;                /* 1: cov, var_row, var_col and their two offsets are given; 0: all NULL */
  int32_t max_grid;                /* > 0: a cap on every grid below the handle's; 0: the handle's */
  int32_t reserved0;
  int32_t modes[CTR_MAX_PARAMS];   /* CTR_MODE_CONST, _VAR or _CLUSTER per column */
  int64_t n_frames;                /* T */
  int64_t n_features;              /* N < 2^31 - 1 */
  int64_t n_clusters;              /* C */
  int64_t n_vars_total;            /* entries of var_row and var_col (want_cov) */
  int64_t n_cov_total;             /* entries of cov (want_cov) */
  int64_t shape[CTR_MAX_NDIM];     /* (z,) y, x of a frame */
  int64_t radius[CTR_MAX_NDIM];    /* of the masks, 1 .. 1024 */
  double residual_factor;          /* > 0 (default 1e5) */
  const void* frames;              /* [T, (z,) y, x] */
  const int64_t* frame_offset;     /* [T + 1] */
  const double* params;            /* [N, 2 + ndim + (isotropic ? 1 : ndim) + n_profile] */
  const double* mask_pos;          /* [N, ndim] or NULL */
  const int64_t* order;            /* [N] the rows sorted by (frame, cluster label), stable */
  const int64_t* cluster_offset;   /* [C + 1] the clusters' ranges in order */
  const int64_t* var_offset;       /* [C + 1] or NULL: the first variable of a cluster in var_row, var_col */
  const int64_t* cov_offset;       /* [C + 1] or NULL: the first entry of a cluster's n_vars x n_vars block in cov */
  double* params_std;              /* [N, n_params] out */
  int32_t* status;                 /* [N] out: CTR_FITERR_* of the row's cluster */
  int32_t* n_vars;                 /* [N] out: variables of the row's cluster */
  int64_t* n_pix;                  /* [N] out: P of the row's cluster */
  double* cov;                     /* [n_cov_total] out or NULL; NaN for a failed cluster */
  int64_t* var_row;                /* [n_vars_total] out or NULL: the table row of a variable, -1 for a cluster variable */
  int32_t* var_col;                /* [n_vars_total] out or NULL: its column */
} ctr_fit_error;
int ctr_fit_error_device(ctr_handle* h, const ctr_fit_error* e, void* hip_stream);
/* No device needed: the launch decision of ctr_fit_error_device from the scalars of e (its pointers
 * are not looked at) and the default cap of a handle: per size class (CTR_FITERR_CLASSES entries)
 * max_vars the most variables it takes, chunk the pixel rows [J | res] it stages at once and
 * lds_bytes its LDS request; grid the workgroups of a class's launch, scratch_bytes the scratch of
 * the call. */
int ctr_fit_error_plan(const ctr_fit_error* e, int32_t* max_vars, int32_t* chunk, int64_t* lds_bytes, int64_t* grid,
                       int64_t* scratch_bytes);

/* ---- refine from device tables: group, bound and lay out a batch (ABI 8, additions) ----
 * What refine_leastsq's host code does between the located features and ctr_refine_batch_device
 * (find_clusters, the stable sort by (frame, cluster), FitFunctions.feature_bounds, the feasibility
 * check of the box), on tables that stay in HBM; tests/_refine_arrays.py restates it in NumPy.
 * Input: pos [N, ndim], rows sorted by frame; frame_offset [T + 1], 0 = off[0] <= off[t] <=
 * off[t + 1] <= off[T] = N; params0 [N, n_params], start values in the column order of ctr_problem;
 * separation [ndim] > 0; the three bound templates of FitFunctions.validate_bounds, each
 * [2][CTR_MAX_PARAMS] (row 0 lower, row 1 upper; the first n_params of a row are used), NaN = none;
 * modes [n_params] as in ctr_problem.
 * CTR_PREPARE_BATCH:
 *   label [N]: the smallest row index of the row's cluster -- the rule of ctr_find_clusters: two rows
 *     of a frame are joined when the sum over the axes of ((pos_i - pos_j) / separation)^2, with
 *     pos / separation rounded first and every product rounded before it is added, is <= 1;
 *     clusters are the connected components.  cluster_size [N]: the rows of the row's cluster.
 *   order [N]: the input rows sorted by (frame, label), input order kept inside a cluster;
 *     feat_offset [C + 1] and frame_index [C]: the clusters' row ranges in that order and their
 *     frames (the caller gives room for N + 1 and N entries); n_clusters [1] = C.
 *   params, low, high [N, n_params], in that order: params a copy of params0;
 *     low  = fmax over the terms that are set of p - diff[0], p * (1 - rel[0]), abs[0],
 *     high = fmin over the terms that are set of p + diff[1], p * (1 + rel[1]), abs[1],
 *     every term one rounded operation on the row's own p (1 -+ rel rounded first), -inf / +inf
 *     where no term is set or the result is NaN (a NaN p); with neither diff nor rel set the
 *     absolute bound alone, whatever p.  No operation is contracted: the doubles are those of
 *     FitFunctions.feature_bounds bit for bit (the sign of a zero apart).
 *   status [2]: {CTR_PREPARE_OK, n_params}; {CTR_PREPARE_BAD_TABLE, n_params} when frame_offset is
 *     not as above (checked by the first kernel before any offset is followed; C = 0, nothing else
 *     is written); {CTR_PREPARE_INFEASIBLE, k} when a lower bound exceeds its upper bound, k the
 *     smallest such parameter: per row for CTR_MODE_VAR, after the min of the lows and the max of
 *     the highs over the cluster for the shared modes, never for CTR_MODE_CONST.
 *   Launches: a setup kernel over the rows; one workgroup of 256 threads per frame that labels
 *   (scaled positions in LDS tiles of 256 rows, so a frame of any row count; sweeps of
 *   take-the-smallest-label-of-a-neighbour-and-of-that-label until one changes nothing, at most
 *   rows + 1 of them), counts and ranks the rows; one workgroup that scans the clusters per frame;
 *   one workgroup per frame that writes the tables; a kernel over the clusters for the feasibility.
 *   Integer atomics only, no float sums.  Asynchronous; scratch (8 ndim + 12) N + 4 (T + 1) bytes of the handle
 *   (ctr_refine_prepare_plan gives the number without a device).
 * CTR_PREPARE_SCATTER: the fit's results back into input row order.  order, feat_offset as written
 *   above, n_clusters = C as read by the host; fit_params [N, n_params], fit_cost [C] and fit_std
 *   ([N, n_params] or NULL) are ctr_batch's params_out, cost and params_std; out params_out [N,
 *   n_params], cost_out [N] (the cost of the row's cluster), std_out (or NULL).  No scratch.
 * Descriptors are checked before the handle, as for ctr_characterize_device.  Device pointers. */
#define CTR_PREPARE_BATCH 0
#define CTR_PREPARE_SCATTER 1
#define CTR_PREPARE_OK 0
#define CTR_PREPARE_BAD_TABLE 1
#define CTR_PREPARE_INFEASIBLE 2
typedef struct ctr_refine_prepare {
  int32_t mode;                    /* CTR_PREPARE_BATCH or CTR_PREPARE_SCATTER */
  int32_t ndim;                    /* 2 or 3 */
  int32_t n_params;                /* 1 .. CTR_MAX_PARAMS */
  int32_t reserved0;
  int32_t modes[CTR_MAX_PARAMS];   /* CTR_MODE_* (BATCH) */
  int64_t n_frames;                /* T (BATCH) */
  int64_t n_features;              /* N < 2^31 - 1 */
  int64_t n_clusters;              /* C (SCATTER) */
  double separation[CTR_MAX_NDIM];
  double bound_abs[2 * CTR_MAX_PARAMS];   /* [2][CTR_MAX_PARAMS] */
  double bound_diff[2 * CTR_MAX_PARAMS];
  double bound_rel[2 * CTR_MAX_PARAMS];
  const double* pos;               /* [N, ndim]      (BATCH) */
  const int64_t* frame_offset;     /* [T + 1]        (BATCH) */
  const double* params0;           /* [N, n_params]  (BATCH) */
  int32_t* label;                  /* [N] out        (BATCH) */
  int32_t* cluster_size;           /* [N] out        (BATCH) */
  int32_t* order;                  /* [N]: BATCH out, SCATTER in */
  int32_t* feat_offset;            /* [N + 1], the first C + 1 used: BATCH out, SCATTER in */
  int32_t* frame_index;            /* [N], the first C used: out (BATCH) */
  int32_t* n_clusters_out;         /* [1] out        (BATCH) */
  double* params;                  /* [N, n_params] out (BATCH) */
  double* low;
  double* high;
  int32_t* status;                 /* [2] out        (BATCH) */
  const double* fit_params;        /* [N, n_params]  (SCATTER) */
  const double* fit_cost;          /* [C]            (SCATTER) */
  const double* fit_std;           /* [N, n_params] or NULL (SCATTER) */
  double* params_out;              /* [N, n_params] out (SCATTER) */
  double* cost_out;                /* [N] out        (SCATTER) */
  double* std_out;                 /* [N, n_params] out, with fit_std (SCATTER) */
} ctr_refine_prepare;
int ctr_refine_prepare_device(ctr_handle* h, const ctr_refine_prepare* r, void* hip_stream);
/* No device needed: the scratch of a call (0 for CTR_PREPARE_SCATTER). */
int ctr_refine_prepare_plan(const ctr_refine_prepare* r, int64_t* scratch_bytes);

/* A test switch: the most workgroups that a grid-stride kernel of the table stages is launched with
 * by every later stage call of this handle (refine_prepare, drift, msd / emsd, vanhove,
 * pair_correlation, neighbors, twopoint, cluster_tracks / track_positions, and the per-level refinement of
 * ctr_find_link_refine_device, whose fixed grid is lowered to it).  max_grid within [1, 65536], or
 * 0 for the default of 65536.  Returns the cap that held before; a null handle or a value outside
 * the range returns -1 and changes nothing.  A stage's results never depend on it: every such
 * kernel strides past its grid, and the suite lowers the cap to make small tables take those
 * further trips.  Not synchronised with calls of other threads on the same handle. */
int32_t ctr_set_stage_max_grid(ctr_handle* h, int32_t max_grid);

/* Has the last ctr_refine_batch_device call of this handle finished on the device?  1 yes (also
 * when there was none), 0 still running, -1 error.  Never blocks: lets a pipeline that keeps
 * several batches in flight hand finished batches on (e.g. to the result gather) from the host
 * without parking a stream in a device-side wait. */
int ctr_query_done(ctr_handle* h);

/* Block until the work queued by the *_device calls on `hip_stream` is done; NULL: the handle's
 * own stream and the refine call that was last queued for it. */
int ctr_synchronize(ctr_handle* h, void* hip_stream);

/* Later ctr_refine_batch_device calls on `device` use only the first n lanes (see "Lanes" above);
 * n within 1 .. the number of lanes, or 0 for all of them.  Returns the number in use before; -1,
 * and nothing changes, for a value outside the range or a device on which no handle lives.  Work
 * already queued stays where it is.  Results never depend on it: the suite runs the same calls on
 * one lane, on two and on all. */
int32_t ctr_set_lane_limit(int32_t device, int32_t n);

/* The inbox of a multi-GPU pipeline (one process per GPU): the rank that collects the result rows
 * allocates a block on its device and exports it; every other rank maps it and passes addresses
 * inside it as ctr_batch.result_rows / done_flag, so that the rows travel as peer stores over xGMI
 * while they are written -- no collective per batch (bench.py:open_inbox is the worked example).
 *   ctr_ipc_alloc: hipMalloc of `bytes` zeroed bytes on the handle's device + a blob of
 *     CTR_IPC_HANDLE_BYTES bytes to be sent to the other processes by any means: the HIP IPC
 *     handle followed by the PCI bus id of the owning device (ABI 6).
 *   ctr_ipc_open: maps such a block into this process for the handle's device
 *     (hipIpcOpenMemHandle with lazy peer access, called with that device current).  The owner
 *     named in the blob must be this device or one it has peer access to (hipDeviceCanAccessPeer),
 *     checked BEFORE anything is mapped; an owner this process cannot resolve is refused
 *     (CTR_ERR_DEVICE): the caller then gathers with a collective instead.
 *   ctr_ipc_probe: stores `value` at `dst` (8 bytes) FROM A KERNEL of the handle's device and
 *     waits for it: proves at set-up time that this device can write the mapped block.
 *   ctr_ipc_read: copies `bytes` from device / mapped memory to the host (blocking).
 *   ctr_ipc_close / ctr_ipc_free: unmap (importer) / release (owner, after every importer closed). */
#define CTR_IPC_HANDLE_BYTES 128
int ctr_ipc_alloc(ctr_handle* h, int64_t bytes, void** dev_ptr, unsigned char* handle_out);
int ctr_ipc_open(ctr_handle* h, const unsigned char* handle, void** dev_ptr);
int ctr_ipc_probe(ctr_handle* h, void* dst, int64_t value);
int ctr_ipc_read(ctr_handle* h, void* dst_host, const void* src, int64_t bytes);
int ctr_ipc_close(ctr_handle* h, void* dev_ptr);
int ctr_ipc_free(ctr_handle* h, void* dev_ptr);

/* Ordering with a caller's stream when the *_device calls run on the handle's own stream
 * (hip_stream = NULL above), without blocking the host.  `hip_stream` here is a hipStream_t
 * passed as void*; NULL means the legacy default stream (what PyTorch uses unless told
 * otherwise).
 *   ctr_engine_wait_stream: work queued later on the handle's stream -- the next refine call
 *     for it included, whose kernels run on the lanes -- starts only when everything queued so
 *     far on `hip_stream` has finished (inputs produced there).
 *   ctr_stream_wait_engine: work queued later on `hip_stream` starts only when everything
 *     queued so far on the handle's stream, and the refine call last queued for it, has finished
 *     (results consumed there). */
int ctr_engine_wait_stream(ctr_handle* h, void* hip_stream);
int ctr_stream_wait_engine(ctr_handle* h, void* hip_stream);

/* Timing of the kernels of the last ctr_refine_batch_device call, measured with HIP events at
 * the start of the call, after its frame maxima and at its end (milliseconds); synchronises. */
int ctr_last_kernel_ms(ctr_handle* h, double* frame_max_ms, double* refine_ms);

#ifdef __cplusplus
}
#endif
#endif /* CTREFINE_H */
