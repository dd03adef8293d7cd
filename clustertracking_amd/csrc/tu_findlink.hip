// tu_findlink.hip -- find and link with relocation (ctr_find_link_device and, with the
// centre-of-mass refinement of every level, ctr_find_link_refine_device; findlink_kernels.h,
// DESIGN.md 7b).  Distances are compared with the host linker's and the relocation's: no
// floating-point contraction in this unit.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "stage_common.h"
#include "link_kernels.h"
#include "findlink_kernels.h"

// lays the scratch of a call out from `base` (nullptr: only the size is wanted; else the bytes at
// the front that every call zeroes): the linker's arrays over the padded table, then this stage's
size_t layout(FlArgs& a, char* base, int ndim, long long n_levels) {
  size_t at = lnk_layout(a.l, nullptr, a.ncap, ndim, n_levels);
  const size_t zeroed = base ? lnk_layout(a.l, base, a.ncap, ndim, n_levels) : 0;
  const size_t N = (size_t)a.ncap, L = (size_t)n_levels + 1, Q = (size_t)a.Q, K = (size_t)a.K, Z = (size_t)a.nsz;
  a.start = (long long*)(base + carve(at, L * sizeof(long long)));
  a.cnt = (int*)(base + carve(at, L * sizeof(int)));
  a.ppos = (double*)(base + carve(at, N * ndim * sizeof(double)));
  a.pmass = (double*)(base + carve(at, N * sizeof(double)));
  a.psignal = (double*)(base + carve(at, N * sizeof(double)));
  a.psize = (double*)(base + carve(at, N * Z * sizeof(double)));
  a.pparticle = (long long*)(base + carve(at, N * sizeof(long long)));
  int** per_row[] = {&a.preloc, &a.pquery, &a.sn_ns, &a.sn_nd, &a.mrg, &a.m_ns, &a.m_nd, &a.qof, &a.nmnb};
  for (int** p : per_row) *p = (int*)(base + carve(at, N * sizeof(int)));
  a.mnb = (int*)(base + carve(at, N * LNK_MAXC * sizeof(int)));
  a.q_soff = (long long*)(base + carve(at, (Q + 1) * sizeof(long long)));
  a.q_frame = (long long*)(base + carve(at, Q * sizeof(long long)));
  a.q_spos = (double*)(base + carve(at, Q * LNK_MAX_SRC * ndim * sizeof(double)));
  int** per_query[] = {&a.q_root, &a.q_short, &a.q_fill, &a.r_found, &a.r_status};
  for (int** p : per_query) *p = (int*)(base + carve(at, Q * sizeof(int)));
  a.n_q = (int*)(base + carve(at, sizeof(int)));
  a.r_pos = (int*)(base + carve(at, Q * K * ndim * sizeof(int)));
  a.r_mass = (double*)(base + carve(at, Q * K * sizeof(double)));
  a.r_signal = (double*)(base + carve(at, Q * K * sizeof(double)));
  a.r_size = (double*)(base + carve(at, Q * K * Z * sizeof(double)));
  a.claim = (int*)(base + carve(at, Q * K * sizeof(int)));
  return base ? zeroed : at;
}

// com (may be null): the rows of level t are refined in place in the table (ctr_refine_com_launch)
int refine_level(const FlArgs& a, const ctr_refine_com* com, int t, StageRun* sub, const char** msg) {
  if (!com) return CTR_OK;
  RefineComLevel level = {a.start + t, a.cnt + t, a.ncap, t, a.ppos, a.pmass, a.l.spos, {a.l.sr[0], a.l.sr[1], a.l.sr[2]}};
  return ctr_refine_com_launch(com, sub, msg, &level);
}

template <int ND>
int run(const FlArgs& a, const ctr_relocate& rel, const ctr_refine_com* com, const StageRun* stage, const char** msg) {
  const hipStream_t s = stage->stream;
  const unsigned rows = (unsigned)((a.ncap + LNK_THREADS - 1) / LNK_THREADS);
  hipLaunchKernelGGL(fl_start_kernel, dim3(1), dim3(LNK_THREADS), 0, s, a);
  hipLaunchKernelGGL(fl_fill_kernel<ND>, dim3(rows), dim3(LNK_THREADS), 0, s, a);
  // the host does not read the levels' sizes: a fixed grid strides over a level's rows
  const unsigned per_level = rows < 16u ? rows : 16u;
  StageRun sub = {STAGE_LAUNCH, s, nullptr, 0, stage->max_grid};
  int rc = refine_level(a, com, 0, &sub, msg);
  if (rc != CTR_OK) return rc;
  for (int t = 1; t < a.n_levels; ++t) {
    hipLaunchKernelGGL(link_cand_kernel<ND>, dim3(per_level), dim3(LNK_THREADS), 0, s, a.l, t, t + 1);
    hipLaunchKernelGGL(fl_merge_kernel<ND>, dim3(1), dim3(LNK_THREADS), 0, s, a, t);
    rc = ctr_relocate_launch(&rel, &sub, msg, nullptr, nullptr);
    if (rc != CTR_OK) return rc;
    hipLaunchKernelGGL(fl_solve_kernel<ND>, dim3(1), dim3(LNK_THREADS), 0, s, a, t);
    rc = refine_level(a, com, t, &sub, msg);
    if (rc != CTR_OK) return rc;
  }
  hipLaunchKernelGGL(link_rank_kernel<ND>, dim3(rows), dim3(LNK_THREADS), 0, s, a.l);
  if (com) hipLaunchKernelGGL(fl_birth_rank_kernel<ND>, dim3(rows), dim3(LNK_THREADS), 0, s, a);
  hipLaunchKernelGGL(link_scan_kernel, dim3(1), dim3(LNK_THREADS), 0, s, a.l);
  for (long long reach = 1; reach < a.n_levels - 1; reach *= 2)
    hipLaunchKernelGGL(link_jump_kernel, dim3(rows), dim3(LNK_THREADS), 0, s, a.l);
  hipLaunchKernelGGL(link_ids_kernel, dim3(rows), dim3(LNK_THREADS), 0, s, a.l);
  hipLaunchKernelGGL(fl_offsets_kernel, dim3(1), dim3(LNK_THREADS), 0, s, a);
  hipLaunchKernelGGL(fl_emit_kernel<ND>, dim3(rows), dim3(LNK_THREADS), 0, s, a);
  return CTR_OK;
}

// what both entry points run.  com (may be null): the refinement of every level
int find_link(const ctr_find_link* f, const ctr_refine_com* com, StageRun* stage, const char** msg) {
  *msg = "";
  if (!f) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (f->ndim != 2 && f->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (f->n_frames < 0 || f->n_located < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (f->memory < 0) { *msg = "memory must be >= 0"; return CTR_ERR_INVALID; }
  if (f->max_queries < 1 || f->max_queries > 1024) { *msg = "max_queries must be in [1, 1024]"; return CTR_ERR_INVALID; }
  if (f->max_relocated < 1 || f->max_relocated > 1024) { *msg = "max_relocated must be in [1, 1024]"; return CTR_ERR_INVALID; }
  if (f->n_frames > 0xfffffLL) { *msg = "too many frames for one call"; return CTR_ERR_INVALID; }
  const long long ncap = f->n_located + f->n_frames * (long long)f->max_relocated;
  if (ncap > 0x7ffffff0LL) { *msg = "too many features for one call"; return CTR_ERR_INVALID; }
  // the relocation's view of the same arguments: its own checks of shape, radius, separation,
  // search_range, minmass and scale_factor
  ctr_relocate rel = {};
  rel.ndim = f->ndim;
  rel.frame_dtype = f->frame_dtype;
  rel.n_frames = f->n_frames;
  double max_dist = 0.;
  for (int d = 0; d < f->ndim; ++d) {
    rel.shape[d] = f->shape[d];
    rel.radius[d] = f->radius[d];
    rel.separation[d] = f->separation[d];
    rel.search_range[d] = f->search_range[d];
  }
  rel.isotropic = f->isotropic;
  rel.max_candidates = LNK_MAX_SRC;     // a shortage is at most the sources of a sub-network
  rel.minmass = f->minmass;
  rel.scale_factor = f->scale_factor;
  StageRun scalars = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, stage->max_grid};
  const int rc = ctr_relocate_launch(&rel, &scalars, msg, nullptr, nullptr);
  if (rc != CTR_OK) return rc;
  for (int d = 0; d < f->ndim; ++d) {   // FindLinker.__init__ (find_link.py:766-781), as tu_relocate.hip
    const long long slr = (long long)(f->search_range[d] + (double)f->radius[d] + 1.);
    max_dist = std::max(max_dist, (double)(slr + f->radius[d] + 1) / f->search_range[d]);
  }
  if (com) {   // its own checks of max_iterations, shift_thresh and the window; then the shared fields
    StageRun com_scalars = {STAGE_CHECK_SCALARS, nullptr, nullptr, 0, stage->max_grid};
    const int rcc = ctr_refine_com_launch(com, &com_scalars, msg, nullptr);
    if (rcc != CTR_OK) return rcc;
    if (com->ndim != f->ndim) { *msg = "the refinement's ndim differs from the find-link descriptor's"; return CTR_ERR_INVALID; }
    if (com->n_frames != f->n_frames) { *msg = "the refinement's n_frames differs from the find-link descriptor's"; return CTR_ERR_INVALID; }
    for (int d = 0; d < f->ndim; ++d) {
      if (com->shape[d] != f->shape[d]) { *msg = "the refinement's shape differs from the find-link descriptor's"; return CTR_ERR_INVALID; }
      if (com->radius[d] != f->radius[d]) { *msg = "the refinement's radius differs from the find-link descriptor's"; return CTR_ERR_INVALID; }
    }
    if (f->n_frames > 0 && !com->frames) { *msg = "null frames of the refinement"; return CTR_ERR_INVALID; }
  }
  if (f->n_frames > 0 && !f->frame_offset) { *msg = "null frame_offset"; return CTR_ERR_INVALID; }
  if (f->n_located > 0 && (!f->pos || !f->mass || !f->signal || !f->size)) { *msg = "null table of located rows"; return CTR_ERR_INVALID; }
  if (f->n_frames > 0) {
    if (!f->frames || !f->threshold) { *msg = "null frames or threshold"; return CTR_ERR_INVALID; }
    if (f->capacity < f->n_located + (f->n_frames - 1) * (long long)f->max_relocated) { *msg = "capacity below n_located + (n_frames - 1) * max_relocated"; return CTR_ERR_INVALID; }
    if (!f->pos_out || !f->frame_offset_out || !f->particle || !f->mass_out || !f->signal_out || !f->size_out ||
        !f->relocated || !f->n_tracks || !f->coupled || !f->status) { *msg = "null output"; return CTR_ERR_INVALID; }
  }
  FlArgs a = {};
  a.ncap = ncap > 0 ? ncap : 1;
  a.Q = f->max_queries;
  a.R = f->max_relocated;
  a.K = rel.max_candidates;
  a.nsz = f->isotropic ? 1 : f->ndim;
  stage->scratch_bytes = f->n_frames > 0 ? layout(a, nullptr, f->ndim, f->n_frames) : 0;
  if (stage->mode != STAGE_LAUNCH || f->n_frames == 0) return CTR_OK;
  const hipStream_t s = stage->stream;
  const size_t zeroed = layout(a, (char*)stage->scratch, f->ndim, f->n_frames);
  if (hipMemsetAsync(stage->scratch, 0, zeroed, s) != hipSuccess ||
      hipMemsetAsync(f->status, 0, 4 * sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(f->n_tracks, 0, sizeof(int64_t), s) != hipSuccess ||
      hipMemsetAsync(f->coupled, 0, (size_t)f->n_frames * sizeof(int32_t), s) != hipSuccess) { *msg = "hipMemsetAsync failed"; return CTR_ERR_DEVICE; }
  a.n_levels = (int)f->n_frames;
  a.max_dist2 = max_dist * max_dist;
  a.loc_off = (const long long*)f->frame_offset;
  a.loc_pos = f->pos;
  a.loc_mass = f->mass;
  a.loc_signal = f->signal;
  a.loc_size = f->size;
  a.o_pos = f->pos_out;
  a.o_off = (long long*)f->frame_offset_out;
  a.o_particle = (long long*)f->particle;
  a.o_mass = f->mass_out;
  a.o_signal = f->signal_out;
  a.o_size = f->size_out;
  a.o_reloc = f->relocated;
  a.coupled = f->coupled;
  a.l.ndim = f->ndim;
  a.l.memory = f->memory < f->n_frames ? (int)f->memory : (int)f->n_frames;   // a longer memory reaches no further
  a.l.n_levels = a.n_levels;
  a.l.n = ncap;
  a.l.pos = a.ppos;
  a.l.off = a.start;
  for (int d = 0; d < 3; ++d) a.l.sr[d] = d < f->ndim ? f->search_range[d] : 1.;
  a.l.particle = a.pparticle;
  a.l.n_tracks = (long long*)f->n_tracks;
  a.l.status = f->status;
  // every level's relocation: max_queries queries of frame t over tables that fl_merge_kernel fills
  rel.frames = f->frames;
  rel.threshold = f->threshold;
  rel.n_known = f->n_located;
  rel.known_pos = f->pos;
  rel.known_offset = f->frame_offset;
  rel.n_queries = a.Q;
  rel.query_frame = (const int64_t*)a.q_frame;
  rel.source_offset = (const int64_t*)a.q_soff;
  rel.source_pos = a.q_spos;
  rel.n_found = a.r_found;
  rel.cand_pos = a.r_pos;
  rel.mass = a.r_mass;
  rel.signal = a.r_signal;
  rel.size = a.r_size;
  rel.status = a.r_status;
  const int rr = f->ndim == 2 ? run<2>(a, rel, com, stage, msg) : run<3>(a, rel, com, stage, msg);
  if (rr != CTR_OK) return rr;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}

}  // namespace

int ctr_find_link_launch(const ctr_find_link* f, StageRun* stage, const char** msg) {
  return find_link(f, nullptr, stage, msg);
}

int ctr_find_link_refine_launch(const FindLinkRefine* d, StageRun* stage, const char** msg) {
  *msg = "";
  if (!d || !d->f) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (!d->com) { *msg = "null refinement descriptor"; return CTR_ERR_INVALID; }
  return find_link(d->f, d->com, stage, msg);
}
