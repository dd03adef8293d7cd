// tu_msd.hip -- mean squared displacement of linked particles (ctr_msd_device, ctr_emsd_device;
// msd_kernels.h) and, on the same sorted rows, their van Hove displacement distributions
// (ctr_vanhove_device; vanhove_kernels.h): the descriptors' checks, the scratch and the queue of kernels.
#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "stage_common.h"
#include "msd_kernels.h"
#include "vanhove_kernels.h"

// what the two descriptors share; a static message, or null
const char* msd_scalars(int ndim, long long L, long long T, long long N, long long P, const double* mpp) {
  if (ndim != 2 && ndim != 3) return "ndim must be 2 or 3";
  if (L < 1) return "max_lagtime must be >= 1";
  if (T < 0 || N < 0 || P < 0) return "negative counts";
  if (L > 0x7ffffffdLL || T > 0x7ffffffdLL || N > 0x7fffffffLL || P > 0x7ffffffeLL)
    return "too many lags, frames, features or particles for one call";
  for (int d = 0; d < ndim; ++d)
    if (!std::isfinite(mpp[d])) return "mpp must be finite";
  return nullptr;
}

// the part of the scratch that both calls fill: the sorted rows and the row range of every id
struct MsdLayout { size_t code, key, spos, first, last; };

MsdLayout msd_layout(size_t& total, int ndim, long long N, long long P) {
  const size_t n = (size_t)(N > 0 ? N : 1), p = (size_t)(P > 0 ? P : 1);
  MsdLayout o;
  o.code = carve(total, sizeof(int) * n);
  o.key = carve(total, sizeof(int) * n);
  o.spos = carve(total, sizeof(double) * (size_t)ndim * n);
  o.first = carve(total, sizeof(int) * p);
  o.last = carve(total, sizeof(int) * p);      // right behind first: one memset for both
  return o;
}

// status zeroed, the check, the row ranges zeroed, the sorted rows
hipError_t msd_prepare(MsdArgs& a, const MsdLayout& o, const StageRun* stage) {
  char* scratch = (char*)stage->scratch;
  const hipStream_t s = stage->stream;
  a.code = (int*)(scratch + o.code);
  a.key = (int*)(scratch + o.key);
  a.spos = (double*)(scratch + o.spos);
  a.first = (int*)(scratch + o.first);
  a.last = (int*)(scratch + o.last);
  hipError_t e = hipMemsetAsync(a.status, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.first, 0, (size_t)((char*)a.last - (char*)a.first) + sizeof(int) * (size_t)(a.P > 0 ? a.P : 1), s);
  if (e != hipSuccess) return e;
  const dim3 block(MSD_THREADS);
  hipLaunchKernelGGL(msd_check_kernel, dim3(stride_grid(a.T + 1 > a.N ? a.T + 1 : a.N, MSD_THREADS, stage->max_grid)), block, 0, s, a);
  if (a.N > 0) hipLaunchKernelGGL(msd_rows_kernel, dim3(stride_grid(a.N, MSD_THREADS, stage->max_grid)), block, 0, s, a);
  return hipSuccess;
}

}  // namespace

int ctr_msd_launch(const ctr_msd* c, StageRun* stage, const char** msg) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (const char* why = msd_scalars(c->ndim, c->max_lagtime, c->n_frames, c->n_features, c->n_particles, c->mpp)) {
    *msg = why; return CTR_ERR_INVALID;
  }
  if (c->n_select < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (c->n_select > 0x7ffffffeLL) { *msg = "too many ids selected for one call"; return CTR_ERR_INVALID; }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!c->status || !c->frame_offset) { *msg = "null status or frame_offset"; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && (!c->particle || !c->pos || !c->order)) { *msg = "features without particle, pos or order"; return CTR_ERR_INVALID; }
  if (c->n_select > 0 && (!c->msd || !c->mean_d || !c->mean_d2 || !c->n)) { *msg = "null output"; return CTR_ERR_INVALID; }
  size_t total = 0;
  const MsdLayout o = msd_layout(total, c->ndim, c->n_features, c->n_particles);
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  MsdArgs a = {};
  a.ndim = c->ndim;
  a.L = c->max_lagtime; a.T = c->n_frames; a.N = c->n_features; a.P = c->n_particles; a.M = c->n_select;
  for (int d = 0; d < c->ndim; ++d) a.mpp[d] = c->mpp[d];
  a.frame_offset = (const long long*)c->frame_offset;
  a.particle = (const long long*)c->particle;
  a.order = (const long long*)c->order;
  a.select = (const long long*)c->select;
  a.pos = c->pos;
  a.msd = c->msd; a.mean_d = c->mean_d; a.mean_d2 = c->mean_d2; a.n = c->n;
  a.status = c->status;
  STAGE_TRY(msd_prepare(a, o, stage));
  if (a.M > 0) hipLaunchKernelGGL(msd_particle_kernel, dim3(frame_grid(a.M, stage->max_grid)), dim3(MSD_THREADS), 0, s, a);
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}

int ctr_emsd_launch(const ctr_emsd* c, StageRun* stage, const char** msg) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (const char* why = msd_scalars(c->ndim, c->max_lagtime, c->n_frames, c->n_features, c->n_particles, c->mpp)) {
    *msg = why; return CTR_ERR_INVALID;
  }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!c->status || !c->frame_offset) { *msg = "null status or frame_offset"; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && (!c->particle || !c->pos || !c->order)) { *msg = "features without particle, pos or order"; return CTR_ERR_INVALID; }
  if (!c->msd || !c->mean_d || !c->mean_d2 || !c->n) { *msg = "null output"; return CTR_ERR_INVALID; }
  const long long n_chunks = (c->n_particles + MSD_CHUNK - 1) / MSD_CHUNK;
  const size_t lags = (size_t)c->max_lagtime, parts = (size_t)(n_chunks > 0 ? n_chunks : 1);
  size_t total = 0;
  const MsdLayout o = msd_layout(total, c->ndim, c->n_features, c->n_particles);
  const size_t o_part = carve(total, sizeof(double) * 2 * (size_t)c->ndim * lags * parts);
  const size_t o_part_n = carve(total, sizeof(long long) * lags * parts);
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  MsdArgs a = {};
  a.ndim = c->ndim;
  a.L = c->max_lagtime; a.T = c->n_frames; a.N = c->n_features; a.P = c->n_particles;
  for (int d = 0; d < c->ndim; ++d) a.mpp[d] = c->mpp[d];
  a.frame_offset = (const long long*)c->frame_offset;
  a.particle = (const long long*)c->particle;
  a.order = (const long long*)c->order;
  a.pos = c->pos;
  a.part = (double*)((char*)stage->scratch + o_part);
  a.part_n = (long long*)((char*)stage->scratch + o_part_n);
  a.n_chunks = n_chunks;
  a.msd = c->msd; a.mean_d = c->mean_d; a.mean_d2 = c->mean_d2; a.n_pool = (long long*)c->n;
  a.status = c->status;
  STAGE_TRY(msd_prepare(a, o, stage));
  const dim3 block(MSD_THREADS);
  // few chunks: their lags are shared among workgroups until about MSD_FILL of them are in flight
  long long groups = n_chunks > 0 ? MSD_FILL / n_chunks : 1;
  groups = groups < 1 ? 1 : groups > a.L ? a.L : groups;
  a.lag_groups = groups;
  if (n_chunks > 0) hipLaunchKernelGGL(msd_chunk_kernel, dim3(frame_grid(n_chunks * groups, stage->max_grid)), block, 0, s, a);
  hipLaunchKernelGGL(msd_pool_kernel, dim3(stride_grid(a.L, MSD_THREADS, stage->max_grid)), block, 0, s, a);
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}

int ctr_vanhove_launch(const ctr_vanhove* c, StageRun* stage, const char** msg) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (c->ndim != 2 && c->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (c->n_lags < 1 || c->n_lags > CTR_VANHOVE_MAX_LAGS) { *msg = "n_lags must be within [1, 64]"; return CTR_ERR_INVALID; }
  for (int q = 0; q < c->n_lags; ++q)
    if (c->lag[q] < 1 || c->lag[q] > 0x7ffffffdLL || (q > 0 && c->lag[q] <= c->lag[q - 1])) {
      *msg = "lags must be ascending, >= 1 and <= 2^31 - 3"; return CTR_ERR_INVALID;
    }
  if (c->half_bins < 1 || c->half_bins > CTR_VANHOVE_MAX_HALF_BINS) { *msg = "half_bins must be within [1, 1024]"; return CTR_ERR_INVALID; }
  if (!std::isfinite(c->bin_width) || !(c->bin_width > 0.)) { *msg = "bin_width must be finite and positive"; return CTR_ERR_INVALID; }
  if (c->n_frames < 0 || c->n_features < 0 || c->n_particles < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (c->n_frames > 0x7ffffffdLL || c->n_features > 0x7fffffffLL || c->n_particles > 0x7ffffffeLL) {
    *msg = "too many frames, features or particles for one call"; return CTR_ERR_INVALID;
  }
  for (int d = 0; d < c->ndim; ++d)
    if (!std::isfinite(c->mpp[d])) { *msg = "mpp must be finite"; return CTR_ERR_INVALID; }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!c->status || !c->frame_offset) { *msg = "null status or frame_offset"; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && (!c->particle || !c->pos || !c->order)) { *msg = "features without particle, pos or order"; return CTR_ERR_INVALID; }
  if (!c->edges || !c->edge2) { *msg = "null edges or edge2"; return CTR_ERR_INVALID; }
  if (!c->count || !c->below || !c->above || !c->density || !c->count_r || !c->above_r || !c->density_r || !c->n ||
      !c->mean_d || !c->mean_d2 || !c->mean_d4 || !c->alpha2) { *msg = "null output"; return CTR_ERR_INVALID; }
  const long long n_chunks = (c->n_particles + MSD_CHUNK - 1) / MSD_CHUNK;
  const size_t lags = (size_t)c->n_lags, parts = (size_t)(n_chunks > 0 ? n_chunks : 1);
  size_t total = 0;
  const MsdLayout o = msd_layout(total, c->ndim, c->n_features, c->n_particles);
  const size_t o_part = carve(total, sizeof(double) * 3 * (size_t)c->ndim * lags * parts);
  const size_t o_part_n = carve(total, sizeof(long long) * lags * parts);
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  VanhoveArgs v = {};
  MsdArgs& a = v.t;
  a.ndim = c->ndim;
  a.T = c->n_frames; a.N = c->n_features; a.P = c->n_particles;
  for (int d = 0; d < c->ndim; ++d) a.mpp[d] = c->mpp[d];
  a.frame_offset = (const long long*)c->frame_offset;
  a.particle = (const long long*)c->particle;
  a.order = (const long long*)c->order;
  a.pos = c->pos;
  a.n_chunks = n_chunks;
  a.status = c->status;
  v.K = c->n_lags; v.H = (int)c->half_bins;
  for (int q = 0; q < c->n_lags; ++q) v.lag[q] = c->lag[q];
  v.bin_width = c->bin_width; v.inv_width = 1. / c->bin_width;
  v.edges = c->edges; v.edge2 = c->edge2;
  v.part = (double*)((char*)stage->scratch + o_part);
  v.part_n = (long long*)((char*)stage->scratch + o_part_n);
  v.count = (unsigned long long*)c->count; v.below = (unsigned long long*)c->below; v.above = (unsigned long long*)c->above;
  v.count_r = (unsigned long long*)c->count_r; v.above_r = (unsigned long long*)c->above_r;
  v.n = (long long*)c->n;
  v.density = c->density; v.density_r = c->density_r;
  v.mean_d = c->mean_d; v.mean_d2 = c->mean_d2; v.mean_d4 = c->mean_d4; v.alpha2 = c->alpha2;
  STAGE_TRY(msd_prepare(a, o, stage));
  const dim3 block(MSD_THREADS);
  hipLaunchKernelGGL(vanhove_clear_kernel, dim3(stride_grid((long long)v.K * a.ndim * 2 * v.H, MSD_THREADS, stage->max_grid)), block, 0, s, v);
  if (n_chunks > 0) hipLaunchKernelGGL(vanhove_bin_kernel, dim3(frame_grid(n_chunks * v.K, stage->max_grid)), block, 0, s, v);
  hipLaunchKernelGGL(vanhove_finish_kernel, dim3(frame_grid(v.K, stage->max_grid)), block, 0, s, v);
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
