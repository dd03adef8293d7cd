// tu_neighbors.hip -- nearest neighbours and proximity of a feature table (ctr_neighbors_device;
// neighbors_kernels.h): the descriptor's checks, the scratch and the queue of kernels.
// A squared distance is compared with the limit that the host squared and with the distances kept:
// every product and sum rounds on its own, no floating-point contraction anywhere in this unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "stage_common.h"
#include "pair_walk.h"
#include "neighbors_kernels.h"

// a static message, or null
const char* nbr_scalars(const ctr_neighbors* c) {
  const char* too_many = "too many frames, features or particles for one call";
  if (const char* why = pair_scalars(c, too_many)) return why;
  if (c->k < 1 || c->k > CTR_NBR_MAX_K) return "k must be within 1 .. CTR_NBR_MAX_K";
  if (c->lag < 0) return "lag must be >= 0";
  if (c->n_particles < 0) return "negative counts";
  if (c->n_particles > 0x7ffffffeLL) return too_many;
  if (!(c->limit2 > 0.)) return "limit2 must be positive or +inf";
  return nullptr;
}

template <int K>
void nbr_pairs(unsigned grid, hipStream_t s, const NbrArgs& a) {
  hipLaunchKernelGGL(nbr_pairs_kernel<K>, dim3(grid), dim3(NBR_THREADS), 0, s, a);
}

}  // namespace

int ctr_neighbors_launch(const ctr_neighbors* c, StageRun* stage, const char** msg) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (const char* why = nbr_scalars(c)) { *msg = why; return CTR_ERR_INVALID; }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!c->status || !c->frame_offset) { *msg = "null status or frame_offset"; return CTR_ERR_INVALID; }
  if (const char* why = pair_columns(c)) { *msg = why; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && (!c->dist || !c->dist2 || !c->index || !c->count)) { *msg = "null output"; return CTR_ERR_INVALID; }
  if (c->n_particles > 0 && (!c->particle_min || !c->particle_min2)) { *msg = "a particle column without particle_min"; return CTR_ERR_INVALID; }
  if (c->n_particles > 0 && c->n_features > 0 && !c->particle) { *msg = "n_particles without particle"; return CTR_ERR_INVALID; }
  size_t total = 0, o_start;
  const long long max_items = pair_max_items(c, total, o_start);
  const size_t o_pkey = carve(total, sizeof(unsigned long long) * (size_t)c->n_particles);
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  NbrArgs a = {};
  a.tab = pair_table(c, stage->scratch, o_start);
  a.k = c->k; a.lag = c->lag; a.P = c->n_particles;
  a.limit2 = c->limit2;
  a.particle = (const long long*)c->particle;
  a.pkey = (unsigned long long*)((char*)stage->scratch + o_pkey);
  a.dist = c->dist; a.dist2 = c->dist2; a.index = (long long*)c->index; a.count = (long long*)c->count;
  a.particle_min = c->particle_min; a.particle_min2 = c->particle_min2;
  STAGE_TRY(hipMemsetAsync(c->status, 0, sizeof(int32_t), s));
  const dim3 block(NBR_THREADS);
  const long long defaults = c->n_features > a.P ? c->n_features : a.P;
  hipLaunchKernelGGL(nbr_check_kernel, dim3(stride_grid(c->n_frames + 1, NBR_THREADS, stage->max_grid)), block, 0, s, a);
  if (defaults > 0) hipLaunchKernelGGL(nbr_defaults_kernel, dim3(stride_grid(defaults, NBR_THREADS, stage->max_grid)), block, 0, s, a);
  hipLaunchKernelGGL(nbr_items_kernel, dim3(1), block, 0, s, a);
  if (max_items > 0) {
    const unsigned grid = frame_grid(max_items, stage->max_grid);
    if (a.k <= 1) nbr_pairs<1>(grid, s, a);
    else if (a.k <= 4) nbr_pairs<4>(grid, s, a);
    else nbr_pairs<CTR_NBR_MAX_K>(grid, s, a);
  }
  if (a.P > 0) hipLaunchKernelGGL(nbr_particles_kernel, dim3(stride_grid(a.P, NBR_THREADS, stage->max_grid)), block, 0, s, a);
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
