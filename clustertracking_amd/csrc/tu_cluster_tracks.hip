// tu_cluster_tracks.hip -- cluster tracks (ctr_cluster_tracks_device, ctr_track_positions_device;
// cluster_track_kernels.h): the descriptors' checks, the scratch layout, the round
// bound and the queue of rounds.
#include <cstdint>

#include "kargs.h"

namespace {

#include "stage_common.h"
#include "cluster_track_kernels.h"

int ceil_log2(long long n) {
  int l = 0;
  while ((1LL << l) < n) ++l;
  return l;
}

}  // namespace

int ctr_cluster_tracks_launch(const ctr_cluster_tracks* c, StageRun* stage, const char** msg, ctr_tracks_plan* plan) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (c->phase != CTR_TRACKS_PAIRS && c->phase != CTR_TRACKS_COMPONENTS) { *msg = "unknown phase"; return CTR_ERR_INVALID; }
  if (c->cluster_size < 2 || c->cluster_size > 4) { *msg = "cluster_size must be 2, 3 or 4"; return CTR_ERR_INVALID; }
  if (c->min_frames < 1) { *msg = "min_frames must be >= 1"; return CTR_ERR_INVALID; }
  if (c->check_every < 0) { *msg = "check_every must be >= 0"; return CTR_ERR_INVALID; }
  if (c->n_frames < 0 || c->n_features < 0 || c->n_particles < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (c->n_frames > 0x7ffffffeLL || c->n_features > 0x7fffffffLL || c->n_particles > 0x7ffffffeLL) {
    *msg = "too many frames, features or particles for one call"; return CTR_ERR_INVALID;
  }
  const long long P = c->n_particles, M = c->n_features * (c->cluster_size - 1);
  // a tree with an edge to another tree is merged within two rounds; one more round hooks nothing
  const int L = ceil_log2(P), R = 2 * L + 2, J = L + 1;
  const long long nb = (P + CTK_THREADS - 1) / CTK_THREADS;
  size_t total = 0;
  const size_t o_flags = carve(total, 4 * (size_t)R * (J + 1)), o_A = carve(total, 4 * (size_t)P), o_B = carve(total, 4 * (size_t)P),
               o_size = carve(total, 4 * (size_t)P), o_num = carve(total, 4 * (size_t)P), o_bs = carve(total, 4 * (size_t)(nb + 1));
  if (plan) { plan->scratch_bytes = (long long)total; plan->max_rounds = R; plan->jumps_per_round = J; }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!c->status) { *msg = "null status"; return CTR_ERR_INVALID; }
  if (M > 0 && !c->keys) { *msg = "features without keys"; return CTR_ERR_INVALID; }
  if (c->phase == CTR_TRACKS_PAIRS) {
    if (!c->frame_offset) { *msg = "null frame_offset"; return CTR_ERR_INVALID; }
    if (c->n_features > 0 && (!c->particle || !c->cluster)) { *msg = "features without particle or cluster"; return CTR_ERR_INVALID; }
  } else {
    if (!c->n_tracks) { *msg = "null n_tracks"; return CTR_ERR_INVALID; }
    if (P > 0 && !c->track_of_particle) { *msg = "particles without track_of_particle"; return CTR_ERR_INVALID; }
    if (P > 1 && !c->n_members) { *msg = "particles without n_members"; return CTR_ERR_INVALID; }
  }
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  char* ws = (char*)stage->scratch;
  CtkArgs a = {};
  a.cs = c->cluster_size;
  a.min_frames = c->min_frames;
  a.T = c->n_frames; a.N = c->n_features; a.P = P; a.M = M;
  a.frame_offset = (const long long*)c->frame_offset;
  a.particle = (const long long*)c->particle;
  a.cluster = (const long long*)c->cluster;
  a.keys = (long long*)c->keys;
  a.status = c->status;
  const dim3 block(CTK_THREADS);
  if (c->phase == CTR_TRACKS_PAIRS) {
    STAGE_TRY(hipMemsetAsync(c->status, 0, sizeof(int32_t), s));
    long long n = a.T + 1 > a.N ? a.T + 1 : a.N;
    n = M > n ? M : n;
    hipLaunchKernelGGL(ctk_setup_kernel, dim3(stride_grid(n, CTK_THREADS, stage->max_grid)), block, 0, s, a, 1);
    if (a.T > 0 && a.N > 0)
      hipLaunchKernelGGL(ctk_groups_kernel, dim3(frame_grid(a.T, stage->max_grid)), block, 0, s, a);
    STAGE_TRY(hipGetLastError());
    return CTR_OK;
  }
  a.flags = (int*)(ws + o_flags);
  a.A = (int*)(ws + o_A);
  a.B = (int*)(ws + o_B);
  a.size = (int*)(ws + o_size);
  a.num = (int*)(ws + o_num);
  a.blocksum = (int*)(ws + o_bs);
  a.R = R; a.J = J;
  a.track_of = c->track_of_particle;
  a.n_tracks = c->n_tracks;
  a.n_members = c->n_members;
  a.n_rounds = c->n_rounds;
  STAGE_TRY(hipMemsetAsync(ws + o_flags, 0, o_A - o_flags, s));
  const dim3 gP(stride_grid(P, CTK_THREADS, stage->max_grid)), gM(stride_grid(M, CTK_THREADS, stage->max_grid));
  hipLaunchKernelGGL(ctk_init_kernel, gP, block, 0, s, a);
  bool synced = false;
  for (int r = 0; r < R && M > 0 && P > 1; ++r) {
    hipLaunchKernelGGL(ctk_hook_kernel, gM, block, 0, s, a, r);
    for (int j = 0; j < J; ++j) hipLaunchKernelGGL(ctk_jump_kernel, gP, block, 0, s, a, r, j);
    if (c->check_every > 0 && (r + 1) % c->check_every == 0) {
      int hooked = 0;
      STAGE_TRY(hipMemcpyAsync(&hooked, a.flags + (size_t)r * (J + 1), sizeof(int), hipMemcpyDeviceToHost, s));
      STAGE_TRY(hipStreamSynchronize(s));
      synced = true;
      if (!hooked) break;
    }
  }
  hipLaunchKernelGGL(ctk_verify_kernel, dim3(stride_grid(M > P ? M : P, CTK_THREADS, stage->max_grid)), block, 0, s, a);
  hipLaunchKernelGGL(ctk_count_kernel, gP, block, 0, s, a);
  if (nb > 0) hipLaunchKernelGGL(ctk_blocksum_kernel, dim3((unsigned)nb), block, 0, s, a);
  hipLaunchKernelGGL(ctk_scan_kernel, dim3(1), block, 0, s, a, nb);
  if (nb > 0) hipLaunchKernelGGL(ctk_number_kernel, dim3((unsigned)nb), block, 0, s, a);
  hipLaunchKernelGGL(ctk_assign_kernel, gP, block, 0, s, a);
  STAGE_TRY(hipGetLastError());
  if (synced) STAGE_TRY(hipStreamSynchronize(s));
  return CTR_OK;
}

int ctr_track_positions_launch(const ctr_track_positions* p, StageRun* stage, const char** msg) {
  *msg = "";
  if (!p) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (p->ndim != 2 && p->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (p->cluster_size < 2 || p->cluster_size > 4) { *msg = "cluster_size must be 2, 3 or 4"; return CTR_ERR_INVALID; }
  if (p->n_frames < 0 || p->n_features < 0 || p->n_particles < 0 || p->n_tracks < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (p->n_frames > 0x7ffffffeLL || p->n_features > 0x7fffffffLL || p->n_particles > 0x7ffffffeLL) {
    *msg = "too many frames, features or particles for one call"; return CTR_ERR_INVALID;
  }
  if (2 * p->n_tracks > p->n_particles) { *msg = "more tracks than pairs of particles"; return CTR_ERR_INVALID; }
  if (p->n_tracks > 0 && p->n_frames > (1LL << 40) / (p->n_tracks * p->cluster_size * p->ndim)) {
    *msg = "more than 2^40 output values"; return CTR_ERR_INVALID;
  }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!p->status || !p->frame_offset) { *msg = "null status or frame_offset"; return CTR_ERR_INVALID; }
  if (p->n_features > 0 && (!p->particle || !p->pos)) { *msg = "features without particle or pos"; return CTR_ERR_INVALID; }
  if (p->n_particles > 0 && !p->track_of_particle) { *msg = "particles without track_of_particle"; return CTR_ERR_INVALID; }
  const long long cells = p->n_tracks * p->n_frames;
  if (cells > 0 && (!p->present || !p->pos_out)) { *msg = "null output"; return CTR_ERR_INVALID; }
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  CtkArgs a = {};
  a.cs = p->cluster_size; a.ndim = p->ndim;
  a.T = p->n_frames; a.N = p->n_features; a.P = p->n_particles; a.n_trk = p->n_tracks;
  a.frame_offset = (const long long*)p->frame_offset;
  a.particle = (const long long*)p->particle;
  a.track_in = p->track_of_particle;
  a.pos = p->pos;
  a.present = p->present;
  a.pos_out = p->pos_out;
  a.status = p->status;
  const dim3 block(CTK_THREADS);
  STAGE_TRY(hipMemsetAsync(p->status, 0, sizeof(int32_t), s));
  long long n = a.T + 1 > a.N ? a.T + 1 : a.N;
  n = a.P > n ? a.P : n;
  hipLaunchKernelGGL(ctk_setup_kernel, dim3(stride_grid(n, CTK_THREADS, stage->max_grid)), block, 0, s, a, 0);
  if (cells > 0) {
    const dim3 gT(frame_grid(a.T, stage->max_grid));
    hipLaunchKernelGGL(ctk_fill_kernel, dim3(stride_grid(cells * a.cs * a.ndim, CTK_THREADS, stage->max_grid)), block, 0, s, a);
    if (a.N > 0) {
      hipLaunchKernelGGL(ctk_present_kernel, gT, block, 0, s, a);
      hipLaunchKernelGGL(ctk_scatter_kernel, gT, block, 0, s, a);
    }
  }
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
