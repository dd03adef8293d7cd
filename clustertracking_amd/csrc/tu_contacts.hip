// tu_contacts.hip -- contact episodes and bond lifetimes of linked particles (ctr_contacts_device;
// contacts_kernels.h): the descriptor's checks, the scratch and the queue of kernels of
// the three phases.  A squared distance is compared with the limits that the host squared and kept as
// it is: every product and sum rounds on its own, no floating-point contraction anywhere in this unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "stage_common.h"
#include "pair_walk.h"
#include "contacts_kernels.h"

// a static message, or null
const char* cont_scalars(const ctr_contacts* c) {
  const char* too_many = "too many frames, features or particles for one call";
  if (c->phase != CTR_CON_COUNT && c->phase != CTR_CON_FILL && c->phase != CTR_CON_EPISODES) return "unknown phase";
  if (const char* why = pair_scalars(c, too_many)) return why;
  if (c->n_particles < 0 || c->max_entries < 0) return "negative counts";
  if (c->n_particles > 0x7fffffffLL) return too_many;
  if (c->max_entries > (1LL << 40)) return "more than 2^40 entries";
  if (c->gap < 0 || c->gap > 0x7fffffffLL) return "gap must be within 0 .. 2^31 - 1";
  if (!(c->on2 > 0.) || !(c->off2 >= c->on2) || !std::isfinite(c->off2)) return "0 < on2 <= off2 < inf";
  if (c->phase == CTR_CON_EPISODES && (c->max_lifetime < 1 || c->max_lifetime > CTR_CON_MAX_LIFETIME))
    return "max_lifetime must be within 1 .. CTR_CON_MAX_LIFETIME";
  return nullptr;
}

// the pointers that a phase follows; a static message, or null
const char* cont_columns(const ctr_contacts* c) {
  const long long N = c->n_features, P = c->n_particles, M = c->max_entries, T = c->n_frames;
  if (!c->status || !c->n_entries) return "null status or n_entries";
  if (P > 0 && (!c->first_seen || !c->last_seen)) return "particles without first_seen or last_seen";
  if (c->phase != CTR_CON_EPISODES) {
    if (!c->frame_offset || !c->entry_start) return "null frame_offset or entry_start";
    if (const char* why = pair_columns(c)) return why;
    if (N > 0 && !c->particle) return "features without particle";
  }
  if (c->phase != CTR_CON_COUNT && M > 0 && (!c->key || !c->frame || !c->d2)) return "entries without key, frame or d2";
  if (c->phase == CTR_CON_EPISODES) {
    if (M > 0 && (!c->a || !c->b || !c->first || !c->last || !c->lifetime || !c->n_seen || !c->left_open || !c->right_open ||
                  !c->min_d2 || !c->max_d2))
      return "entries without the episode columns";
    if (M > 0 && (!c->pair_a || !c->pair_b || !c->pair_episodes || !c->pair_frames || !c->pair_first || !c->pair_last))
      return "entries without the pair columns";
    if (T > 0 && (!c->formed || !c->broken || !c->active)) return "frames without formed, broken or active";
    if (!c->lifetime_count || !c->lifetime_above || !c->duplicates || !c->n_episodes || !c->n_pairs) return "null output";
  }
  return nullptr;
}

}  // namespace

int ctr_contacts_launch(const ctr_contacts* c, StageRun* stage, const char** msg, ctr_contacts_launch_plan* plan) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (const char* why = cont_scalars(c)) { *msg = why; return CTR_ERR_INVALID; }
  const long long N = c->n_features, P = c->n_particles, M = c->max_entries, T = c->n_frames, L = c->max_lifetime;
  const long long most = N > M ? N : M;
  size_t total = 0, o_start;
  const long long max_items = pair_max_items(c, total, o_start);
  const size_t o_diff = carve(total, sizeof(long long) * (size_t)(T + 1));
  const size_t o_sums = carve(total, sizeof(long long) * (size_t)(most / CONT_THREADS + 1));
  const size_t o_words = carve(total, sizeof(long long));
  size_t o_m[7];
  for (size_t& o : o_m) o = carve(total, sizeof(long long) * (size_t)M);
  const unsigned cap = stage->max_grid;
  const unsigned g_check = stride_grid(T + 1 > N ? T + 1 : N, CONT_THREADS, cap);
  const unsigned g_walk = max_items > 0 ? frame_grid(max_items, cap) : 0;
  const unsigned g_entries = stride_grid(M, CONT_THREADS, cap);
  const unsigned g_waves = stride_grid(M, CONT_WAVES, cap);
  if (plan) {
    plan->scratch_bytes = (long long)total;
    plan->scan_tiles[0] = (N + CONT_THREADS - 1) / CONT_THREADS;
    plan->scan_tiles[1] = (M + CONT_THREADS - 1) / CONT_THREADS;
    plan->grids[0] = g_check; plan->grids[1] = g_walk; plan->grids[2] = g_entries; plan->grids[3] = g_waves;
  }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (const char* why = cont_columns(c)) { *msg = why; return CTR_ERR_INVALID; }
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  char* ws = (char*)stage->scratch;
  ContArgs a = {};
  a.tab = pair_table(c, ws, o_start);
  a.P = P; a.gap = c->gap; a.L = L; a.M = M;
  a.on2 = c->on2; a.off2 = c->off2;
  a.particle = (const long long*)c->particle;
  a.entry_start = (long long*)c->entry_start;
  a.key = (long long*)c->key; a.frame = c->frame; a.d2 = c->d2;
  a.n_entries = (long long*)c->n_entries;
  a.first_seen = (long long*)c->first_seen; a.last_seen = (long long*)c->last_seen;
  a.diff = (long long*)(ws + o_diff);
  a.sums = (long long*)(ws + o_sums);
  a.n_chains = (long long*)(ws + o_words);
  a.chain_start = (long long*)(ws + o_m[0]); a.c_on = (long long*)(ws + o_m[1]); a.c_seen = (long long*)(ws + o_m[2]);
  a.c_min = (double*)(ws + o_m[3]); a.c_max = (double*)(ws + o_m[4]);
  a.ep_chain = (long long*)(ws + o_m[5]); a.pair_start = (long long*)(ws + o_m[6]);
  a.ep_a = (long long*)c->a; a.ep_b = (long long*)c->b; a.ep_first = (long long*)c->first; a.ep_last = (long long*)c->last;
  a.ep_lifetime = (long long*)c->lifetime; a.ep_seen = (long long*)c->n_seen;
  a.ep_left = c->left_open; a.ep_right = c->right_open; a.ep_min = c->min_d2; a.ep_max = c->max_d2;
  a.pair_a = (long long*)c->pair_a; a.pair_b = (long long*)c->pair_b; a.pair_episodes = (long long*)c->pair_episodes;
  a.pair_frames = (long long*)c->pair_frames; a.pair_first = (long long*)c->pair_first; a.pair_last = (long long*)c->pair_last;
  a.formed = (long long*)c->formed; a.broken = (long long*)c->broken; a.active = (long long*)c->active;
  a.lifetime_count = (long long*)c->lifetime_count; a.lifetime_above = (long long*)c->lifetime_above;
  a.duplicates = (long long*)c->duplicates; a.n_episodes = (long long*)c->n_episodes; a.n_pairs = (long long*)c->n_pairs;

  const dim3 block(CONT_THREADS);
  // the three launches of a scan over at most n values (stage_common.h: grid_scan_*)
  auto scan = [&](int which, long long n) {
    const dim3 grid(stride_grid((n + CONT_THREADS - 1) / CONT_THREADS, 1, cap));
    hipLaunchKernelGGL(cont_scan_sums_kernel, grid, block, 0, s, a, which);
    hipLaunchKernelGGL(cont_scan_top_kernel, dim3(1), block, 0, s, a, which);
    hipLaunchKernelGGL(cont_scan_apply_kernel, grid, block, 0, s, a, which);
  };
  if (c->phase == CTR_CON_COUNT) {
    STAGE_TRY(hipMemsetAsync(c->status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(cont_check_kernel, dim3(g_check), block, 0, s, a);
    hipLaunchKernelGGL(cont_count_defaults_kernel, dim3(stride_grid(N + 1 > P ? N + 1 : P, CONT_THREADS, cap)), block, 0, s, a);
    hipLaunchKernelGGL(cont_items_kernel, dim3(1), block, 0, s, a);
    if (g_walk > 0) hipLaunchKernelGGL(cont_count_kernel, dim3(g_walk), block, 0, s, a);
    scan(CONT_SCAN_ROWS, N);
  } else if (c->phase == CTR_CON_FILL) {
    hipLaunchKernelGGL(cont_fill_defaults_kernel, dim3(stride_grid(M > P ? M : P, CONT_THREADS, cap)), block, 0, s, a);
    hipLaunchKernelGGL(cont_items_kernel, dim3(1), block, 0, s, a);
    if (g_walk > 0 && M > 0) hipLaunchKernelGGL(cont_fill_kernel, dim3(g_walk), block, 0, s, a);
  } else {
    long long n = M > T + 1 ? M : T + 1;
    n = 2 * L > n ? 2 * L : n;
    hipLaunchKernelGGL(cont_episode_defaults_kernel, dim3(stride_grid(n, CONT_THREADS, cap)), block, 0, s, a);
    if (M > 0 && P > 0) {
      scan(CONT_SCAN_HEADS, M);
      hipLaunchKernelGGL(cont_chains_kernel, dim3(g_waves), block, 0, s, a);
      scan(CONT_SCAN_CHAINS, M);
      hipLaunchKernelGGL(cont_episodes_kernel, dim3(g_entries), block, 0, s, a);
      scan(CONT_SCAN_PAIRS, M);
      hipLaunchKernelGGL(cont_pairs_kernel, dim3(g_waves), block, 0, s, a);
      if (T > 0) hipLaunchKernelGGL(cont_active_kernel, dim3(1), block, 0, s, a);
    }
  }
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
