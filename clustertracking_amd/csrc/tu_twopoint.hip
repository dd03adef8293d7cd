// tu_twopoint.hip -- two-point displacement correlations of linked particles (ctr_twopoint_device;
// twopoint_kernels.h): the descriptor's checks, the unit of the fixed point, the scratch
// and the queue of kernels.  The products and sums of a pair are rounded one by one, as the rule and
// its restatement have them: no floating-point contraction anywhere in this unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "stage_common.h"
#include "pair_walk.h"
#include "particle_match.h"
#include "twopoint_kernels.h"

// a static message, or null
const char* twopt_scalars(const ctr_twopoint* c) {
  const char* too_many = "too many frames, features or particles for one call";
  if (const char* why = pair_scalars(c, too_many)) return why;
  if (c->n_lags < 1 || c->n_lags > CTR_TP_MAX_LAGS) return "n_lags must be within 1 .. CTR_TP_MAX_LAGS";
  for (int k = 0; k < c->n_lags; ++k) {
    if (c->lag[k] < 1 || c->lag[k] > 0x7ffffffdLL) return "a lag must be within 1 .. 2^31 - 3";
    if (k > 0 && c->lag[k] <= c->lag[k - 1]) return "the lags must be ascending and distinct";
  }
  if (c->n_bins < 1) return "n_bins must be >= 1";
  if (c->n_bins > CTR_TP_MAX_BINS) return "more than CTR_TP_MAX_BINS bins";
  if (!std::isfinite(c->dr) || !(c->dr > 0.)) return "dr must be finite and positive";
  if (c->n_particles < 0) return "negative counts";
  if (c->n_particles > 0x7ffffffeLL) return too_many;
  if (!(c->max2 >= std::ldexp(1., -500) && c->max2 <= std::ldexp(1., 500))) return "max2 must be within [2^-500, 2^500]";
  // |a_i a_j| <= u2 d2 < max2 edge2[B], and u2_i u2_j <= max2^2: every product of a pair stays finite and
  // every integer of clause 8 below 2^41
  const double reach = (double)c->n_bins * c->dr;
  if (!((reach * reach) * c->max2 <= std::ldexp(1., 1000))) return "cutoff squared times max2 must be at most 2^1000";
  return nullptr;
}

// clause 8: the smallest integer e with 2^e >= max2
int twopt_exponent(double max2) {
  int x;
  const double m = std::frexp(max2, &x);       // max2 = m * 2^x, m in [0.5, 1)
  return m == 0.5 ? x - 1 : x;
}

}  // namespace

int ctr_twopoint_launch(const ctr_twopoint* c, StageRun* stage, const char** msg) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (const char* why = twopt_scalars(c)) { *msg = why; return CTR_ERR_INVALID; }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (!c->status || !c->frame_offset) { *msg = "null status or frame_offset"; return CTR_ERR_INVALID; }
  if (!c->edge2) { *msg = "null edge2"; return CTR_ERR_INVALID; }
  if (const char* why = pair_columns(c)) { *msg = why; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && !c->particle) { *msg = "features without particle"; return CTR_ERR_INVALID; }
  if (!c->n || !c->dot || !c->longitudinal || !c->transverse || !c->cos || !c->sums || !c->n_moved || !c->beyond) {
    *msg = "null output"; return CTR_ERR_INVALID;
  }
  size_t total = 0, o_start;
  const long long max_items = pair_max_items(c, total, o_start);
  const size_t o_partner = carve(total, sizeof(int) * (size_t)c->n_lags * (size_t)c->n_features);
  stage->scratch_bytes = total;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;

  const hipStream_t s = stage->stream;
  TwoptArgs a = {};
  a.tab = pair_table(c, stage->scratch, o_start);
  a.K = c->n_lags; a.B = c->n_bins; a.P = c->n_particles;
  for (int k = 0; k < a.K; ++k) a.lag[k] = c->lag[k];
  a.dr = c->dr; a.max2 = c->max2;
  const int e = twopt_exponent(c->max2);
  a.unit = std::ldexp(1., e - 40); a.inv_unit = std::ldexp(1., 40 - e);
  a.particle = (const long long*)c->particle;
  a.edge2 = c->edge2;
  a.partner = (int*)((char*)stage->scratch + o_partner);
  a.n = (long long*)c->n; a.dot = c->dot; a.longitudinal = c->longitudinal; a.transverse = c->transverse; a.cosine = c->cos;
  a.sums = (long long*)c->sums; a.n_moved = (long long*)c->n_moved; a.beyond = (long long*)c->beyond;
  const long long T = c->n_frames, N = c->n_features, cells = (long long)a.K * a.B;
  STAGE_TRY(hipMemsetAsync(c->status, 0, sizeof(int32_t), s));
  const dim3 block(TP_THREADS);
  hipLaunchKernelGGL(twopt_check_kernel, dim3(stride_grid(T + 1 > N ? T + 1 : N, TP_THREADS, stage->max_grid)), block, 0, s, a);
  hipLaunchKernelGGL(twopt_defaults_kernel, dim3(stride_grid(cells * TP_SUMS * 2, TP_THREADS, stage->max_grid)), block, 0, s, a);
  if (T > 0) hipLaunchKernelGGL(twopt_partner_kernel, dim3(frame_grid(a.K * T, stage->max_grid)), block, 0, s, a);
  hipLaunchKernelGGL(twopt_items_kernel, dim3(1), block, 0, s, a);
  if (max_items > 0) hipLaunchKernelGGL(twopt_pairs_kernel, dim3(frame_grid(a.K * max_items, stage->max_grid)), block, 0, s, a);
  hipLaunchKernelGGL(twopt_finish_kernel, dim3(stride_grid(cells, TP_THREADS, stage->max_grid)), block, 0, s, a);
  STAGE_TRY(hipGetLastError());
  return CTR_OK;
}
