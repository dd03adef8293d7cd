// tu_motion.hip -- orientation and diffusion tensor of tracked clusters (ctr_orientation_device,
// ctr_diffusion_device; motion_kernels.h).  No floating-point contraction: a row is
// the same bytes whether its later frame comes from LDS or from global memory.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "motion_kernels.h"

// LDS a workgroup of the diffusion kernel may take, as the other stages allow themselves
constexpr size_t MOT_LDS_MAX = 64 * 1024;
// frames behind the tile that fit beside it: (8192 - 96) / 12 - 256 = 418
constexpr int MOT_HALO_MAX = (int)((MOT_LDS_MAX / sizeof(double) - MOT_RED) / MOT_ROW) - MOT_TILE;

// The halo staged behind a tile: the frames that exist beyond the first tile, as many as fit.  It
// depends on n_frames alone (the lags are device memory, and the tiling must not depend on them):
// with n_frames <= MOT_TILE + MOT_HALO_MAX every later frame is in LDS, beyond that a row whose
// later frame lies past the staged ones reads it from global memory.
int mot_halo(long long n_frames) {
  const long long beyond = n_frames - MOT_TILE;
  return (int)(beyond < 0 ? 0 : beyond > MOT_HALO_MAX ? MOT_HALO_MAX : beyond);
}

size_t mot_lds_bytes(int halo) { return sizeof(double) * (MOT_RED + (size_t)MOT_ROW * (MOT_TILE + halo)); }

template <int ND>
void launch_orientation(int cs, const OriArgs& a, unsigned grid, hipStream_t s) {
  if (cs == 2) hipLaunchKernelGGL((orientation_kernel<ND, 2>), dim3(grid), dim3(MOT_THREADS), 0, s, a);
  else if (cs == 3) hipLaunchKernelGGL((orientation_kernel<ND, 3>), dim3(grid), dim3(MOT_THREADS), 0, s, a);
  else if (ND == 3) hipLaunchKernelGGL((orientation_kernel<3, 4>), dim3(grid), dim3(MOT_THREADS), 0, s, a);
}

}  // namespace

int ctr_orientation_launch(const ctr_orientation* o, StageRun* stage, const char** msg) {
  *msg = "";
  if (!o) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (o->ndim != 2 && o->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (o->cluster_size == 1) { *msg = "the orientation of a single particle is not implemented (cluster_size 1)"; return CTR_ERR_UNSUPPORTED; }
  if (o->cluster_size < 1 || o->cluster_size > 4) { *msg = "cluster_size must be 2, 3 or 4"; return CTR_ERR_INVALID; }
  if (o->ndim == 2 && o->cluster_size == 4) { *msg = "the orientation of a 2D tetramer is not implemented (nor in the reference)"; return CTR_ERR_UNSUPPORTED; }
  if (o->n_tracks < 0 || o->n_frames < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (!std::isfinite(o->mpp)) { *msg = "mpp must be finite"; return CTR_ERR_INVALID; }
  for (int k = 0; k < o->cluster_size; ++k)
    if (!std::isfinite(o->weights[k])) { *msg = "weights must be finite"; return CTR_ERR_INVALID; }
  if (o->ndim == 3 && o->cluster_size == 2 && !o->angles) { *msg = "angles is required for 3D dimers"; return CTR_ERR_INVALID; }
  const long long lim = (1LL << 31) - 1;
  if (o->n_tracks > lim || o->n_frames > lim || (o->n_frames > 0 && o->n_tracks > lim * MOT_THREADS / o->n_frames)) {
    *msg = "too many tracks or frames for one call";
    return CTR_ERR_INVALID;
  }
  const long long n = o->n_tracks * o->n_frames;
  if (n > 0 && (!o->pos || !o->com || !o->bases)) { *msg = "null input or output"; return CTR_ERR_INVALID; }
  if (stage->mode != STAGE_LAUNCH || n == 0) return CTR_OK;
  const hipStream_t s = stage->stream;
  OriArgs a;
  a.T = o->n_tracks;
  a.F = o->n_frames;
  a.mpp = o->mpp;
  for (int k = 0; k < 4; ++k) a.w[k] = k < o->cluster_size ? o->weights[k] : 0.;
  a.pos = o->pos;
  a.angles = o->angles;
  a.com = o->com;
  a.bases = o->bases;
  const unsigned grid = (unsigned)((n + MOT_THREADS - 1) / MOT_THREADS);
  if (o->ndim == 2) launch_orientation<2>(o->cluster_size, a, grid, s);
  else launch_orientation<3>(o->cluster_size, a, grid, s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}

int ctr_diffusion_launch(const ctr_diffusion* d, StageRun* stage, const char** msg) {
  *msg = "";
  if (!d) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (d->ndim != 2 && d->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (d->n_perm < 1 || d->n_perm > 4096) { *msg = "n_perm must be in [1, 4096]"; return CTR_ERR_INVALID; }
  if (d->n_tracks < 0 || d->n_frames < 0 || d->n_lags < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (!std::isfinite(d->fps) || !(d->fps > 0.)) { *msg = "fps must be positive"; return CTR_ERR_INVALID; }
  const long long lim = (1LL << 31) - 1;
  const long long n_tiles = (d->n_frames + MOT_TILE - 1) / MOT_TILE;
  if (d->n_tracks > lim || d->n_frames > lim || d->n_lags > lim) { *msg = "too many tracks, frames or lags for one call"; return CTR_ERR_INVALID; }
  // one workgroup per (track, permutation, tile) and per (track, lag); the partials in one block
  const long long per_track = (long long)d->n_perm * n_tiles;      // < 2^12 2^23
  if ((per_track > 0 && d->n_tracks > lim / per_track) || (d->n_lags > 0 && d->n_tracks > lim / d->n_lags)) {
    *msg = "too many tracks, frames or lags for one call";
    return CTR_ERR_INVALID;
  }
  const long long groups = d->n_tracks * per_track, outs = d->n_tracks * d->n_lags;
  if (groups > 0 && d->n_lags > (1LL << 40) / MOT_NSUM / groups) { *msg = "partial sums above 8 TiB"; return CTR_ERR_INVALID; }
  if (outs > 0 && (!d->lags || !d->tensor || !d->n_samples)) { *msg = "null lags or output"; return CTR_ERR_INVALID; }
  if (outs > 0 && groups > 0 && (!d->positions || !d->bases)) { *msg = "null input"; return CTR_ERR_INVALID; }
  stage->scratch_bytes = sizeof(double) * (size_t)(groups * d->n_lags * MOT_NSUM) + 256;
  if (stage->mode != STAGE_LAUNCH || outs == 0) return CTR_OK;
  const hipStream_t s = stage->stream;
  DifArgs a;
  a.ndim = d->ndim;
  a.n_perm = d->n_perm;
  a.halo = mot_halo(d->n_frames);
  a.T = d->n_tracks;
  a.F = d->n_frames;
  a.n_lags = d->n_lags;
  a.n_tiles = n_tiles;
  a.fps = d->fps;
  a.lags = (const long long*)d->lags;
  a.positions = d->positions;
  a.bases = d->bases;
  a.partial = (double*)stage->scratch;
  a.tensor = d->tensor;
  a.n_samples = (long long*)d->n_samples;
  if (groups > 0)
    hipLaunchKernelGGL(diffusion_partial_kernel, dim3((unsigned)groups), dim3(MOT_THREADS), mot_lds_bytes(a.halo), s, a);
  hipLaunchKernelGGL(diffusion_final_kernel, dim3((unsigned)outs), dim3(WAVE), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}
