// tu_shape.hip -- shape coordinates of tracked clusters (ctr_shape_device, ctr_shape_dynamics_device,
// ctr_shape_histogram_device, ctr_shape_plan; shape_kernels.h).  No floating-point
// contraction: bonds and the radius of gyration are NumPy's doubles, and a row is the same bytes
// whether its later frame comes from LDS or from global memory.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "shape_kernels.h"

// LDS a workgroup of the dynamics kernel may take, as the other stages allow themselves
constexpr size_t SHP_LDS_MAX = 64 * 1024;

// The most frames staged behind a tile of C coordinates: as many as fit beside the tile, and at
// most SHP_HALO_CAP (a tile never stages more than four tiles' worth): 768, 768, 158 for C = 2, 7, 19.
int shp_halo_max(int C) {
  const int fit = (int)((SHP_LDS_MAX / sizeof(double) - SHP_RED) / C) - SHP_TILE;
  return fit < SHP_HALO_CAP ? fit : SHP_HALO_CAP;
}

// The halo staged behind a tile: the frames that exist beyond the first tile, up to shp_halo_max.
// It depends on n_frames and C alone (the lags are device memory, and the tiling must not depend on
// them): a row whose later frame lies past the staged ones reads it from global memory.
int shp_halo(long long n_frames, int C) {
  const long long beyond = n_frames - SHP_TILE, most = shp_halo_max(C);
  return (int)(beyond < 0 ? 0 : beyond > most ? most : beyond);
}

size_t shp_lds_bytes(int halo, int C) { return sizeof(double) * (SHP_RED + (size_t)C * (SHP_TILE + halo)); }

template <int ND>
void launch_coords(int cs, const ShpCoordArgs& a, unsigned grid, hipStream_t s) {
  if (cs == 2) hipLaunchKernelGGL((shape_coords_kernel<ND, 2>), dim3(grid), dim3(SHP_THREADS), 0, s, a);
  else if (cs == 3) hipLaunchKernelGGL((shape_coords_kernel<ND, 3>), dim3(grid), dim3(SHP_THREADS), 0, s, a);
  else hipLaunchKernelGGL((shape_coords_kernel<ND, 4>), dim3(grid), dim3(SHP_THREADS), 0, s, a);
}

// the coordinates of all T F frames: into the public block (major = false) or coordinate-major
void queue_coords(int ndim, int cs, long long n, const double* mpp, const double* pos, double* out, bool major, hipStream_t s) {
  ShpCoordArgs a;
  a.n = n;
  for (int k = 0; k < 3; ++k) a.mpp[k] = k < ndim ? mpp[k] : 1.;
  a.pos = pos;
  a.out = out;
  a.cstride = major ? n : 1;
  a.fstride = major ? 1 : shp_nc(cs);
  const unsigned grid = (unsigned)((n + SHP_THREADS - 1) / SHP_THREADS);
  if (ndim == 2) launch_coords<2>(cs, a, grid, s);
  else launch_coords<3>(cs, a, grid, s);
}

// what the three descriptors share; n = T F on success
const char* check_block(int ndim, int cs, long long T, long long F, const double* mpp) {
  if (ndim != 2 && ndim != 3) return "ndim must be 2 or 3";
  if (cs < 2 || cs > 4) return "cluster_size must be 2, 3 or 4";
  if (T < 0 || F < 0) return "negative counts";
  for (int k = 0; k < ndim; ++k)
    if (!std::isfinite(mpp[k])) return "mpp must be finite";
  const long long lim = (1LL << 31) - 1;
  // T F C < 2^38: every index is an int64 far from its end, and T F / 256 workgroups fit a grid
  if (T > lim || F > lim || (F > 0 && T > (1LL << 33) / F)) return "too many tracks or frames for one call";
  return nullptr;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

int ctr_shape_launch(const ctr_shape* o, StageRun* stage, const char** msg) {
  *msg = "";
  if (!o) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (const char* why = check_block(o->ndim, o->cluster_size, o->n_tracks, o->n_frames, o->mpp)) { *msg = why; return CTR_ERR_INVALID; }
  const long long n = o->n_tracks * o->n_frames;
  if (n > 0 && (!o->pos || !o->coords)) { *msg = "null input or output"; return CTR_ERR_INVALID; }
  if (stage->mode != STAGE_LAUNCH || n == 0) return CTR_OK;
  queue_coords(o->ndim, o->cluster_size, n, o->mpp, o->pos, o->coords, false, stage->stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}

int ctr_shape_dynamics_launch(const ctr_shape_dynamics* d, StageRun* stage, const char** msg, ctr_shape_launch_plan* plan) {
  *msg = "";
  if (!d) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (const char* why = check_block(d->ndim, d->cluster_size, d->n_tracks, d->n_frames, d->mpp)) { *msg = why; return CTR_ERR_INVALID; }
  if (d->n_lags < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (!std::isfinite(d->fps) || !(d->fps > 0.)) { *msg = "fps must be positive"; return CTR_ERR_INVALID; }
  const int C = shp_nc(d->cluster_size);
  const long long T = d->n_tracks, F = d->n_frames, L = d->n_lags;
  const long long n = T * F, n_tiles = (F + SHP_TILE - 1) / SHP_TILE;
  const long long groups = T * n_tiles;                  // <= T F < 2^34
  const long long lim = (1LL << 31) - 1;
  if (L > lim || groups > lim || T > lim / C || (L > 0 && (T > lim / C / L || groups > (1LL << 36) / C / L))) {
    *msg = "too many tracks, frames or lags for one call";
    return CTR_ERR_INVALID;
  }
  const int halo = shp_halo(F, C);
  const size_t q_bytes = align256(sizeof(double) * (size_t)n * C);
  const size_t part_bytes = sizeof(double) * (size_t)(groups * L * C * SHP_NSUM);
  const size_t scratch = q_bytes + part_bytes + sizeof(double) * (size_t)(T * C * L * SHP_NSUM) + 256;
  if (plan) {
    plan->tile = SHP_TILE;
    plan->halo = halo;
    plan->lds_bytes = (long long)shp_lds_bytes(halo, C);
    plan->n_tiles = n_tiles;
    plan->scratch_bytes = (long long)scratch;
  }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  if (T * C * L > 0 && (!d->lags || !d->n || !d->mean_d || !d->mean_d2 || !d->mean_d4 || !d->flex)) { *msg = "null lags or output"; return CTR_ERR_INVALID; }
  if (C * L > 0 && (!d->pooled_n || !d->pooled_mean_d || !d->pooled_mean_d2 || !d->pooled_mean_d4 || !d->pooled_flex)) { *msg = "null pooled output"; return CTR_ERR_INVALID; }
  if (T > 0 && (!d->count || !d->mean || !d->var || !d->min || !d->max)) { *msg = "null moments output"; return CTR_ERR_INVALID; }
  if (n > 0 && !d->pos) { *msg = "null input"; return CTR_ERR_INVALID; }
  stage->scratch_bytes = scratch;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;
  const hipStream_t s = stage->stream;
  ShpDynArgs a;
  a.C = C;
  a.halo = halo;
  a.T = T;
  a.F = F;
  a.n_lags = L;
  a.n_tiles = n_tiles;
  a.fps = d->fps;
  a.lags = (const long long*)d->lags;
  a.q = (const double*)stage->scratch;
  a.partial = (double*)((char*)stage->scratch + q_bytes);
  a.track_sums = (double*)((char*)stage->scratch + q_bytes + part_bytes);
  a.n = (long long*)d->n;
  a.mean_d = d->mean_d; a.mean_d2 = d->mean_d2; a.mean_d4 = d->mean_d4; a.flex = d->flex;
  a.pooled_n = (long long*)d->pooled_n;
  a.pooled_mean_d = d->pooled_mean_d; a.pooled_mean_d2 = d->pooled_mean_d2; a.pooled_mean_d4 = d->pooled_mean_d4;
  a.pooled_flex = d->pooled_flex;
  a.count = (long long*)d->count;
  a.mean = d->mean; a.var = d->var; a.min = d->min; a.max = d->max;
  if (n > 0) queue_coords(d->ndim, d->cluster_size, n, d->mpp, d->pos, (double*)stage->scratch, true, s);
  if (groups > 0 && L > 0)
    hipLaunchKernelGGL(shape_partial_kernel, dim3((unsigned)groups), dim3(SHP_THREADS), shp_lds_bytes(halo, C), s, a);
  if (T * C * L > 0)
    hipLaunchKernelGGL(shape_final_kernel, dim3((unsigned)((T * C * L + SHP_THREADS - 1) / SHP_THREADS)), dim3(SHP_THREADS), 0, s, a);
  if (C * L > 0)
    hipLaunchKernelGGL(shape_pool_kernel, dim3((unsigned)((C * L + SHP_THREADS - 1) / SHP_THREADS)), dim3(SHP_THREADS), 0, s, a);
  if (T > 0)
    hipLaunchKernelGGL(shape_moments_kernel, dim3((unsigned)(T * C)), dim3(SHP_THREADS), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}

int ctr_shape_histogram_launch(const ctr_shape_histogram* d, StageRun* stage, const char** msg) {
  *msg = "";
  if (!d) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (const char* why = check_block(d->ndim, d->cluster_size, d->n_tracks, d->n_frames, d->mpp)) { *msg = why; return CTR_ERR_INVALID; }
  if (d->bond_bins < 1 || d->bond_bins > CTR_SHAPE_MAX_BOND_BINS) { *msg = "bond_bins must be in [1, 4096]"; return CTR_ERR_INVALID; }
  if (d->angle_bins < 1 || d->angle_bins > CTR_SHAPE_MAX_ANGLE_BINS) { *msg = "angle_bins must be in [1, 1024]"; return CTR_ERR_INVALID; }
  if (!std::isfinite(d->bond_dr) || !(d->bond_dr > 0.)) { *msg = "bond_dr must be positive"; return CTR_ERR_INVALID; }
  if (!std::isfinite(d->angle_width) || !(d->angle_width > 0.)) { *msg = "angle_width must be positive"; return CTR_ERR_INVALID; }
  if (d->per_track != 0 && d->per_track != 1) { *msg = "per_track must be 0 or 1"; return CTR_ERR_INVALID; }
  const int cs = d->cluster_size, C = shp_nc(cs), NB = shp_nb(cs), NA = shp_na(cs);
  const long long T = d->n_tracks, F = d->n_frames, n = T * F;
  const long long G = d->per_track ? T : 1, FG = d->per_track ? F : n;
  const long long chunks = (FG + SHP_HIST_CHUNK - 1) / SHP_HIST_CHUNK;
  const long long B = d->bond_bins, A = d->angle_bins;
  const long long lim = (1LL << 31) - 1;
  // the tables of per_track: G (7 * 4096 + 12 * 1024) cells at the most
  if (G * C * chunks > lim || G > (1LL << 36) / ((NB + 1) * B + NA * A)) { *msg = "too many tracks or frames for one call"; return CTR_ERR_INVALID; }
  if (!d->bond_edges || !d->angle_edges) { *msg = "null edges"; return CTR_ERR_INVALID; }
  if (G > 0 && (!d->count_bond || !d->above || !d->n || !d->density_bond)) { *msg = "null output"; return CTR_ERR_INVALID; }
  if (G > 0 && NA > 0 && (!d->count_angle || !d->density_angle)) { *msg = "null output"; return CTR_ERR_INVALID; }
  if (n > 0 && !d->pos) { *msg = "null input"; return CTR_ERR_INVALID; }
  if (G == 0) return CTR_OK;                              // no table to write: no scratch, nothing to launch
  stage->scratch_bytes = align256(sizeof(double) * (size_t)n * C) + 256;
  if (stage->mode != STAGE_LAUNCH) return CTR_OK;
  const hipStream_t s = stage->stream;
  ShpHistArgs a;
  a.C = C; a.NB = NB; a.NA = NA;
  a.TF = n; a.G = G; a.FG = FG; a.chunks = chunks;
  a.B = (int)B; a.A = (int)A;
  a.inv_dr = 1. / d->bond_dr;
  a.inv_da = 1. / d->angle_width;
  a.bond_dr = d->bond_dr;
  a.angle_width = d->angle_width;
  a.q = (const double*)stage->scratch;
  a.bond_edges = d->bond_edges;
  a.angle_edges = d->angle_edges;
  a.count_bond = (unsigned long long*)d->count_bond;
  a.above = (unsigned long long*)d->above;
  a.count_angle = (unsigned long long*)d->count_angle;
  a.n = (unsigned long long*)d->n;
  a.density_bond = d->density_bond;
  a.density_angle = d->density_angle;
  hipError_t e = hipMemsetAsync(d->count_bond, 0, sizeof(int64_t) * (size_t)(G * (NB + 1) * B), s);
  if (e == hipSuccess) e = hipMemsetAsync(d->above, 0, sizeof(int64_t) * (size_t)(G * (NB + 1)), s);
  if (e == hipSuccess && NA > 0) e = hipMemsetAsync(d->count_angle, 0, sizeof(int64_t) * (size_t)(G * NA * A), s);
  if (e == hipSuccess) e = hipMemsetAsync(d->n, 0, sizeof(int64_t) * (size_t)G, s);
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  if (n > 0) {
    queue_coords(d->ndim, cs, n, d->mpp, d->pos, (double*)stage->scratch, true, s);
    hipLaunchKernelGGL(shape_hist_kernel, dim3((unsigned)(G * C * chunks)), dim3(SHP_THREADS), 0, s, a);
  }
  const long long cells = G * ((NB + 1) * B + NA * A);
  hipLaunchKernelGGL(shape_density_kernel, dim3((unsigned)((cells + SHP_THREADS - 1) / SHP_THREADS)), dim3(SHP_THREADS), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}
