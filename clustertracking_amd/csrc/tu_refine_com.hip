// tu_refine_com.hip -- centre-of-mass refinement of features (ctr_refine_com_device and the
// per-level step of ctr_find_link_refine_device; refine_com_kernels.h).  The mask
// test and the position must equal NumPy's bit for bit: no floating-point contraction anywhere in
// this unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "characterize_kernels.h"
#include "refine_com_kernels.h"

// the decision of tu_characterize.hip: a 2D window of up to 17 x 17 pixels takes a 16-lane row,
// larger and 3D windows take the wavefront
constexpr long long RFC_ROW_WINDOW = 17 * 17;
// workgroups of a level of ctr_find_link_refine_device: its rows are counted on the device, so a
// fixed grid strides over them (fewer where the handle's cap is lower: StageRun::max_grid)
constexpr unsigned RFC_LEVEL_GRID = 32;

template <int ND, typename T, int G>
void launch_g(const RfcArgs& a, long long rows, const StageRun* stage) {
  const long long per = RFC_THREADS / G;
  unsigned grid = (unsigned)((rows + per - 1) / per);
  if (a.level_cnt) {
    const unsigned cap = RFC_LEVEL_GRID < stage->max_grid ? RFC_LEVEL_GRID : stage->max_grid;
    grid = grid < cap ? grid : cap;
  }
  hipLaunchKernelGGL((refine_com_kernel<ND, T, G>), dim3(grid), dim3(RFC_THREADS), 0, stage->stream, a);
}

// rows: the features, or a bound on the rows of a level
template <typename T>
void launch(int ndim, const RfcArgs& a, long long vol, long long rows, const StageRun* stage) {
  if (ndim == 3) launch_g<3, T, 64>(a, rows, stage);
  else if (vol <= RFC_ROW_WINDOW) launch_g<2, T, 16>(a, rows, stage);
  else launch_g<2, T, 64>(a, rows, stage);
}

}  // namespace

int ctr_refine_com_launch(const ctr_refine_com* c, StageRun* stage, const char** msg, const RefineComLevel* level) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (c->ndim != 2 && c->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (c->frame_dtype < CTR_DTYPE_U8 || c->frame_dtype > CTR_DTYPE_F64) { *msg = "unknown frame dtype"; return CTR_ERR_UNSUPPORTED; }
  if (c->n_frames < 0 || (!level && c->n_features < 0)) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (c->max_iterations < 1 || c->max_iterations > 100) { *msg = "max_iterations must be in [1, 100]"; return CTR_ERR_INVALID; }
  if (!(c->shift_thresh > 0.)) { *msg = "shift_thresh must be greater than 0"; return CTR_ERR_INVALID; }
  RfcArgs a = {};
  long long E = 1, vol = 1;
  for (int d = 0; d < 3; ++d) { a.shape[d] = 1; a.radius[d] = 0; a.sr[d] = 1.; }
  for (int d = 0; d < c->ndim; ++d) {
    if (c->shape[d] < 1 || c->shape[d] > (1LL << 30)) { *msg = "frame shape must be in [1, 2^30]"; return CTR_ERR_INVALID; }
    if (c->radius[d] < 1) { *msg = "radius must be >= 1"; return CTR_ERR_INVALID; }
    if (c->radius[d] > 1024) { *msg = "radius above 1024"; return CTR_ERR_UNSUPPORTED; }
    if (2 * c->radius[d] + 1 > c->shape[d]) { *msg = "radius: the window 2 radius + 1 is wider than the frame"; return CTR_ERR_INVALID; }
    E *= c->shape[d];
    if (E > 0x7fffffffLL) { *msg = "more than 2^31 - 1 pixels per frame"; return CTR_ERR_INVALID; }
    vol *= 2 * c->radius[d] + 1;
    a.shape[d] = (int)c->shape[d];
    a.radius[d] = (int)c->radius[d];
  }
  if (vol > (1LL << 24)) { *msg = "window above 2^24 pixels"; return CTR_ERR_UNSUPPORTED; }
  if (c->n_frames > 0x7fffffffLL) { *msg = "too many frames for one call"; return CTR_ERR_INVALID; }
  if (stage->mode == STAGE_CHECK_SCALARS) return CTR_OK;
  long long rows;
  if (level) {
    if (!c->frames) { *msg = "null frames"; return CTR_ERR_INVALID; }
    if (level->frame < 0 || level->frame >= c->n_frames) { *msg = "level beyond the frames"; return CTR_ERR_INVALID; }
    rows = level->max_rows;
    a.level_start = level->start;
    a.level_cnt = level->cnt;
    a.frame = level->frame;
    a.pos = a.pos_out = level->pos;
    a.mass = level->mass;
    a.spos = level->spos;
    for (int d = 0; d < c->ndim; ++d) a.sr[d] = level->sr[d];
  } else {
    if (c->n_features > (1LL << 31) * (RFC_THREADS / 64) - 1) { *msg = "too many features for one call"; return CTR_ERR_INVALID; }
    if (c->n_features > 0 && (c->n_frames < 1 || !c->frames || !c->frame_offset || !c->pos)) { *msg = "features without frames, frame_offset or pos"; return CTR_ERR_INVALID; }
    if (c->n_features > 0 && (!c->pos_out || !c->mass || !c->n_iter)) { *msg = "null output"; return CTR_ERR_INVALID; }
    rows = c->n_features;
    a.n_features = c->n_features;
    a.frame_offset = (const long long*)c->frame_offset;
    a.pos = c->pos;
    a.pos_out = c->pos_out;
    a.mass = c->mass;
    a.n_iter = c->n_iter;
  }
  if (stage->mode != STAGE_LAUNCH || rows <= 0) return CTR_OK;
  a.frames = c->frames;
  a.frame_elems = E;
  a.n_frames = (int)c->n_frames;
  a.max_iterations = c->max_iterations;
  a.shift_thresh = c->shift_thresh;
  switch (c->frame_dtype) {
    case CTR_DTYPE_U8: launch<uint8_t>(c->ndim, a, vol, rows, stage); break;
    case CTR_DTYPE_U16: launch<uint16_t>(c->ndim, a, vol, rows, stage); break;
    case CTR_DTYPE_I16: launch<int16_t>(c->ndim, a, vol, rows, stage); break;
    case CTR_DTYPE_I32: launch<int32_t>(c->ndim, a, vol, rows, stage); break;
    case CTR_DTYPE_F32: launch<float>(c->ndim, a, vol, rows, stage); break;
    default: launch<double>(c->ndim, a, vol, rows, stage); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}
