// tu_characterize.hip -- mass, signal and size of located features (ctr_characterize_device;
// characterize_kernels.h).  The mask test must equal NumPy's bit for bit: no
// floating-point contraction anywhere in this unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "characterize_kernels.h"

// window pixels up to which a 2D feature takes a 16-lane row (17 x 17: about 18 pixels a lane);
// larger and 3D windows take the wavefront
constexpr long long CHR_ROW_WINDOW = 17 * 17;

template <int ND, typename T>
void launch(const ChrArgs& a, long long vol, hipStream_t s) {
  if (ND == 2 && vol <= CHR_ROW_WINDOW) {
    const unsigned grid = (unsigned)((a.n_features + CHR_THREADS / 16 - 1) / (CHR_THREADS / 16));
    hipLaunchKernelGGL((characterize_kernel<ND, T, 16>), dim3(grid), dim3(CHR_THREADS), 0, s, a);
  } else {
    const unsigned grid = (unsigned)((a.n_features + CHR_THREADS / 64 - 1) / (CHR_THREADS / 64));
    hipLaunchKernelGGL((characterize_kernel<ND, T, 64>), dim3(grid), dim3(CHR_THREADS), 0, s, a);
  }
}

template <typename T>
void launch_nd(int ndim, const ChrArgs& a, long long vol, hipStream_t s) {
  if (ndim == 2) launch<2, T>(a, vol, s);
  else launch<3, T>(a, vol, s);
}

}  // namespace

int ctr_characterize_launch(const ctr_characterize* c, StageRun* stage, const char** msg) {
  *msg = "";
  if (!c) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (c->ndim != 2 && c->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (c->frame_dtype < CTR_DTYPE_U8 || c->frame_dtype > CTR_DTYPE_F64) { *msg = "unknown frame dtype"; return CTR_ERR_UNSUPPORTED; }
  if (c->n_frames < 0 || c->n_features < 0) { *msg = "negative counts"; return CTR_ERR_INVALID; }
  if (!(c->scale_factor == c->scale_factor) || c->scale_factor == 0.) { *msg = "scale_factor must be a non-zero number"; return CTR_ERR_INVALID; }
  if ((c->pos != nullptr) == (c->pos_i32 != nullptr)) { *msg = "exactly one of pos and pos_i32 must be given"; return CTR_ERR_INVALID; }
  ChrArgs a;
  long long E = 1, vol = 1;
  for (int d = 0; d < 3; ++d) { a.shape[d] = 1; a.radius[d] = 0; }
  for (int d = 0; d < c->ndim; ++d) {
    if (c->shape[d] < 1 || c->shape[d] > (1LL << 30)) { *msg = "frame shape must be in [1, 2^30]"; return CTR_ERR_INVALID; }
    if (c->radius[d] < 0) { *msg = "radius must be >= 0"; return CTR_ERR_INVALID; }
    if (c->radius[d] > 1024) { *msg = "radius above 1024"; return CTR_ERR_UNSUPPORTED; }
    E *= c->shape[d];
    if (E > 0x7fffffffLL) { *msg = "more than 2^31 - 1 pixels per frame"; return CTR_ERR_INVALID; }
    vol *= 2 * c->radius[d] + 1;
    a.shape[d] = (int)c->shape[d];
    a.radius[d] = (int)c->radius[d];
  }
  if (vol > (1LL << 24)) { *msg = "window above 2^24 pixels"; return CTR_ERR_UNSUPPORTED; }
  if (c->n_frames > 0x7fffffffLL || c->n_features > (1LL << 31) * (CHR_THREADS / 64) - 1) { *msg = "too many frames or features for one call"; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && (c->n_frames < 1 || !c->frames || !c->frame_offset)) { *msg = "features without frames or frame_offset"; return CTR_ERR_INVALID; }
  if (c->n_features > 0 && (!c->mass || !c->signal || !c->size)) { *msg = "null output"; return CTR_ERR_INVALID; }
  if (stage->mode != STAGE_LAUNCH || c->n_features == 0) return CTR_OK;
  const hipStream_t s = stage->stream;
  a.frames = c->frames;
  a.frame_elems = E;
  a.n_frames = (int)c->n_frames;
  a.isotropic = c->isotropic != 0;
  a.scale_factor = c->scale_factor;
  a.n_features = c->n_features;
  a.frame_offset = (const long long*)c->frame_offset;
  a.pos = c->pos;
  a.pos_i32 = c->pos_i32;
  a.mass = c->mass;
  a.signal = c->signal;
  a.size = c->size;
  switch (c->frame_dtype) {
    case CTR_DTYPE_U8: launch_nd<uint8_t>(c->ndim, a, vol, s); break;
    case CTR_DTYPE_U16: launch_nd<uint16_t>(c->ndim, a, vol, s); break;
    case CTR_DTYPE_I16: launch_nd<int16_t>(c->ndim, a, vol, s); break;
    case CTR_DTYPE_I32: launch_nd<int32_t>(c->ndim, a, vol, s); break;
    case CTR_DTYPE_F32: launch_nd<float>(c->ndim, a, vol, s); break;
    default: launch_nd<double>(c->ndim, a, vol, s); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}
