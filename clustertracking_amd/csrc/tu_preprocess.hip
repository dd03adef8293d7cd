// tu_preprocess.hip -- bandpass, lowpass and rescaling of whole frames (ctr_preprocess_device;
// preprocess_kernels.h).  Every operation must round where SciPy's rounds: no
// floating-point contraction anywhere in this unit.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <type_traits>

#include "kargs.h"

namespace {

#include "stage_common.h"
#include "preprocess_kernels.h"

constexpr size_t PRE_LDS_MAX = 64 * 1024;

// dynamic LDS of pre_yx_kernel (the layout is the kernel's)
size_t pre_lds_bytes(const PreGeom& g, int ty, size_t pix, size_t gin) {
  const size_t gcols = PRE_TX + 2 * g.l[2], grows = ty + 2 * g.l[1];
  const size_t bcols = PRE_TX + 2 * g.h[2], brows = ty + 2 * g.h[1];
  size_t b = sizeof(double) * ty * gcols + ((gin * grows * gcols + 7) & ~(size_t)7);
  if (g.with_box) b += pix * (ty * bcols + brows * bcols);
  return b;
}

template <typename T, typename GIN>
void launch_yx(const GIN* gin, const T* bin, const PreGeom& g, long long n_slices, const double* wy, const double* wx,
               int out_mode, double* band, unsigned long long* maxkey, const double* scale, void* out, hipStream_t s) {
  const unsigned ntx = (unsigned)((g.nx + PRE_TX - 1) / PRE_TX);
  hipLaunchKernelGGL((pre_yx_kernel<T, GIN>), dim3((unsigned)(ntx * n_slices), (unsigned)((g.ny + g.ty - 1) / g.ty)),
                     dim3(PRE_THREADS), pre_lds_bytes(g, g.ty, sizeof(T), sizeof(GIN)), s, gin, bin, g, wy, wx, out_mode,
                     band, maxkey, scale, (typename PreOut<T>::type*)out);
}

template <typename T>
int run(const ctr_preprocess* p, const PreGeom& g, bool z_gauss, bool z_box, int strategy, hipStream_t s, const char** msg) {
  typedef typename PreOut<T>::type O;
  const long long F = p->n_frames, total = F * g.E, n_slices = F * g.nz;
  const T* raw = (const T*)p->frames;
  const double *wz = p->taps[0], *wy = p->taps[p->ndim - 2], *wx = p->taps[p->ndim - 1];
  const unsigned eblocks = (unsigned)((total + PRE_THREADS - 1) / PRE_THREADS);
  const double gamut = (double)std::numeric_limits<O>::max();
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };

  if (p->mode == CTR_PRE_SCALE) {   // frames as they are into the integer type (float frames)
    unsigned long long* maxkey = nullptr;
    hipError_t e = hipMallocAsync((void**)&maxkey, sizeof(unsigned long long) * F, s);
    if (e != hipSuccess) { *msg = "cannot allocate the workspace"; return CTR_ERR_NOMEM; }
    e = hipMemsetAsync(maxkey, 0, sizeof(unsigned long long) * F, s);
    if (e == hipSuccess) {
      const int bpf = (int)std::min<long long>(256, std::max<long long>(1, g.E / (PRE_THREADS * 8)));
      hipLaunchKernelGGL(pre_plane_max_kernel<T>, dim3((unsigned)(bpf * F)), dim3(PRE_THREADS), 0, s, raw, g.E, bpf, maxkey);
      hipLaunchKernelGGL(pre_scale_factor_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, s,
                         (const unsigned long long*)maxkey, F, gamut, p->scale_factor);
      hipLaunchKernelGGL((pre_scale_kernel<T, O>), dim3(eblocks), dim3(PRE_THREADS), 0, s, raw, g.E, total,
                         (const double*)p->scale_factor, (O*)p->out);
      e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(maxkey, s);
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
    return CTR_OK;
  }

  const bool scaled = p->mode == CTR_PRE_PREPROCESS;
  const bool plane = scaled && strategy == CTR_PRE_BAND_PLANE;
  const size_t o_max = 0;
  const size_t o_gz = o_max + up(sizeof(unsigned long long) * F);
  const size_t o_bz = o_gz + (z_gauss ? up(sizeof(double) * total) : 0);
  const size_t o_band = o_bz + (z_box ? up(sizeof(T) * total) : 0);
  const size_t bytes = o_band + (plane ? up(sizeof(double) * total) : 0);
  unsigned char* ws = nullptr;
  hipError_t e = hipMallocAsync((void**)&ws, bytes, s);
  if (e != hipSuccess) { *msg = "cannot allocate the workspace"; return CTR_ERR_NOMEM; }
  unsigned long long* maxkey = (unsigned long long*)(ws + o_max);
  double* gz = z_gauss ? (double*)(ws + o_gz) : nullptr;
  T* bz = z_box ? (T*)(ws + o_bz) : nullptr;
  double* band = plane ? (double*)(ws + o_band) : nullptr;

  e = hipMemsetAsync(maxkey, 0, sizeof(unsigned long long) * F, s);
  if (e == hipSuccess) {
    if (z_gauss || z_box)
      hipLaunchKernelGGL(pre_z_kernel<T>, dim3(eblocks), dim3(PRE_THREADS), 0, s, raw, g, total, wz, gz, bz);
    const T* bin = z_box ? (const T*)bz : raw;
    // one pass of the fused kernel; the Gaussian reads float64 planes behind a z pass
    auto yx = [&](int out_mode, double* band_out, unsigned long long* mk, const double* sc, void* out) {
      if (z_gauss) launch_yx<T, double>(gz, bin, g, n_slices, wy, wx, out_mode, band_out, mk, sc, out, s);
      else launch_yx<T, T>(raw, bin, g, n_slices, wy, wx, out_mode, band_out, mk, sc, out, s);
    };
    if (!scaled) {
      yx(PRE_OUT_BAND, (double*)p->out, nullptr, nullptr, nullptr);
    } else {
      yx(plane ? PRE_OUT_BAND : PRE_OUT_MAX, band, maxkey, nullptr, nullptr);
      hipLaunchKernelGGL(pre_scale_factor_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, s,
                         (const unsigned long long*)maxkey, F, gamut, p->scale_factor);
      if (plane)
        hipLaunchKernelGGL((pre_scale_kernel<double, O>), dim3(eblocks), dim3(PRE_THREADS), 0, s, (const double*)band, g.E,
                           total, (const double*)p->scale_factor, (O*)p->out);
      else
        yx(PRE_OUT_SCALED, nullptr, nullptr, p->scale_factor, p->out);
    }
    e = hipGetLastError();
  }
  const hipError_t ef = hipFreeAsync(ws, s);
  if (e == hipSuccess) e = ef;
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}

}  // namespace

int ctr_preprocess_launch(const ctr_preprocess* p, StageRun* stage, const char** msg) {
  *msg = "";
  if (!p) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (p->ndim != 2 && p->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (p->frame_dtype < CTR_DTYPE_U8 || p->frame_dtype > CTR_DTYPE_F64) { *msg = "unknown frame dtype"; return CTR_ERR_INVALID; }
  if (p->n_frames < 0) { *msg = "n_frames must be >= 0"; return CTR_ERR_INVALID; }
  if (p->mode < CTR_PRE_LOWPASS || p->mode > CTR_PRE_SCALE) { *msg = "unknown mode"; return CTR_ERR_INVALID; }
  if (p->strategy < CTR_PRE_AUTO || p->strategy > CTR_PRE_TWICE) { *msg = "unknown strategy"; return CTR_ERR_INVALID; }
  const bool is_float = p->frame_dtype >= CTR_DTYPE_F32;
  if (p->mode == CTR_PRE_SCALE && !is_float) { *msg = "only float frames are rescaled as they are"; return CTR_ERR_INVALID; }
  if (!(p->threshold == p->threshold)) { *msg = "threshold must be a number"; return CTR_ERR_INVALID; }
  const bool stencil = p->mode != CTR_PRE_SCALE, with_box = p->mode == CTR_PRE_BANDPASS || p->mode == CTR_PRE_PREPROCESS;
  const bool scaled = p->mode == CTR_PRE_PREPROCESS || p->mode == CTR_PRE_SCALE;
  PreGeom g;
  const int a0 = 3 - p->ndim;   // axis slot of the first frame axis: (z, y, x)
  long long ext[3] = {1, 1, 1};
  long long E = 1;
  for (int a = 0; a < 3; ++a) { g.lw[a] = g.l[a] = g.h[a] = g.hx[a] = 0; g.bs[a] = 1; }
  for (int i = 0; i < p->ndim; ++i) {
    const int a = a0 + i;
    if (p->shape[i] < 1 || p->shape[i] > (1LL << 30)) { *msg = "frame shape must be in [1, 2^30]"; return CTR_ERR_INVALID; }
    ext[a] = p->shape[i];
    E *= p->shape[i];
    if (E > 0x7fffffffLL) { *msg = "more than 2^31 - 1 pixels per frame"; return CTR_ERR_INVALID; }
    if (!stencil) continue;
    if (p->n_taps[i] < 1 || p->n_taps[i] % 2 == 0) { *msg = "n_taps must be odd and >= 1 (2 lw + 1)"; return CTR_ERR_INVALID; }
    if (p->n_taps[i] > (1 << 20)) { *msg = "more than 2^20 taps"; return CTR_ERR_UNSUPPORTED; }
    if (!p->taps[i]) { *msg = "null taps"; return CTR_ERR_INVALID; }
    g.lw[a] = p->n_taps[i] / 2;
    g.l[a] = (int)std::min<long long>(g.lw[a], ext[a] - 1);
    if (!with_box) continue;
    if (p->box[i] < 1 || p->box[i] % 2 == 0) { *msg = "box sizes must be odd and >= 1"; return CTR_ERR_INVALID; }
    if (p->box[i] > (1 << 20)) { *msg = "box above 2^20"; return CTR_ERR_UNSUPPORTED; }
    g.bs[a] = p->box[i];
    g.h[a] = (int)std::min<long long>(p->box[i] / 2, ext[a] - 1);
    g.hx[a] = p->box[i] / 2 - g.h[a];
  }
  if (p->n_frames * E > (1LL << 40)) { *msg = "block too large for one call"; return CTR_ERR_INVALID; }
  if (p->n_frames > 0 && (!p->frames || !p->out)) { *msg = "null frames or out"; return CTR_ERR_INVALID; }
  if (p->n_frames > 0 && scaled && !p->scale_factor) { *msg = "null scale_factor"; return CTR_ERR_INVALID; }
  g.nz = (int)ext[0];
  g.ny = (int)ext[1];
  g.nx = (int)ext[2];
  g.E = E;
  g.with_box = with_box;
  g.strict = p->mode == CTR_PRE_LOWPASS;
  g.threshold = p->threshold;
  // a z pass only where it does something: a single tap is 1, a box of 1 the pixel itself
  const bool z_gauss = stencil && g.lw[0] > 0, z_box = with_box && g.bs[0] > 1;
  static const size_t elem[6] = {1, 2, 2, 4, 4, 8};
  const size_t pix = elem[p->frame_dtype], gin = z_gauss ? sizeof(double) : pix;
  g.ty = 16;
  if (stencil) {
    while (g.ty > 1 && pre_lds_bytes(g, g.ty, pix, gin) > PRE_LDS_MAX) g.ty /= 2;
    if (pre_lds_bytes(g, g.ty, pix, gin) > PRE_LDS_MAX) { *msg = "taps or box too wide for the device path (LDS tile over 64 KiB)"; return CTR_ERR_UNSUPPORTED; }
    if ((g.ny + g.ty - 1) / g.ty > 65535) { *msg = "too many rows per frame for one call"; return CTR_ERR_UNSUPPORTED; }
    if ((long long)((g.nx + PRE_TX - 1) / PRE_TX) * p->n_frames * g.nz > 0x7fffffffLL) { *msg = "too many tiles for one call"; return CTR_ERR_UNSUPPORTED; }
  }
  if (stage->mode != STAGE_LAUNCH || p->n_frames == 0) return CTR_OK;
  const hipStream_t s = stage->stream;
  // by byte count (3 B against 18 B per uint8 pixel through HBM); see the time paragraph of DESIGN.md 7b
  const int strategy = p->strategy == CTR_PRE_AUTO ? CTR_PRE_TWICE : p->strategy;
  switch (p->frame_dtype) {
    case CTR_DTYPE_U8: return run<uint8_t>(p, g, z_gauss, z_box, strategy, s, msg);
    case CTR_DTYPE_U16: return run<uint16_t>(p, g, z_gauss, z_box, strategy, s, msg);
    case CTR_DTYPE_I16: return run<int16_t>(p, g, z_gauss, z_box, strategy, s, msg);
    case CTR_DTYPE_I32: return run<int32_t>(p, g, z_gauss, z_box, strategy, s, msg);
    case CTR_DTYPE_F32: return run<float>(p, g, z_gauss, z_box, strategy, s, msg);
    default: return run<double>(p, g, z_gauss, z_box, strategy, s, msg);
  }
}
