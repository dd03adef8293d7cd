// tu_locate.hip -- feature location (ctr_locate_maxima_device; locate_kernels.h).
// The threshold must equal NumPy's and the pair distances cKDTree's bit for bit: no
// floating-point contraction anywhere in this unit.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "kargs.h"

namespace {

#include "stage_common.h"
#include "locate_kernels.h"

constexpr size_t LOC_LDS_MAX = 64 * 1024;

template <typename T>
int run(const ctr_locate* l, const LocGeom& g, hipStream_t s, const char** msg) {
  const long long F = l->n_frames;
  const int bpf = (int)std::min<long long>(64, std::max<long long>(1, (g.E + LOC_THREADS * 16 - 1) / (LOC_THREADS * 16)));
  const int cpf = (int)((g.W + LOC_CHUNK_WORDS - 1) / LOC_CHUNK_WORDS);
  const bool suppress = l->precise && g.sep[0] > 0 && g.sep[1] > 0 && g.sep[2] > 0;
  // workspace, 256-byte aligned parts
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_sel = 0;
  const size_t o_hist = o_sel + up(sizeof(LocSel) * F);
  const size_t o_nan = o_hist + up(sizeof(unsigned) * 512 * F);
  const size_t o_thr = o_nan + up(sizeof(unsigned) * F);
  const size_t o_mask = o_thr + up(sizeof(double) * F);
  const size_t o_keep = o_mask + up(sizeof(unsigned long long) * g.W * F);
  const size_t o_count = o_keep + (suppress ? up(sizeof(unsigned long long) * g.W * F) : 0);
  const size_t o_base = o_count + up(sizeof(long long) * cpf * F);
  const size_t bytes = o_base + up(sizeof(long long) * cpf * F);
  unsigned char* ws = nullptr;
  hipError_t e = hipMallocAsync((void**)&ws, bytes, s);
  if (e != hipSuccess) { *msg = "cannot allocate the workspace"; return CTR_ERR_NOMEM; }
  LocSel* sel = (LocSel*)(ws + o_sel);
  unsigned* hist = (unsigned*)(ws + o_hist);
  unsigned* nan_count = (unsigned*)(ws + o_nan);
  double* thr = (double*)(ws + o_thr);
  unsigned long long* mask = (unsigned long long*)(ws + o_mask);
  unsigned long long* keep = suppress ? (unsigned long long*)(ws + o_keep) : mask;
  long long* count = (long long*)(ws + o_count);
  long long* base = (long long*)(ws + o_base);
  const T* frames = (const T*)l->frames;

  e = hipMemsetAsync(ws, 0, o_thr, s);   // selection state, histograms, NaN counts
  if (e == hipSuccess) {
    const unsigned fgrid = (unsigned)((F + 63) / 64);
    for (int shift = LocKey<T>::bits - 8; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(loc_hist_kernel<T>, dim3((unsigned)(bpf * F)), dim3(LOC_THREADS), 0, s,
                         frames, g.E, bpf, shift, sel, hist, nan_count);
      hipLaunchKernelGGL(loc_pick_kernel<T>, dim3(fgrid), dim3(64), 0, s, F, shift, l->percentile, sel, hist,
                         nan_count, thr);
    }
    const int rows = g.ty + g.b[1] - 1, cols = LOC_TX + g.b[2] - 1;
    const size_t smem = sizeof(T) * ((size_t)rows * cols + (size_t)rows * LOC_TX + (size_t)g.ring * g.ty * LOC_TX);
    hipLaunchKernelGGL(loc_maxima_kernel<T>, dim3((unsigned)(g.nwx * F), (unsigned)((g.ny + g.ty - 1) / g.ty)),
                       dim3(LOC_THREADS), smem, s, frames, g, (const double*)thr, mask);
    if (suppress) {
      const long long n_words = g.W * F;
      hipLaunchKernelGGL(loc_suppress_kernel<T>, dim3((unsigned)((n_words + LOC_THREADS - 1) / LOC_THREADS)),
                         dim3(LOC_THREADS), 0, s, frames, g, n_words, (const unsigned long long*)mask, keep);
    }
    hipLaunchKernelGGL(loc_count_kernel, dim3((unsigned)(cpf * F)), dim3(LOC_THREADS), 0, s,
                       (const unsigned long long*)keep, g.W, cpf, count);
    hipLaunchKernelGGL(loc_scan_kernel, dim3(1), dim3(LOC_SCAN_THREADS), 0, s, (const long long*)count, (long long)cpf * F, cpf,
                       F, base, l->frame_offset, l->total);
    hipLaunchKernelGGL(loc_write_kernel, dim3((unsigned)(cpf * F)), dim3(LOC_THREADS), 0, s,
                       (const unsigned long long*)keep, g, cpf, (const long long*)base, (long long)l->capacity,
                       l->pos_out);
    e = hipGetLastError();
    if (e == hipSuccess && l->threshold)
      e = hipMemcpyAsync(l->threshold, thr, sizeof(double) * F, hipMemcpyDeviceToDevice, s);
  }
  const hipError_t ef = hipFreeAsync(ws, s);
  if (e == hipSuccess) e = ef;
  if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
  return CTR_OK;
}

}  // namespace

int ctr_locate_launch(const ctr_locate* l, hipStream_t s, const char** msg) {
  *msg = "";
  if (!l) { *msg = "null descriptor"; return CTR_ERR_INVALID; }
  if (l->ndim != 2 && l->ndim != 3) { *msg = "ndim must be 2 or 3"; return CTR_ERR_INVALID; }
  if (l->frame_dtype < CTR_DTYPE_U8 || l->frame_dtype > CTR_DTYPE_F64) { *msg = "unknown frame dtype"; return CTR_ERR_INVALID; }
  if (l->n_frames < 0) { *msg = "n_frames must be >= 0"; return CTR_ERR_INVALID; }
  if (!(l->percentile >= 0. && l->percentile <= 100.)) { *msg = "percentile must be in [0, 100]"; return CTR_ERR_INVALID; }
  if (l->capacity < 0) { *msg = "capacity must be >= 0"; return CTR_ERR_INVALID; }
  if (!l->frame_offset || !l->total) { *msg = "null frame_offset or total"; return CTR_ERR_INVALID; }
  if (l->capacity > 0 && !l->pos_out) { *msg = "null pos_out"; return CTR_ERR_INVALID; }
  if (l->n_frames > 0 && !l->frames) { *msg = "null frames"; return CTR_ERR_INVALID; }
  LocGeom g;
  g.ndim = l->ndim;
  const int a0 = 3 - l->ndim;   // axis slot of the first frame axis: (z, y, x)
  long long ext[3] = {1, 1, 1};
  long long E = 1;
  for (int a = 0; a < 3; ++a) {
    g.sep[a] = 1.;
    g.margin[a] = 0;
    g.b[a] = 1;
    g.lo[a] = 0;
    g.reach[a] = 0;
  }
  for (int i = 0; i < l->ndim; ++i) {
    const int a = a0 + i;
    if (l->shape[i] < 1 || l->shape[i] > (1LL << 30)) { *msg = "frame shape must be in [1, 2^30]"; return CTR_ERR_INVALID; }
    const double sp = l->separation[i];
    if (!(sp >= 0.) || !(sp <= 1e9)) { *msg = "separation must be finite and >= 0"; return CTR_ERR_INVALID; }
    if (l->margin[i] < 0) { *msg = "margin must be >= 0"; return CTR_ERR_INVALID; }
    ext[a] = l->shape[i];
    E *= l->shape[i];
    if (E > 0x7fffffffLL) { *msg = "more than 2^31 - 1 pixels per frame"; return CTR_ERR_INVALID; }
    g.sep[a] = sp;
    g.margin[a] = l->margin[i];
    // box int(2 s / sqrt(ndim)); size 0 filters like size 1.  A reach past the frame's extent
    // adds only the zero border, which a reach of the extent adds too.
    long long b = (long long)(2. * sp / std::sqrt((double)l->ndim));
    if (b < 1) b = 1;
    long long lo = (b - 1) / 2, hi = b / 2;
    lo = std::min(lo, ext[a]);
    hi = std::min(hi, ext[a]);
    g.b[a] = (int)(lo + hi + 1);
    g.lo[a] = (int)lo;
    g.reach[a] = (int)std::min<double>(std::floor(sp), (double)ext[a]);
  }
  if (l->n_frames * E > (1LL << 40)) { *msg = "block too large for one call"; return CTR_ERR_INVALID; }
  g.E = E;
  g.nz = (int)ext[0];
  g.ny = (int)ext[1];
  g.nx = (int)ext[2];
  g.nwx = (g.nx + LOC_TX - 1) / LOC_TX;
  g.W = (long long)g.nz * g.ny * g.nwx;
  g.ring = std::min(g.b[0], g.nz);
  static const size_t elem[6] = {1, 2, 2, 4, 4, 8};
  const size_t es = elem[l->frame_dtype];
  g.ty = l->ndim == 2 ? 16 : 8;
  auto lds = [&](int ty) {
    return es * ((size_t)(ty + g.b[1] - 1) * (LOC_TX + g.b[2] - 1) + (size_t)(ty + g.b[1] - 1) * LOC_TX +
                 (size_t)g.ring * ty * LOC_TX);
  };
  while (g.ty > 1 && lds(g.ty) > LOC_LDS_MAX) g.ty /= 2;
  if (lds(g.ty) > LOC_LDS_MAX) { *msg = "box too large for the device path (LDS tile over 64 KiB)"; return CTR_ERR_UNSUPPORTED; }
  if ((g.ny + g.ty - 1) / g.ty > 65535) { *msg = "too many rows per frame for one call"; return CTR_ERR_UNSUPPORTED; }
  if (l->n_frames == 0) {
    hipError_t e = hipMemsetAsync(l->frame_offset, 0, sizeof(int64_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(l->total, 0, sizeof(int64_t), s);
    if (e != hipSuccess) { *msg = hipGetErrorString(e); return CTR_ERR_DEVICE; }
    return CTR_OK;
  }
  switch (l->frame_dtype) {
    case CTR_DTYPE_U8: return run<uint8_t>(l, g, s, msg);
    case CTR_DTYPE_U16: return run<uint16_t>(l, g, s, msg);
    case CTR_DTYPE_I16: return run<int16_t>(l, g, s, msg);
    case CTR_DTYPE_I32: return run<int32_t>(l, g, s, msg);
    case CTR_DTYPE_F32: return run<float>(l, g, s, msg);
    default: return run<double>(l, g, s, msg);
  }
}
