// preprocess_kernels.h -- bandpass, lowpass and rescaling of whole frames on the device
// (include/ctrefine.h: ctr_preprocess_device).  Included by tu_preprocess.hip inside
// its anonymous namespace, after stage_common.h (ordered_key).
//
// Two separable stencils over the same pixels: a Gaussian (SciPy's correlate1d, symmetric order,
// zero beyond the frame, float64) and a box (SciPy's uniform_filter1d in the pixel type, edge
// clamped, exact window sum then one float64 division and a truncating cast).  The last two axes
// are fused in pre_yx_kernel: a block loads the two input tiles with their halos into LDS, runs
// the y passes from LDS into LDS and the x passes from LDS into registers.  A stack's first axis
// is a pass of its own through HBM (pre_z_kernel): its neighbours are a plane apart, so the lanes
// of a wavefront read neighbouring pixels whatever the tap.  Every intermediate is rounded where
// SciPy rounds it (once per operation, no contraction), so integer frames come out bit for bit.
#ifndef CTREFINE_PREPROCESS_KERNELS_H
#define CTREFINE_PREPROCESS_KERNELS_H

constexpr int PRE_THREADS = 256;
constexpr int PRE_TX = 64;       // tile width: one wavefront per tile row

// what pre_yx_kernel does with the band value of a pixel
enum { PRE_OUT_BAND = 0,     // write it (float64)
       PRE_OUT_MAX = 1,      // only its per-frame maximum
       PRE_OUT_SCALED = 2 }; // write it scaled into the integer type

struct PreGeom {
  int nz, ny, nx;        // 2D: nz = 1
  long long E;           // pixels per frame
  // per axis slot (z, y, x):
  int lw[3];             // half-width of the Gaussian taps = index of the centre tap
  int l[3];              // taps that can reach the frame: min(lw, n - 1)
  int bs[3];             // box size (odd, >= 1)
  int h[3];              // box half-width that can reach past the edge pixel: min(bs / 2, n - 1)
  int hx[3];             // bs / 2 - h: copies of each edge pixel the window holds beyond those
  int ty;                // tile rows
  int with_box;          // 0: lowpass (no background)
  int strict;            // threshold test: 1 `>` (lowpass), 0 `>=` (bandpass)
  double threshold;
};

// window sums: exact in 64 bits for integer pixels, float64 for float pixels
template <typename T> struct PreAcc { typedef long long type; };
template <> struct PreAcc<float> { typedef double type; };
template <> struct PreAcc<double> { typedef double type; };

// the integer type preprocess writes: the pixel type, uint8 for float frames
template <typename T> struct PreOut { typedef T type; };
template <> struct PreOut<float> { typedef uint8_t type; };
template <> struct PreOut<double> { typedef uint8_t type; };

// per-frame maximum: wavefront reduction, then one vector atomic per wavefront
__device__ __forceinline__ void pre_max_commit(unsigned long long key, unsigned long long* slot) {
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned lo = __shfl_down((unsigned)key, d), hi = __shfl_down((unsigned)(key >> 32), d);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(slot, key);
}

// scale * clip(v, 0) cast to the integer type (a C cast: truncation); a frame without a pixel
// above zero (scale not a positive finite number) is written as zeros.  The product stays inside
// the type: v <= the frame's maximum m, and fl(fl(gamut / m) * m) <= gamut (1 + 2^-52), which for
// the widest type (int32) is below gamut + 1e-6 and truncates to gamut.
template <typename O>
__device__ __forceinline__ O pre_to_gamut(double v, double scale) {
  if (!(scale > 0.) || scale > 1.7e308) return (O)0;
  return (O)(scale * (v < 0. ? 0. : v));
}

// The first axis of a stack.  One thread per voxel: gz = Gaussian along z of the raw stack
// (float64), bz = box along z (pixel type); either may be null.
template <typename T>
__global__ __launch_bounds__(PRE_THREADS) void pre_z_kernel(const T* __restrict__ frames, PreGeom g, long long total,
                                                            const double* __restrict__ wz, double* __restrict__ gz,
                                                            T* __restrict__ bz) {
  const long long i = (long long)blockIdx.x * PRE_THREADS + threadIdx.x;
  if (i >= total) return;
  const long long plane = (long long)g.ny * g.nx;
  const long long f = i / g.E, rem = i - f * g.E;
  const int z = (int)(rem / plane);
  const T* col = frames + f * g.E + (rem - (long long)z * plane);
  if (gz) {
    const int c = g.lw[0];
    double t = (double)col[(long long)z * plane] * wz[c];
    for (int j = -g.l[0]; j < 0; ++j) {
      const double a = z + j >= 0 ? (double)col[(long long)(z + j) * plane] : 0.;
      const double b = z - j < g.nz ? (double)col[(long long)(z - j) * plane] : 0.;
      t += (a + b) * wz[c + j];
    }
    gz[i] = t;
  }
  if (bz) {
    typedef typename PreAcc<T>::type A;
    const int h = g.h[0];
    A sum = 0;
    for (int j = -h; j <= h; ++j) {
      int zz = z + j;
      zz = zz < 0 ? 0 : (zz >= g.nz ? g.nz - 1 : zz);
      sum += (A)col[(long long)zz * plane];
    }
    if (g.hx[0]) sum += (A)g.hx[0] * ((A)col[0] + (A)col[(long long)(g.nz - 1) * plane]);
    bz[i] = (T)((double)sum / (double)g.bs[0]);
  }
}

// The last two axes of every slice (a 2D frame, or one plane of a stack; slice s belongs to frame
// s / nz).  gin: what the Gaussian reads (the raw pixels, or pre_z_kernel's gz); bin: what the box
// reads (the raw pixels, or bz).  Grid: x = tiles along x * slices, y = tiles along y.
// Dynamic LDS (pre_lds_bytes): G1 [ty][TX + 2 lx] float64, RG [ty + 2 ly][TX + 2 lx] GIN,
// B1 [ty][TX + 2 hx] T, RB [ty + 2 hy][TX + 2 hx] T.
template <typename T, typename GIN>
__global__ __launch_bounds__(PRE_THREADS) void pre_yx_kernel(const GIN* __restrict__ gin, const T* __restrict__ bin, PreGeom g,
                                                             const double* __restrict__ wy, const double* __restrict__ wx,
                                                             int out_mode, double* __restrict__ band,
                                                             unsigned long long* __restrict__ maxkey,
                                                             const double* __restrict__ scale,
                                                             typename PreOut<T>::type* __restrict__ out) {
  typedef typename PreAcc<T>::type A;
  extern __shared__ double pre_smem[];
  const int ntx = (g.nx + PRE_TX - 1) / PRE_TX;
  const long long slice = blockIdx.x / ntx;
  const int x0 = (int)(blockIdx.x % ntx) * PRE_TX, y0 = (int)blockIdx.y * g.ty;
  const int ty = g.ty, ly = g.l[1], lx = g.l[2], hy = g.h[1], hx = g.h[2];
  const int gcols = PRE_TX + 2 * lx, grows = ty + 2 * ly;
  const int bcols = PRE_TX + 2 * hx, brows = ty + 2 * hy;
  const long long plane = (long long)g.ny * g.nx;
  const int tid = threadIdx.x;

  double* G1 = pre_smem;
  GIN* RG = (GIN*)(G1 + (size_t)ty * gcols);
  const size_t rg_bytes = (sizeof(GIN) * (size_t)grows * gcols + 7) & ~(size_t)7;
  T* B1 = (T*)((unsigned char*)RG + rg_bytes);
  T* RB = B1 + (size_t)ty * bcols;

  // the tiles: zero beyond the frame for the Gaussian, the edge pixel for the box
  const GIN* gsrc = gin + slice * plane;
  for (int i = tid; i < grows * gcols; i += PRE_THREADS) {
    const int r = i / gcols, c = i - r * gcols;
    const int fy = y0 - ly + r, fx = x0 - lx + c;
    GIN v = (GIN)0;
    if (fy >= 0 && fy < g.ny && fx >= 0 && fx < g.nx) v = gsrc[(long long)fy * g.nx + fx];
    RG[i] = v;
  }
  if (g.with_box) {
    const T* bsrc = bin + slice * plane;
    for (int i = tid; i < brows * bcols; i += PRE_THREADS) {
      const int r = i / bcols, c = i - r * bcols;
      int fy = y0 - hy + r, fx = x0 - hx + c;
      fy = fy < 0 ? 0 : (fy >= g.ny ? g.ny - 1 : fy);
      fx = fx < 0 ? 0 : (fx >= g.nx ? g.nx - 1 : fx);
      RB[i] = bsrc[(long long)fy * g.nx + fx];
    }
  }
  __syncthreads();

  // y passes, LDS to LDS
  {
    const int c0 = g.lw[1];
    for (int i = tid; i < ty * gcols; i += PRE_THREADS) {
      const int r = i / gcols, c = i - r * gcols;
      const GIN* p = RG + (size_t)(r + ly) * gcols + c;
      double t = (double)p[0] * wy[c0];
      for (int j = -ly; j < 0; ++j) t += ((double)p[j * gcols] + (double)p[-j * gcols]) * wy[c0 + j];
      G1[i] = t;
    }
  }
  if (g.with_box) {
    for (int i = tid; i < ty * bcols; i += PRE_THREADS) {
      const int r = i / bcols, c = i - r * bcols;
      const T* p = RB + (size_t)r * bcols + c;
      A sum = 0;
      for (int j = 0; j <= 2 * hy; ++j) sum += (A)p[j * bcols];
      if (g.hx[1]) sum += (A)g.hx[1] * ((A)p[0] + (A)p[2 * hy * bcols]);
      B1[i] = (T)((double)sum / (double)g.bs[1]);
    }
  }
  __syncthreads();

  // x passes and the output: a wavefront per tile row
  const long long frame = slice / g.nz;
  const int c = tid & (PRE_TX - 1), x = x0 + c;
  const int cx = g.lw[2];
  const double sc = out_mode == PRE_OUT_SCALED ? scale[frame] : 0.;
  unsigned long long key = 0;
  for (int r = tid / PRE_TX; r < ty; r += PRE_THREADS / PRE_TX) {
    const int y = y0 + r;
    if (y >= g.ny || x >= g.nx) continue;
    const double* p = G1 + (size_t)r * gcols + c + lx;
    double v = p[0] * wx[cx];
    for (int j = -lx; j < 0; ++j) v += (p[j] + p[-j]) * wx[cx + j];
    if (g.with_box) {
      const T* q = B1 + (size_t)r * bcols + c;
      A sum = 0;
      for (int j = 0; j <= 2 * hx; ++j) sum += (A)q[j];
      if (g.hx[2]) sum += (A)g.hx[2] * ((A)q[0] + (A)q[2 * hx]);
      const T bg = (T)((double)sum / (double)g.bs[2]);
      v -= (double)bg;
    }
    v = (g.strict ? v > g.threshold : v >= g.threshold) ? v : 0.;
    const long long o = slice * plane + (long long)y * g.nx + x;
    if (out_mode == PRE_OUT_BAND) band[o] = v;
    else if (out_mode == PRE_OUT_SCALED) out[o] = pre_to_gamut<typename PreOut<T>::type>(v, sc);
    const unsigned long long k = ordered_key(v);   // never NaN: the threshold test made one 0
    key = k > key ? k : key;
  }
  if (maxkey) pre_max_commit(key, maxkey + frame);
}

// per-frame maximum of a plane as it is (float frames that are only rescaled)
template <typename S>
__global__ __launch_bounds__(PRE_THREADS) void pre_plane_max_kernel(const S* __restrict__ src, long long E, int bpf,
                                                                    unsigned long long* __restrict__ maxkey) {
  const long long frame = blockIdx.x / bpf;
  const S* p = src + frame * E;
  unsigned long long key = 0;
  for (long long i = (long long)(blockIdx.x % bpf) * PRE_THREADS + threadIdx.x; i < E; i += (long long)bpf * PRE_THREADS) {
    // the plain key: a NaN pixel has no defined result (include/ctrefine.h), so no rule for it
    const unsigned long long k = ordered_key((double)p[i]);
    key = k > key ? k : key;
  }
  pre_max_commit(key, maxkey + frame);
}

// scale_factor[f] = max of the integer type / max of the frame (one float64 division); a frame
// whose maximum is zero gets +inf
__global__ void pre_scale_factor_kernel(const unsigned long long* __restrict__ maxkey, long long n_frames, double gamut,
                                        double* __restrict__ scale) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  const double m = ordered_unkey(maxkey[f]);
  scale[f] = m == 0. ? __longlong_as_double(0x7ff0000000000000LL) : gamut / m;
}

// a plane (the band plane, or float pixels as they are) scaled into the integer type
template <typename S, typename O>
__global__ __launch_bounds__(PRE_THREADS) void pre_scale_kernel(const S* __restrict__ src, long long E, long long total,
                                                                const double* __restrict__ scale, O* __restrict__ out) {
  const long long i = (long long)blockIdx.x * PRE_THREADS + threadIdx.x;
  if (i >= total) return;
  out[i] = pre_to_gamut<O>((double)src[i], scale[i / E]);
}

#endif  // CTREFINE_PREPROCESS_KERNELS_H
