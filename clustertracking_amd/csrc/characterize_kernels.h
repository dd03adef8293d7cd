// characterize_kernels.h -- mass, signal and radius of gyration of located features
// (ctr_characterize_device).  Included by tu_characterize.hip inside its anonymous
// namespace, after device_common.h (the mask rule and the DPP moves are the refine kernels').
//
// A group of G lanes (a 16-lane DPP row, or the wavefront) takes one feature: its lanes stride the
// window in C order (x fastest: neighbouring lanes read neighbouring pixels of a row), keep partial
// sums in int64 (integer frames: exact, so the result does not depend on G or the launch) or in
// float64 (float frames) and a running maximum, all-reduce them inside the group, and lane 0
// divides, takes the square root and writes.
#ifndef CTREFINE_CHARACTERIZE_KERNELS_H
#define CTREFINE_CHARACTERIZE_KERNELS_H

constexpr int CHR_THREADS = 256;

struct ChrArgs {
  const void* frames;
  long long frame_elems;
  int n_frames;
  int shape[3];          // frame extent per axis, (z,) y, x in slots 0 .. ND-1
  int radius[3];
  int isotropic;
  double scale_factor;
  long long n_features;
  const long long* frame_offset;
  const double* pos;     // one of the two
  const int* pos_i32;
  double* mass;
  double* signal;
  double* size;
};

// what the sums of a pixel type are kept in (NumPy: integer windows sum exactly in 64 bits)
template <typename T> struct ChrAcc { typedef long long type; };
template <> struct ChrAcc<float> { typedef double type; };
template <> struct ChrAcc<double> { typedef double type; };

__device__ __forceinline__ long long chr_add(long long a, long long b) { return a + b; }
__device__ __forceinline__ double chr_add(double a, double b) { return a + b; }
__device__ __forceinline__ long long chr_max(long long a, long long b) { return b > a ? b : a; }
// np.max: a NaN stays
__device__ __forceinline__ double chr_max(double a, double b) { return (b > a || b != b) ? b : a; }

template <int CTRL> __device__ __forceinline__ double chr_dpp(double x) { return dpp_f64<CTRL>(x); }
template <int CTRL> __device__ __forceinline__ long long chr_dpp(long long x) {
  return __double_as_longlong(dpp_f64<CTRL>(__longlong_as_double(x)));   // the bits travel as they are
}

// all-reduce over the G lanes of a group: the DPP row steps of row_sum, then (G = 64) the two
// cross-row exchanges
template <int G, bool MAX, typename A>
__device__ __forceinline__ A chr_reduce(A x) {
  auto op = [](A a, A b) -> A { return MAX ? chr_max(a, b) : chr_add(a, b); };
  x = op(x, chr_dpp<0xB1>(x));    // quad_perm [1,0,3,2]
  x = op(x, chr_dpp<0x4E>(x));    // quad_perm [2,3,0,1]
  x = op(x, chr_dpp<0x141>(x));   // row_half_mirror
  x = op(x, chr_dpp<0x140>(x));   // row_mirror
  if (G == 64) {
    x = op(x, __shfl_xor(x, 16));
    x = op(x, __shfl_xor(x, 32));
  }
  return x;
}

template <int ND, typename T, int G>
__global__ __launch_bounds__(CHR_THREADS) void characterize_kernel(ChrArgs a) {
  typedef typename ChrAcc<T>::type A;
  constexpr bool INTEGER = std::is_integral<T>::value;
  const int lane = threadIdx.x % G;
  const long long feat = (long long)blockIdx.x * (CHR_THREADS / G) + threadIdx.x / G;
  // groups past the end leave as whole DPP rows / wavefronts (G is 16 or 64): the reductions of
  // the others never read them
  if (feat >= a.n_features) return;

  // frame of the feature: the last t with frame_offset[t] <= feat
  int lo = 0, hi = a.n_frames - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.frame_offset[mid] <= feat) lo = mid; else hi = mid - 1;
  }
  const T* frame = (const T*)a.frames + (size_t)lo * a.frame_elems;

  int radius[ND], corner[ND], wshape[ND];
  double rel[ND], rel_w[ND], inv_r2[ND];
  int vol = 1;
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    const double c = a.pos ? a.pos[feat * ND + d] : (double)a.pos_i32[feat * ND + d];
    radius[d] = a.radius[d];
    // int(round(c - radius)), half to even; a centre far outside any frame keeps an empty window
    const double cr = fmin(fmax(rint(c - (double)radius[d]), -1e9), 1e9);
    corner[d] = (int)cr;
    rel[d] = c - cr;
    rel_w[d] = (double)radius[d];
    inv_r2[d] = 1. / ((double)radius[d] * (double)radius[d]);
    wshape[d] = 2 * radius[d] + 1;
    vol *= wshape[d];
  }

  A mass = 0, mx = 0, w[ND];
  bool any = false;
#pragma unroll
  for (int d = 0; d < ND; ++d) w[d] = 0;
  for (int p = lane; p < vol; p += G) {
    int idx[ND];
    int q = p;
#pragma unroll
    for (int d = ND - 1; d > 0; --d) { idx[d] = q % wshape[d]; q /= wshape[d]; }
    idx[0] = q;
    bool inside = true;
    size_t off = 0;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const int g = corner[d] + idx[d];
      inside = inside && g >= 0 && g < a.shape[d];
      off = off * (size_t)a.shape[d] + (size_t)g;
    }
    A v = 0;   // beyond the frame: the padding
    if (inside) {
      const T px = frame[off];
      if (INTEGER) {
        v = in_mask<ND>(idx, rel, inv_r2, radius) ? (A)px : (A)0;
      } else {
        // image * mask as NumPy multiplies it: a NaN or an infinity outside the mask is a NaN
        v = (A)px * (in_mask<ND>(idx, rel, inv_r2, radius) ? (A)1 : (A)0);
      }
    }
    mass = chr_add(mass, v);
    mx = any ? chr_max(mx, v) : v;
    any = true;
    if (in_mask<ND>(idx, rel_w, inv_r2, radius)) {
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const int k = idx[d] - radius[d];
        w[d] = chr_add(w[d], (A)(k * k) * v);
      }
    } else if (!INTEGER) {
#pragma unroll
      for (int d = 0; d < ND; ++d) w[d] = chr_add(w[d], (A)0 * v);   // 0 * NaN, as the table times the window
    }
  }
  // a lane without a pixel (window smaller than the group) takes lane 0's first pixel as its
  // maximum: every window has one
  const A first = __shfl(mx, threadIdx.x % WAVE - lane);
  if (!any) mx = first;
  mass = chr_reduce<G, false>(mass);
  mx = chr_reduce<G, true>(mx);
#pragma unroll
  for (int d = 0; d < ND; ++d) w[d] = chr_reduce<G, false>(w[d]);

  if (lane == 0) {
    a.mass[feat] = (double)mass / a.scale_factor;
    a.signal[feat] = (double)mx / a.scale_factor;
    if (a.isotropic) {
      A s = w[0];
#pragma unroll
      for (int d = 1; d < ND; ++d) s = chr_add(s, w[d]);
      a.size[feat] = sqrt((double)s / (double)mass);
    } else {
#pragma unroll
      for (int d = 0; d < ND; ++d) a.size[feat * ND + d] = sqrt((double)((A)ND * w[d]) / (double)mass);
    }
  }
}

#endif  // CTREFINE_CHARACTERIZE_KERNELS_H
