// frame_max_kernels.h -- the per-frame maximum of a frame block (the norm of refine.py:354 and
// refine.py:325-331) and the one function that queues it.  Included inside the anonymous namespace
// of the units that need it (ctrefine.hip through aux_kernels.h, tu_train.hip), after
// device_common.h and stage_common.h (ordered_key).
#ifndef CTREFINE_FRAME_MAX_KERNELS_H
#define CTREFINE_FRAME_MAX_KERNELS_H

// ---- per-frame maximum (the norm of refine.py:354) --------------------------------
// Streams the frame block once: 16 B per lane per load, one ordered-u64 atomicMax
// per workgroup.  HBM-bound.

// The ordered key of a double with a rule for NaN.  A NaN has to win every maximum (NumPy's max
// propagates it), and by its bits only a NaN with the sign bit clear does: one with the sign bit
// set -- what 0 * inf, inf - inf and 0 / 0 give on x86 -- would come out below -inf and be lost,
// together with the maximum its lane had found.  So every NaN is encoded as the positive quiet NaN.
__device__ __forceinline__ unsigned long long enc_f64(double x) {
  if (x != x) return 0xfff8000000000000ull;   // = ordered_key of 0x7ff8000000000000, above +inf
  return ordered_key(x);
}

template <typename T>
__device__ __forceinline__ double chunk_max(const T* p, size_t n, int tid, int nthreads) {
  constexpr int V = 16 / sizeof(T);
  double m = -INFINITY;
  const uintptr_t addr = (uintptr_t)p;
  size_t head = (16 - (addr & 15)) & 15;
  head /= sizeof(T);
  if (head > n) head = n;
  for (size_t i = tid; i < head; i += nthreads) {
    const double x = (double)p[i];
    m = (x > m || x != x) ? x : m;
  }
  const size_t nvec = (n - head) / V;
  const uint4* pv = (const uint4*)(p + head);
  for (size_t i = tid; i < nvec; i += nthreads) {
    uint4 raw = pv[i];
    T vals[V];
    __builtin_memcpy(vals, &raw, 16);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const double x = (double)vals[j];
      m = (x > m || x != x) ? x : m;
    }
  }
  for (size_t i = head + nvec * V + tid; i < n; i += nthreads) {
    const double x = (double)p[i];
    m = (x > m || x != x) ? x : m;
  }
  return m;
}

constexpr int FM_THREADS = 256;
constexpr size_t FM_CHUNK_BYTES = 64 * 1024;

__global__ void __launch_bounds__(FM_THREADS) frame_max_kernel(const void* frames, int dtype,
                                                               size_t frame_elems, int chunks_per_frame,
                                                               size_t chunk_elems,
                                                               unsigned long long* enc) {
  const int frame = blockIdx.x / chunks_per_frame, chunk = blockIdx.x % chunks_per_frame;
  const size_t begin = (size_t)chunk * chunk_elems;
  size_t n = frame_elems - begin;
  if (n > chunk_elems) n = chunk_elems;
  const size_t e0 = (size_t)frame * frame_elems + begin;
  double m;
  switch (dtype) {
    case CTR_DTYPE_U8: m = chunk_max((const uint8_t*)frames + e0, n, threadIdx.x, FM_THREADS); break;
    case CTR_DTYPE_U16: m = chunk_max((const uint16_t*)frames + e0, n, threadIdx.x, FM_THREADS); break;
    case CTR_DTYPE_I16: m = chunk_max((const int16_t*)frames + e0, n, threadIdx.x, FM_THREADS); break;
    case CTR_DTYPE_I32: m = chunk_max((const int32_t*)frames + e0, n, threadIdx.x, FM_THREADS); break;
    case CTR_DTYPE_F32: m = chunk_max((const float*)frames + e0, n, threadIdx.x, FM_THREADS); break;
    default: m = chunk_max((const double*)frames + e0, n, threadIdx.x, FM_THREADS); break;
  }
  unsigned long long e = enc_f64(m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    unsigned long long other = __shfl_xor(e, o);
    e = other > e ? other : e;
  }
  __shared__ unsigned long long part[FM_THREADS / WAVE];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = e;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int wv = 1; wv < FM_THREADS / WAVE; ++wv) e = part[wv] > e ? part[wv] : e;
    atomicMax(enc + frame, e);
  }
}

__global__ void frame_max_decode_kernel(const unsigned long long* enc, double* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = ordered_unkey(enc[i]);
}

// bytes of a pixel of CTR_DTYPE_*; 0 for an unknown one
inline size_t host_dtype_size(int dtype) {
  switch (dtype) {
    case CTR_DTYPE_U8: return 1;
    case CTR_DTYPE_U16: case CTR_DTYPE_I16: return 2;
    case CTR_DTYPE_I32: case CTR_DTYPE_F32: return 4;
    case CTR_DTYPE_F64: return 8;
    default: return 0;
  }
}

// Queues the maxima of n_frames > 0 frames of frame_elems pixels on s: enc [n_frames] is scratch, out
// [n_frames] receives the doubles.  *too_large: the block does not fit one launch (nothing queued).
inline hipError_t queue_frame_max(const void* frames, int dtype, int64_t n_frames, int64_t frame_elems,
                                  unsigned long long* enc, double* out, hipStream_t s, bool* too_large) {
  const size_t chunk_elems = FM_CHUNK_BYTES / host_dtype_size(dtype);
  const int chunks = (int)(((size_t)frame_elems + chunk_elems - 1) / chunk_elems);
  const long long grid = (long long)n_frames * chunks;
  *too_large = grid > 0x7fffffffLL;
  if (*too_large) return hipSuccess;
  const hipError_t e = hipMemsetAsync(enc, 0, sizeof(unsigned long long) * (size_t)n_frames, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(frame_max_kernel, dim3((unsigned)grid), dim3(FM_THREADS), 0, s, frames, dtype,
                     (size_t)frame_elems, chunks, chunk_elems, enc);
  hipLaunchKernelGGL(frame_max_decode_kernel, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, s,
                     (const unsigned long long*)enc, out, n_frames);
  return hipGetLastError();
}

#endif  // CTREFINE_FRAME_MAX_KERNELS_H
