// locate_kernels.h -- feature location on the device (include/ctrefine.h: ctr_locate_maxima_device;
// DESIGN.md 7b): the rule of reference find.grey_dilation (find.py:166-277).  Included by
// tu_locate.hip inside its anonymous namespace, which also turns floating-point contraction off:
// the threshold and the pair distances must round as NumPy and cKDTree do.
//
// One call = one pipeline on one stream:
//   loc_hist_kernel / loc_pick_kernel  per frame, the two order statistics around the
//       percentile's index among the non-zero pixels: MSB-first radix select, 8 bits per pass,
//       over order-preserving integer keys, counted in LDS and merged with integer atomics;
//       the last pick interpolates as NumPy's _lerp does.
//   loc_maxima_kernel  box maximum (separable, in LDS, a ring of plane maxima along z) compared
//       with each pixel, threshold and margin applied: one bit per pixel, a 64-bit word per
//       64 pixels of a row (one wave ballot).
//   loc_suppress_kernel  (precise) clears the bits of maxima beaten by a close neighbour.
//   loc_count_kernel / loc_scan_kernel / loc_write_kernel  ordered compaction of the bits into
//       positions in C order, frame after frame.
#ifndef CTREFINE_LOCATE_KERNELS_H
#define CTREFINE_LOCATE_KERNELS_H

constexpr int LOC_THREADS = 256;
constexpr int LOC_TX = 64;                  // tile width = one wave = one mask word
constexpr int LOC_CHUNK_WORDS = 4 * LOC_THREADS;   // mask words per compaction block
constexpr int LOC_SCAN_THREADS = 1024;      // the one workgroup of loc_scan_kernel

// ---- order-preserving keys ------------------------------------------------------------------
template <typename T> struct LocKey;
template <> struct LocKey<uint8_t> {
  static constexpr int bits = 8;
  __device__ static unsigned long long key(uint8_t v) { return v; }
  __device__ static uint8_t value(unsigned long long k) { return (uint8_t)k; }
};
template <> struct LocKey<uint16_t> {
  static constexpr int bits = 16;
  __device__ static unsigned long long key(uint16_t v) { return v; }
  __device__ static uint16_t value(unsigned long long k) { return (uint16_t)k; }
};
template <> struct LocKey<int16_t> {
  static constexpr int bits = 16;
  __device__ static unsigned long long key(int16_t v) { return (uint16_t)v ^ 0x8000u; }
  __device__ static int16_t value(unsigned long long k) { return (int16_t)(uint16_t)(k ^ 0x8000u); }
};
template <> struct LocKey<int32_t> {
  static constexpr int bits = 32;
  __device__ static unsigned long long key(int32_t v) { return (uint32_t)v ^ 0x80000000u; }
  __device__ static int32_t value(unsigned long long k) { return (int32_t)(uint32_t)(k ^ 0x80000000u); }
};
template <> struct LocKey<float> {
  static constexpr int bits = 32;
  __device__ static unsigned long long key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? (uint32_t)~b : (b | 0x80000000u);
  }
  __device__ static float value(unsigned long long k) {
    const uint32_t b = (uint32_t)k;
    return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
  }
};
template <> struct LocKey<double> {
  static constexpr int bits = 64;
  __device__ static unsigned long long key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
  }
  __device__ static double value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
  }
};

template <typename T> __device__ inline bool loc_is_nan(T v) { return v != v; }
template <typename T> __device__ inline T loc_max(T a, T b) { return a < b ? b : a; }

// pixel > threshold in the frame's type: integers against the float64 threshold, float32
// against the float32 one (stored exactly as a double), float64 against float64
template <typename T> __device__ inline bool loc_above(T v, double thr) { return (double)v > thr; }
template <> __device__ inline bool loc_above<float>(float v, double thr) { return v > (float)thr; }

// ---- percentile ------------------------------------------------------------------------------
struct LocSel {
  unsigned long long prefix[2];   // key bits found so far of the two order statistics
  long long rank[2];              // their rank among the keys that share the prefix
  long long n;                    // non-zero pixels (NaN excluded)
  int valid;                      // n > 0 and no NaN pixel
  int above;                      // virtual index at or past the last element
};

// NumPy's linear virtual index (n - 1) * q, its floor and gamma, in the arithmetic of the
// array's type (q = percentile / 100 is float32 for float32 arrays, float64 otherwise)
template <typename T> struct LocIndex {
  __device__ static void get(long long n, double pct, long long* prev, int* above, double* gamma) {
    const double q = pct / 100.0;
    const double vi = (double)(n - 1) * q;
    if (vi >= (double)(n - 1)) { *above = 1; *prev = n - 1; *gamma = vi + 1.0; return; }
    *above = 0;
    *prev = (long long)floor(vi);
    *gamma = vi - (double)*prev;
  }
};
template <> struct LocIndex<float> {
  __device__ static void get(long long n, double pct, long long* prev, int* above, double* gamma) {
    const float q = (float)pct / 100.0f;
    const float vi = (float)(n - 1) * q;
    if (vi >= (float)(n - 1)) { *above = 1; *prev = n - 1; *gamma = (double)(float)((double)vi + 1.0); return; }
    *above = 0;
    *prev = (long long)floorf(vi);
    *gamma = (double)(float)((double)vi - (double)*prev);
  }
};

// _lerp(a, b, t): a + (b - a) t, or b - (b - a)(1 - t) where t >= 0.5; b - a in the array's type
// (integers wrap), the rest in float64 (float32 for float32 arrays)
template <typename T> struct LocLerp {
  __device__ static double get(T a, T b, double t) {
    typedef typename std::make_unsigned<T>::type U;
    const T diff = (T)(U)((U)b - (U)a);
    const double d = (double)diff;
    double r = (double)a + d * t;
    if (t >= 0.5) r = (double)b - d * (1.0 - t);
    return r;
  }
};
template <> struct LocLerp<float> {
  __device__ static double get(float a, float b, double t64) {
    const float t = (float)t64;
    const float d = b - a;
    float r = a + d * t;
    if (t >= 0.5f) r = b - d * (1.0f - t);
    return (double)r;
  }
};
template <> struct LocLerp<double> {
  __device__ static double get(double a, double b, double t) {
    const double d = b - a;
    double r = a + d * t;
    if (t >= 0.5) r = b - d * (1.0 - t);
    return r;
  }
};

// grid.x = blocks_per_frame * n_frames.  Pass 0 (shift = bits - 8) counts every non-zero,
// non-NaN key into histogram 0 and the NaNs; later passes count, for each of the two order
// statistics, the keys that share its prefix.
template <typename T>
__global__ void __launch_bounds__(LOC_THREADS)
loc_hist_kernel(const T* __restrict__ frames, long long E, int bpf, int shift,
                const LocSel* __restrict__ sel, unsigned* __restrict__ hist, unsigned* __restrict__ nan_count) {
  __shared__ unsigned h[512];
  const int frame = blockIdx.x / bpf, part = blockIdx.x % bpf;
  const bool pass0 = shift + 8 == LocKey<T>::bits;
  if (!pass0 && !sel[frame].valid) return;
  for (int i = threadIdx.x; i < 512; i += LOC_THREADS) h[i] = 0;
  __syncthreads();
  const T* f = frames + (long long)frame * E;
  const unsigned long long p0 = pass0 ? 0 : sel[frame].prefix[0], p1 = pass0 ? 0 : sel[frame].prefix[1];
  const int hi = shift + 8;
  unsigned nnan = 0;
  for (long long i = (long long)part * LOC_THREADS + threadIdx.x; i < E; i += (long long)bpf * LOC_THREADS) {
    const T v = f[i];
    if (v == T(0)) continue;
    if (loc_is_nan(v)) { ++nnan; continue; }
    const unsigned long long k = LocKey<T>::key(v);
    const unsigned d = (unsigned)(k >> shift) & 255u;
    if (pass0) {
      atomicAdd(&h[d], 1u);
    } else {
      if ((k >> hi) == (p0 >> hi)) atomicAdd(&h[d], 1u);
      if ((k >> hi) == (p1 >> hi)) atomicAdd(&h[256 + d], 1u);
    }
  }
  if (nnan) atomicAdd(&nan_count[frame], nnan);
  __syncthreads();
  for (int i = threadIdx.x; i < (pass0 ? 256 : 512); i += LOC_THREADS)
    if (h[i]) atomicAdd(&hist[(long long)frame * 512 + i], h[i]);
}

// one thread per frame: picks the digit of each order statistic, clears the histogram for the
// next pass; the last pass writes the threshold (NaN: no features)
template <typename T>
__global__ void __launch_bounds__(64)
loc_pick_kernel(long long n_frames, int shift, double pct, LocSel* __restrict__ sel, unsigned* __restrict__ hist,
                const unsigned* __restrict__ nan_count, double* __restrict__ thr) {
  const long long frame = (long long)blockIdx.x * 64 + threadIdx.x;
  if (frame >= n_frames) return;
  const bool pass0 = shift + 8 == LocKey<T>::bits;
  LocSel s = sel[frame];
  unsigned* h = hist + frame * 512;
  double gamma = 0.;
  if (pass0) {
    long long n = 0;
    for (int d = 0; d < 256; ++d) n += h[d];
    s.n = n;
    s.valid = n > 0 && nan_count[frame] == 0;
    s.prefix[0] = s.prefix[1] = 0;
    long long prev = 0;
    if (s.valid) LocIndex<T>::get(n, pct, &prev, &s.above, &gamma);
    s.rank[0] = prev;
    s.rank[1] = s.above ? prev : prev + 1;
  }
  if (s.valid) {
    for (int j = 0; j < 2; ++j) {
      const unsigned* hj = h + (pass0 ? 0 : 256 * j);
      long long cum = 0;
      for (int d = 0; d < 256; ++d) {
        const long long c = hj[d];
        if (s.rank[j] < cum + c) {
          s.prefix[j] |= (unsigned long long)d << shift;
          s.rank[j] -= cum;
          break;
        }
        cum += c;
      }
    }
  }
  for (int d = 0; d < 512; ++d) h[d] = 0;
  sel[frame] = s;
  if (shift == 0) {
    double t = __longlong_as_double(0x7ff8000000000000LL);
    if (s.valid) {
      long long prev;
      int above;
      LocIndex<T>::get(s.n, pct, &prev, &above, &gamma);
      t = LocLerp<T>::get(LocKey<T>::value(s.prefix[0]), LocKey<T>::value(s.prefix[1]), gamma);
    }
    thr[frame] = t;
  }
}

// ---- local maxima ----------------------------------------------------------------------------
struct LocGeom {
  long long E;          // pixels per frame
  int nz, ny, nx, nwx;  // nz = 1 in 2D; nwx = mask words per row
  int b[3], lo[3];      // box and its lower reach -((b-1)/2) per axis (z, y, x); hi = b - 1 - lo
  long long margin[3];
  double sep[3];
  int reach[3];         // |offset| of a close neighbour is at most floor(separation)
  int ndim, ty, ring;   // rows per tile, plane maxima kept along z
  long long W;          // mask words per frame
};

// grid = (nwx * n_frames, ceil(ny / ty)); one wave per row of the tile, lane = column.
// LDS: input rows of the tile with halo [ty + by - 1][64 + bx - 1], their row maxima
// [ty + by - 1][64], and `ring` plane maxima [ring][ty][64].
template <typename T>
__global__ void __launch_bounds__(LOC_THREADS)
loc_maxima_kernel(const T* __restrict__ frames, const LocGeom g, const double* __restrict__ thr_of,
                  unsigned long long* __restrict__ mask) {
  extern __shared__ unsigned char loc_smem[];
  const int frame = blockIdx.x / g.nwx, wx = blockIdx.x % g.nwx;
  const int x0 = wx * LOC_TX, y0 = blockIdx.y * g.ty;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = g.ty + g.b[1] - 1, cols = LOC_TX + g.b[2] - 1;
  T* A = (T*)loc_smem;
  T* B = A + rows * cols;
  T* P = B + rows * LOC_TX;
  const T* f = frames + (long long)frame * g.E;
  unsigned long long* m = mask + (long long)frame * g.W;
  const double thr = thr_of[frame];
  const bool valid = !(thr != thr);
  const int hz = g.b[0] - 1 - g.lo[0];
  const int x = x0 + lane;
  for (int zi = 0; zi < g.nz + hz; ++zi) {
    if (valid && zi < g.nz) {
      const T* plane = f + (long long)zi * g.ny * g.nx;
      for (int i = threadIdx.x; i < rows * cols; i += LOC_THREADS) {
        const int r = i / cols, c = i - r * cols;
        const int gy = y0 - g.lo[1] + r, gx = x0 - g.lo[2] + c;
        A[i] = (gy >= 0 && gy < g.ny && gx >= 0 && gx < g.nx) ? plane[(long long)gy * g.nx + gx] : T(0);
      }
      __syncthreads();
      for (int i = threadIdx.x; i < rows * LOC_TX; i += LOC_THREADS) {
        const int r = i >> 6, c = i & 63;
        const T* a = A + r * cols + c;
        T v = a[0];
        for (int k = 1; k < g.b[2]; ++k) v = loc_max(v, a[k]);
        B[i] = v;
      }
      __syncthreads();
      T* ps = P + (zi % g.ring) * g.ty * LOC_TX;
      for (int i = threadIdx.x; i < g.ty * LOC_TX; i += LOC_THREADS) {
        const T* bb = B + i;
        T v = bb[0];
        for (int k = 1; k < g.b[1]; ++k) v = loc_max(v, bb[k * LOC_TX]);
        ps[i] = v;
      }
      __syncthreads();
    }
    const int z = zi - hz;
    if (z < 0) continue;
    int zlo = z - g.lo[0], zhi = z + hz;
    const bool clipped = zlo < 0 || zhi > g.nz - 1;
    zlo = zlo < 0 ? 0 : zlo;
    zhi = zhi > g.nz - 1 ? g.nz - 1 : zhi;
    for (int yy = wave; yy < g.ty; yy += LOC_THREADS / 64) {
      const int y = y0 + yy;
      if (y >= g.ny) break;
      bool is = false;
      if (valid && x < g.nx) {
        T mx = P[(zlo % g.ring) * g.ty * LOC_TX + yy * LOC_TX + lane];
        for (int zz = zlo + 1; zz <= zhi; ++zz) mx = loc_max(mx, P[(zz % g.ring) * g.ty * LOC_TX + yy * LOC_TX + lane]);
        if (clipped) mx = loc_max(mx, T(0));
        const T v = f[((long long)z * g.ny + y) * g.nx + x];
        const long long pz = z, py = y, px = x;
        is = v == mx && loc_above(v, thr) &&
             py >= g.margin[1] && py <= (long long)g.ny - g.margin[1] - 1 &&
             px >= g.margin[2] && px <= (long long)g.nx - g.margin[2] - 1 &&
             (g.ndim == 2 || (pz >= g.margin[0] && pz <= (long long)g.nz - g.margin[0] - 1));
      }
      const unsigned long long word = __ballot(is);
      if (lane == 0) m[((long long)z * g.ny + y) * g.nwx + wx] = word;
    }
    __syncthreads();   // the next plane overwrites A, B and a ring slot
  }
}

// ---- suppression of close maxima (precise) ---------------------------------------------------
// one thread per mask word: each maximum of the word is dropped when a close maximum beats it
// in the order (value, sum of pos / separation, C-order index).  Reads `cand`, writes `keep`:
// every pair is decided on the same candidate set.
template <typename T>
__global__ void __launch_bounds__(LOC_THREADS)
loc_suppress_kernel(const T* __restrict__ frames, const LocGeom g, long long n_words,
                    const unsigned long long* __restrict__ cand, unsigned long long* __restrict__ keep) {
  const long long w = (long long)blockIdx.x * LOC_THREADS + threadIdx.x;
  if (w >= n_words) return;
  const unsigned long long bits = cand[w];
  unsigned long long out = bits;
  if (bits) {
    const long long frame = w / g.W;
    long long rem = w - frame * g.W;
    const int wx = (int)(rem % g.nwx);
    rem /= g.nwx;
    const int y = (int)(rem % g.ny), z = (int)(rem / g.ny);
    const T* f = frames + frame * g.E;
    const unsigned long long* cm = cand + frame * g.W;
    const double r = 1. - 1e-7;
    const double r2 = r * r;
    const int a0 = g.ndim == 3 ? 0 : 1;
    unsigned long long todo = bits;
    while (todo) {
      const int bit = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int x = wx * 64 + bit;
      const int pi[3] = {z, y, x};
      double qi[3], si = 0.;
      for (int a = a0; a < 3; ++a) { qi[a] = (double)pi[a] / g.sep[a]; si = si + qi[a]; }
      const long long li = ((long long)z * g.ny + y) * g.nx + x;
      const T vi = f[li];
      bool beaten = false;
      const int zb = g.ndim == 3 ? max(0, z - g.reach[0]) : 0, ze = g.ndim == 3 ? min(g.nz - 1, z + g.reach[0]) : 0;
      const int yb = max(0, y - g.reach[1]), ye = min(g.ny - 1, y + g.reach[1]);
      const int xb = max(0, x - g.reach[2]), xe = min(g.nx - 1, x + g.reach[2]);
      for (int zz = zb; zz <= ze && !beaten; ++zz) {
        for (int yy = yb; yy <= ye && !beaten; ++yy) {
          const unsigned long long* row = cm + ((long long)zz * g.ny + yy) * g.nwx;
          for (int ww = xb >> 6; ww <= (xe >> 6) && !beaten; ++ww) {
            unsigned long long nb = row[ww];
            const int lo = max(xb - ww * 64, 0), hi = min(xe - ww * 64, 63);
            nb &= (~0ull << lo) & (~0ull >> (63 - hi));
            while (nb) {
              const int b2 = __builtin_ctzll(nb);
              nb &= nb - 1;
              const int xx = ww * 64 + b2;
              if (zz == z && yy == y && xx == x) continue;
              const int pj[3] = {zz, yy, xx};
              double d2 = 0., sj = 0.;
              for (int a = a0; a < 3; ++a) {
                const double qj = (double)pj[a] / g.sep[a];
                const double d = qi[a] - qj;
                d2 = d2 + d * d;
                sj = sj + qj;
              }
              if (!(d2 <= r2)) continue;
              const long long lj = ((long long)zz * g.ny + yy) * g.nx + xx;
              const T vj = f[lj];
              if (vj > vi || (vj == vi && (sj > si || (sj == si && lj > li)))) { beaten = true; break; }
            }
          }
        }
      }
      if (beaten) out &= ~(1ull << bit);
    }
  }
  keep[w] = out;
}

// ---- ordered compaction ----------------------------------------------------------------------
// grid.x = chunks_per_frame * n_frames; a chunk = LOC_CHUNK_WORDS mask words of one frame
__global__ void __launch_bounds__(LOC_THREADS)
loc_count_kernel(const unsigned long long* __restrict__ mask, long long W, int cpf, long long* __restrict__ count) {
  __shared__ long long part[LOC_THREADS / 64];
  const long long frame = blockIdx.x / cpf, chunk = blockIdx.x % cpf;
  const unsigned long long* m = mask + frame * W;
  long long c = 0;
  for (int k = 0; k < 4; ++k) {
    const long long w = chunk * LOC_CHUNK_WORDS + threadIdx.x * 4 + k;
    if (w < W) c += __popcll(m[w]);
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t = 0;
    for (int i = 0; i < LOC_THREADS / 64; ++i) t += part[i];
    count[blockIdx.x] = t;
  }
}

// one workgroup: exclusive scan of the chunk counts in (frame, chunk) order -> chunk bases,
// frame offsets and the total
__global__ void __launch_bounds__(LOC_SCAN_THREADS)
loc_scan_kernel(const long long* __restrict__ count, long long n_chunks, int cpf, long long n_frames,
                long long* __restrict__ base, int64_t* __restrict__ frame_offset, int64_t* __restrict__ total) {
  const long long n = workgroup_scan_n<LOC_SCAN_THREADS, long long>(
      n_chunks, [&](long long i) { return count[i]; },
      [&](long long i, long long before) {
        base[i] = before;
        if (i % cpf == 0) frame_offset[i / cpf] = before;
      });
  if (threadIdx.x == 0) {
    frame_offset[n_frames] = n;
    *total = n;
  }
}

__global__ void __launch_bounds__(LOC_THREADS)
loc_write_kernel(const unsigned long long* __restrict__ mask, const LocGeom g, int cpf,
                 const long long* __restrict__ base, long long capacity, int32_t* __restrict__ pos) {
  const long long frame = blockIdx.x / cpf, chunk = blockIdx.x % cpf;
  const unsigned long long* m = mask + frame * g.W;
  unsigned long long wd[4];
  long long c = 0;
  for (int k = 0; k < 4; ++k) {
    const long long w = chunk * LOC_CHUNK_WORDS + threadIdx.x * 4 + k;
    wd[k] = w < g.W ? m[w] : 0ull;
    c += __popcll(wd[k]);
  }
  long long in_chunk;
  long long row = base[blockIdx.x] + workgroup_scan<LOC_THREADS, long long>(c, in_chunk);
  for (int k = 0; k < 4; ++k) {
    unsigned long long bits = wd[k];
    if (!bits) continue;
    long long w = chunk * LOC_CHUNK_WORDS + threadIdx.x * 4 + k;
    const int wx = (int)(w % g.nwx);
    w /= g.nwx;
    const int y = (int)(w % g.ny), z = (int)(w / g.ny);
    while (bits) {
      const int bit = __builtin_ctzll(bits);
      bits &= bits - 1;
      if (row < capacity) {
        int32_t* p = pos + row * g.ndim;
        if (g.ndim == 3) { p[0] = z; p[1] = y; p[2] = wx * 64 + bit; }
        else { p[0] = y; p[1] = wx * 64 + bit; }
      }
      ++row;
    }
  }
}

#endif  // CTREFINE_LOCATE_KERNELS_H
