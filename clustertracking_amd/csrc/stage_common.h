// stage_common.h -- what the stage units are made of: relaxed loads and stores, the ordered key of
// a double, the workgroup scan, the scan over many workgroups, the check of a caller's
// frame_offset, the cluster labelling of a frame, and on the host the grids, the error macro and
// the scratch carver.  Included inside the
// anonymous namespace of the units that use it, after device_common.h where that is included; only
// label_frame needs it (scaled_dist2).
#ifndef CTREFINE_STAGE_COMMON_H
#define CTREFINE_STAGE_COMMON_H

// ---- relaxed loads and stores ---------------------------------------------------------------
// words other lanes change through atomics: read them past the L1
__device__ __forceinline__ int ld_agent(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// words that only the lanes of this workgroup change (the labels of a frame)
__device__ __forceinline__ int ld_workgroup(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- ordered key ----------------------------------------------------------------------------
// order-preserving key of a float64 (any sign), so that an unsigned atomicMax finds the maximum.
// The plain bit map: a NaN lands above +inf with the sign bit clear and below -inf with it set.
__device__ __forceinline__ unsigned long long ordered_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ordered_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// ---- scan -----------------------------------------------------------------------------------
// Every thread of a workgroup of THREADS (a multiple of 64) calls it with its value: returns the
// sum of the values of the threads before it, `total` the sum of all.  Inclusive scan of a
// wavefront by shuffles, the wavefronts' totals through LDS; two barriers, the first of which
// lets a call follow another.
template <int THREADS, typename V>
__device__ __forceinline__ V workgroup_scan(V v, V& total) {
  __shared__ V s_wave[THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  V incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const V up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  __syncthreads();
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  V before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const V t = s_wave[w];
    if (w < wave) before += t;
    total += t;
  }
  return before + incl - v;
}

// Exclusive scan of n values by one workgroup of THREADS, a chunk of THREADS at a time with a
// carry: store(i, sum of load(0 .. i - 1)) for every i < n; returns the sum of all, in every thread.
template <int THREADS, typename V, typename Load, typename Store>
__device__ __forceinline__ V workgroup_scan_n(long long n, Load load, Store store) {
  V carry = 0;
  for (long long c = 0; c < n; c += THREADS) {
    const long long i = c + threadIdx.x;
    V total;
    const V before = workgroup_scan<THREADS, V>(i < n ? (V)load(i) : (V)0, total);
    if (i < n) store(i, carry + before);
    carry += total;
  }
  return carry;
}

// Exclusive int64 scan of n values by any number of workgroups of THREADS, in three launches; the
// kernel boundary is the only synchronisation, no workgroup waits on another.  A tile is THREADS
// consecutive values, tiles are strided over the grid, and `sums` has a word per tile.
// First launch, any grid: sums[tile] = the sum of load(i) over the tile.
template <int THREADS, typename Load>
__device__ __forceinline__ void grid_scan_sums(long long n, long long* sums, Load load) {
  const long long tiles = (n + THREADS - 1) / THREADS;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long i = tile * THREADS + threadIdx.x;
    long long total;
    workgroup_scan<THREADS, long long>(i < n ? (long long)load(i) : 0LL, total);
    if (threadIdx.x == 0) sums[tile] = total;
  }
}

// Second launch, one workgroup: the exclusive scan of the tiles' sums, in place; returns the sum of
// all n values, in every thread.
template <int THREADS>
__device__ __forceinline__ long long grid_scan_top(long long n, long long* sums) {
  return workgroup_scan_n<THREADS, long long>(
      (n + THREADS - 1) / THREADS, [&](long long k) { return sums[k]; }, [&](long long k, long long before) { sums[k] = before; });
}

// Third launch, any grid: store(i, sum of load(0 .. i - 1)) for every i < n.  load(i) and store(i)
// belong to one thread, so a scan may replace its values.
template <int THREADS, typename Load, typename Store>
__device__ __forceinline__ void grid_scan_apply(long long n, const long long* sums, Load load, Store store) {
  const long long tiles = (n + THREADS - 1) / THREADS;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long i = tile * THREADS + threadIdx.x;
    long long total;
    const long long before = workgroup_scan<THREADS, long long>(i < n ? (long long)load(i) : 0LL, total);
    if (i < n) store(i, sums[tile] + before);
  }
}

// ---- the caller's frame_offset, before an index is followed ---------------------------------
// entry i <= T of offsets that must stay within [0, N] and never fall
__device__ __forceinline__ bool offsets_bad(const long long* frame_offset, long long i, long long T, long long N) {
  const long long o = frame_offset[i];
  return o < 0 || o > N || (i < T && frame_offset[i + 1] < o);
}

// ---- cluster labelling of one frame ---------------------------------------------------------
// The rule of cKDTree(pos / separation).query_pairs(1), label = smallest row of the component.
// Every thread of a workgroup of THREADS calls it for the rows [r0, r1) of one frame; spos holds
// their scaled positions and label[i] == i; s_pos: THREADS * ND doubles of LDS.  Every row takes
// the smallest label among the rows within the scaled distance 1 (tiles of THREADS scaled
// positions through LDS; the labels themselves are read where they live, so a sweep sees what it
// has already lowered) and then the label of that label, which is a row of the same cluster with a
// label no larger; sweeps until one changes nothing.  A label only falls and always names a row of
// the cluster, so the fixed point is the smallest row of the connected component, and rows + 1
// sweeps reach it on any input.  The last thing it does is a barrier: the labels are final.
#ifdef CTREFINE_DEVICE_COMMON_H   // scaled_dist2: a unit without device_common.h has no labelling
template <int ND, int THREADS>
__device__ __forceinline__ void label_frame(const double* spos, int* label, int r0, int r1, double* s_pos) {
  const int tid = threadIdx.x;
  for (int sweep = 0; sweep <= r1 - r0; ++sweep) {
    bool changed = false;
    for (int base = r0; base < r1; base += THREADS) {
      const int i = base + tid;
      const bool act = i < r1;
      double p[ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) p[d] = act ? spos[(size_t)i * ND + d] : 0.;
      const int mine = act ? ld_workgroup(label + i) : 0;
      int m = mine;
      for (int tb = r0; tb < r1; tb += THREADS) {
        __syncthreads();
        if (tb + tid < r1) {
#pragma unroll
          for (int d = 0; d < ND; ++d) s_pos[tid * ND + d] = spos[(size_t)(tb + tid) * ND + d];
        }
        __syncthreads();
        const int n = r1 - tb < THREADS ? r1 - tb : THREADS;
        if (act)
          for (int q = 0; q < n; ++q)
            if (scaled_dist2<ND>(p, s_pos + q * ND) <= 1.) {
              const int lj = ld_workgroup(label + tb + q);
              m = lj < m ? lj : m;
            }
      }
      if (act && m < mine) {
        const int mm = ld_workgroup(label + m);
        __hip_atomic_store(label + i, mm < m ? mm : m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        changed = true;
      }
    }
    if (!__syncthreads_or(changed ? 1 : 0)) break;
  }
}
#endif  // CTREFINE_DEVICE_COMMON_H

// ---- host -----------------------------------------------------------------------------------
constexpr size_t STAGE_ALIGN = 256;          // of every part of a stage's scratch
constexpr unsigned STAGE_MAX_GRID = 1u << 16;   // grid-stride kernels: the cap of a handle unless lowered
                                                // (ctr_set_stage_max_grid); it travels as StageRun::max_grid

inline size_t align_up(size_t x) { return (x + STAGE_ALIGN - 1) / STAGE_ALIGN * STAGE_ALIGN; }

// where the next `bytes` of a scratch laid out so far up to `at` begin; moves `at` past them
inline size_t carve(size_t& at, size_t bytes) {
  const size_t here = at;
  at += align_up(bytes);
  return here;
}

// workgroups of `threads` for n elements of a grid-stride kernel: at least one, at most max_grid
inline unsigned stride_grid(long long n, int threads, unsigned max_grid) {
  const long long g = (n + threads - 1) / threads;
  return g < 1 ? 1u : g > (long long)max_grid ? max_grid : (unsigned)g;
}

// one workgroup per frame, striding past max_grid frames
inline unsigned frame_grid(long long T, unsigned max_grid) {
  return T < (long long)max_grid ? (unsigned)T : max_grid;
}

// in a launch function with `const char** msg`
#define STAGE_TRY(call)                                                            \
  do {                                                                             \
    const hipError_t e_ = (call);                                                  \
    if (e_ != hipSuccess) { *msg = hipGetErrorString(e_); return CTR_ERR_DEVICE; } \
  } while (0)

#endif  // CTREFINE_STAGE_COMMON_H
