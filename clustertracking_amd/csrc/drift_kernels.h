// drift_kernels.h -- drift of a linked video: the step of every frame, its smoothing and running
// sum, the subtraction, and the stub filter (ctr_drift_device, ctr_drift_subtract_device,
// ctr_filter_stubs_device; include/ctrefine.h has the rule).  Included by
// tu_drift.hip inside its anonymous namespace, after stage_common.h and particle_match.h (the LDS
// table particle -> row, which the two-point stage shares).  The kernel boundary is the
// only synchronisation between workgroups; every loop is bounded by the launch's arguments or, for
// the rows of a frame, by offsets that drift_check_kernel has checked against them; integer atomics
// only: every float sum is taken in an order that the input alone decides.
#ifndef CTREFINE_DRIFT_KERNELS_H
#define CTREFINE_DRIFT_KERNELS_H

constexpr int DR_THREADS = 256;         // a workgroup of every kernel here: 4 wavefronts
constexpr int DR_ROWS = 8;              // rows of frame t per thread and chunk (a chunk: DR_THREADS * DR_ROWS rows)
// DR_TILE rows of frame t - 1 in one LDS table of DR_SLOTS slots: particle_match.h, with drift_insert and drift_lookup

struct DriftArgs {
  int ndim, smoothing;
  long long threshold;
  long long T, N, P;
  const long long* frame_offset;
  const long long* particle;
  const double* pos;
  double* dx;                // [T, ndim] scratch: the step of every frame
  double* drift;             // [T, ndim] out (compute) or in (subtract)
  int* n_pairs;
  double* pos_out;
  long long* particle_out;
  int* count;
  int* status;
};

// The caller's tables, before any kernel follows an index: offsets monotone and within N (where
// there are any), particle < P (where there is one).  status[0] was zeroed in front of this kernel.
__global__ void __launch_bounds__(DR_THREADS) drift_check_kernel(const DriftArgs a) {
  const long long stride = (long long)gridDim.x * DR_THREADS;
  const long long n_off = a.frame_offset ? a.T + 1 : 0, n_par = a.particle ? a.N : 0;
  const long long n = n_off > n_par ? n_off : n_par;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * DR_THREADS + threadIdx.x; i < n; i += stride) {
    if (i < n_off) bad |= offsets_bad(a.frame_offset, i, a.T, a.N);
    if (i < n_par) bad |= a.particle[i] >= a.P;
  }
  if (bad) st_agent(a.status, CTR_DRIFT_BAD_TABLE);
}

// One workgroup per frame t: n_pairs[t] and dx[t], the mean of pos[i] - pos[j] over its pairs.
// The rows of frame t - 1 go through LDS in tiles of DR_TILE, in ascending row order, each an
// open-addressing table particle -> row (counted from the frame's first row) that keeps the lowest
// row of a repeated particle; a row of frame t without a match yet probes the tile, so the first
// tile that answers gives the lowest row of all.  The rows of frame t are taken in chunks of
// DR_THREADS * DR_ROWS, the matches of a thread's DR_ROWS rows in registers.  A thread adds the
// displacements of its rows in ascending row order; the workgroup adds the threads' sums in a
// binary tree over the thread index: the same bytes for the same table.
__global__ void __launch_bounds__(DR_THREADS) drift_pairs_kernel(const DriftArgs a) {
  __shared__ unsigned long long s_tab[DR_SLOTS];
  __shared__ double s_sum[CTR_MAX_NDIM * DR_THREADS];
  __shared__ int s_cnt[DR_THREADS];
  if (ld_agent(a.status) != CTR_DRIFT_OK) return;
  const int tid = threadIdx.x, nd = a.ndim;
  for (long long t = blockIdx.x; t < a.T; t += gridDim.x) {
    double acc[CTR_MAX_NDIM] = {0., 0., 0.};
    int cnt = 0;
    const long long q0 = t > 0 ? a.frame_offset[t - 1] : 0, r0 = a.frame_offset[t], r1 = a.frame_offset[t + 1];
    const long long q1 = t > 0 ? r0 : 0;       // frame 0 has no frame before it: no tile, no pair
    for (long long base = r0; base < r1 && q0 < q1; base += DR_THREADS * DR_ROWS) {
      int pk[DR_ROWS], jrel[DR_ROWS];
#pragma unroll
      for (int k = 0; k < DR_ROWS; ++k) {
        const long long i = base + k * DR_THREADS + tid;
        const long long p = i < r1 ? a.particle[i] : -1;
        pk[k] = p < 0 ? -1 : (int)p;           // p < P <= 2^31 - 2 (drift_check_kernel)
        jrel[k] = -1;
      }
      for (long long tb = q0; tb < q1; tb += DR_TILE) {
        __syncthreads();                       // the lookups of the tile before are done
        for (int s = tid; s < DR_SLOTS; s += DR_THREADS) s_tab[s] = DR_EMPTY;
        __syncthreads();
        const int n = q1 - tb < DR_TILE ? (int)(q1 - tb) : DR_TILE;
        for (int q = tid; q < n; q += DR_THREADS) {
          const long long p = a.particle[tb + q];
          if (p >= 0) drift_insert(s_tab, (int)p, (unsigned)(tb - q0 + q));
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < DR_ROWS; ++k)
          if (pk[k] >= 0 && jrel[k] < 0) jrel[k] = drift_lookup(s_tab, pk[k]);
      }
#pragma unroll
      for (int k = 0; k < DR_ROWS; ++k)
        if (jrel[k] >= 0) {
          const long long i = base + k * DR_THREADS + tid, j = q0 + jrel[k];
          for (int d = 0; d < nd; ++d) acc[d] += a.pos[i * nd + d] - a.pos[j * nd + d];
          ++cnt;
        }
    }
    __syncthreads();                           // the sums of the frame before are read
    for (int d = 0; d < nd; ++d) s_sum[d * DR_THREADS + tid] = acc[d];
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int w = DR_THREADS / 2; w > 0; w >>= 1) {
      if (tid < w) {
        for (int d = 0; d < nd; ++d) s_sum[d * DR_THREADS + tid] += s_sum[d * DR_THREADS + tid + w];
        s_cnt[tid] += s_cnt[tid + w];
      }
      __syncthreads();
    }
    const int n = s_cnt[0];
    if (tid < nd) a.dx[t * nd + tid] = n > 0 ? s_sum[tid * DR_THREADS] / (double)n : 0.;
    if (tid == 0) a.n_pairs[t] = n;
  }
}

// sm[t] of coordinate d: dx[t] without smoothing, else the mean of dx[u] over the frames u of the
// window [max(1, t - s + 1), t] that have a pair, added in ascending u; 0 where there is none
__device__ __forceinline__ double drift_smoothed(const DriftArgs& a, long long t, int d) {
  if (a.smoothing <= 1) return a.n_pairs[t] > 0 ? a.dx[t * a.ndim + d] : 0.;
  long long lo = t - a.smoothing + 1;
  lo = lo < 1 ? 1 : lo;
  double sum = 0.;
  int n = 0;
  for (long long u = lo; u <= t; ++u)
    if (a.n_pairs[u] > 0) { sum += a.dx[u * a.ndim + d]; ++n; }
  return n > 0 ? sum / (double)n : 0.;
}

// One workgroup: drift[t] = sm[1] + ... + sm[t], per coordinate by workgroup_scan_n -- a fixed tree
// of depth log2 of the chunk plus a carry per chunk of DR_THREADS frames, not a chain of T dependent
// adds in one lane.  A refused table gives NaN and no pair.
__global__ void __launch_bounds__(DR_THREADS) drift_scan_kernel(const DriftArgs a) {
  const int nd = a.ndim;
  if (ld_agent(a.status) != CTR_DRIFT_OK) {
    for (long long t = threadIdx.x; t < a.T; t += DR_THREADS) {
      for (int d = 0; d < nd; ++d) a.drift[t * nd + d] = __builtin_nan("");
      a.n_pairs[t] = 0;
    }
    return;
  }
  for (int d = 0; d < nd; ++d) {
    double mine = 0.;
    workgroup_scan_n<DR_THREADS, double>(
        a.T, [&](long long t) { mine = drift_smoothed(a, t, d); return mine; },
        [&](long long t, double before) { a.drift[t * nd + d] = before + mine; });
  }
}

// pos_out[i] = pos[i] - drift[frame of i]; the frame by bisection of frame_offset.  A row in no
// frame is copied; a refused table gives NaN.  pos_out may be pos: a thread reads what it writes.
__global__ void __launch_bounds__(DR_THREADS) drift_subtract_kernel(const DriftArgs a) {
  const bool ok = ld_agent(a.status) == CTR_DRIFT_OK;
  const long long stride = (long long)gridDim.x * DR_THREADS;
  const int nd = a.ndim;
  for (long long i = (long long)blockIdx.x * DR_THREADS + threadIdx.x; i < a.N; i += stride) {
    if (!ok) {
      for (int d = 0; d < nd; ++d) a.pos_out[i * nd + d] = __builtin_nan("");
      continue;
    }
    long long lo = 0, hi = a.T;           // the last frame with frame_offset[t] <= i
    while (hi - lo > 1) {
      const long long mid = (lo + hi) / 2;
      if (a.frame_offset[mid] <= i) lo = mid;
      else hi = mid;
    }
    const bool in = a.T > 0 && a.frame_offset[lo] <= i && i < a.frame_offset[a.T];
    for (int d = 0; d < nd; ++d) {
      const double p = a.pos[i * nd + d];
      a.pos_out[i * nd + d] = in ? p - a.drift[lo * nd + d] : p;
    }
  }
}

// count[p]: the rows of particle p (count was zeroed in front of this kernel)
__global__ void __launch_bounds__(DR_THREADS) drift_count_kernel(const DriftArgs a) {
  if (ld_agent(a.status) != CTR_DRIFT_OK) return;
  const long long stride = (long long)gridDim.x * DR_THREADS;
  for (long long i = (long long)blockIdx.x * DR_THREADS + threadIdx.x; i < a.N; i += stride) {
    const long long p = a.particle[i];
    if (p >= 0) atomicAdd(a.count + p, 1);
  }
}

// a row whose particle has fewer than `threshold` rows is unlinked; a refused table: every row.
// particle_out may be particle.
__global__ void __launch_bounds__(DR_THREADS) drift_stubs_kernel(const DriftArgs a) {
  const bool ok = ld_agent(a.status) == CTR_DRIFT_OK;
  const long long stride = (long long)gridDim.x * DR_THREADS;
  for (long long i = (long long)blockIdx.x * DR_THREADS + threadIdx.x; i < a.N; i += stride) {
    const long long p = a.particle[i];
    a.particle_out[i] = ok && p >= 0 && (long long)a.count[p] >= a.threshold ? p : -1;
  }
}

#endif  // CTREFINE_DRIFT_KERNELS_H
