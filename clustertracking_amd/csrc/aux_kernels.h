// aux_kernels.h -- mark_kernel, find_clusters_kernel; frame_max_kernel through frame_max_kernels.h
// Part of the MI355X cluster-refinement engine; included by ctrefine.hip inside its
// anonymous namespace (device code only, gfx950).
#ifndef CTREFINE_AUX_KERNELS_H
#define CTREFINE_AUX_KERNELS_H

// Order of the clusters inside every bin for one call: clusters with two features closer
// than a quarter of the mask radius (scaled distance, as find.py:72-93 scales by the
// separation) and clusters of more than 8 features go to the front of their bin.  Those
// are the fits that take tens of iterations and several re-window rounds; a bin lasts
// as long as its slowest cluster, so they must start first.  The results do not depend on
// the order.
struct FrontArgs { int begin[16]; int count[16]; int nbins; int keep_bin; /* bin copied as it is */ };

__global__ void front_load_kernel(const KArgs k, const FrontArgs fa, const int* __restrict__ order_in,
                                  int* __restrict__ order_out, int* __restrict__ counters, int total) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int b = -1, cl = 0;
  bool close = false;
  if (t < total) {
    b = 0;
    for (int j = 1; j < fa.nbins; ++j)
      if (t >= fa.begin[j]) b = j;
    cl = order_in[t];
    if (b == fa.keep_bin) {   // the bulk of singles keeps its (frame) order
      order_out[t] = cl;
      b = -1;
    } else {
      const int f0 = k.feat_offset[cl], n = k.feat_offset[cl + 1] - f0;
      const int np = k.prob.n_params, nd = k.prob.ndim;
      close = n > 8;
      for (int i = 0; i < n && !close; ++i)
        for (int j = i + 1; j < n && !close; ++j) {
          double d2 = 0.;
          for (int a = 0; a < nd; ++a) {
            const double d = (k.params[(size_t)(f0 + i) * np + 2 + a] - k.params[(size_t)(f0 + j) * np + 2 + a]) /
                             (double)k.prob.radius[a];
            d2 += d * d;
          }
          if (d2 < 0.0625) close = true;
        }
    }
  }
  // one pair of atomics per wave and bin instead of one per cluster (all on two addresses)
  unsigned long long todo = __ballot(b >= 0);
  while (todo != 0ull) {
    const int leader = __builtin_ctzll(todo);
    const int lb = __shfl(b, leader);
    const unsigned long long same = __ballot(b == lb);
    const unsigned long long mc = __ballot(b == lb && close), mf = same & ~mc;
    int basec = 0, basef = 0;
    if (lane == leader) {
      basec = atomicAdd(&counters[2 * lb], __popcll(mc));
      basef = atomicAdd(&counters[2 * lb + 1], __popcll(mf));
    }
    basec = __shfl(basec, leader);
    basef = __shfl(basef, leader);
    if (b == lb) {
      const unsigned long long below = (1ull << lane) - 1ull;
      const int pos = close ? basec + __popcll(mc & below) : fa.count[lb] - 1 - (basef + __popcll(mf & below));
      order_out[fa.begin[lb] + pos] = cl;
    }
    todo &= ~same;
  }
}

// Head start for the workgroups that need a large contiguous piece of LDS (block kernel):
// the small kernels allocate ~1 KB of LDS per wave all over every CU, and once they have
// flooded the machine a 70..150 KB request finds no contiguous room until they drain.
// One wave that waits `ticks` of the 100 MHz clock, ahead of the small kernels in their streams.
__global__ void delay_kernel(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// ctr_batch.result_rows: [N, n_params + 1] = params_out and the cost of the row's cluster
__global__ void result_rows_kernel(const double* __restrict__ params_out, const double* __restrict__ cost,
                                   const int32_t* __restrict__ feat_offset, int n_clusters, int n_features,
                                   int np, double* __restrict__ rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_features) return;
  int lo = 0, hi = n_clusters;   // the cluster c with feat_offset[c] <= i < feat_offset[c + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (feat_offset[mid] <= i) lo = mid; else hi = mid;
  }
  for (int q = 0; q < np; ++q) rows[(size_t)i * (np + 1) + q] = params_out[(size_t)i * np + q];
  rows[(size_t)i * (np + 1) + np] = cost[lo];
}

// clusters the engine cannot take (too many variables / features)
__global__ void mark_kernel(const KArgs k, int code) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= k.n_bin) return;
  const int cl = k.order[t];
  const int np = k.prob.n_params;
  for (int e = k.feat_offset[cl] * np; e < k.feat_offset[cl + 1] * np; ++e) {
    k.params_out[e] = k.params[e];
    if (k.params_std) k.params_std[e] = NAN;
  }
  k.status[cl] = code;
  k.cost[cl] = NAN;
  k.n_rounds[cl] = 0;
  k.n_iter[cl] = 0;
}


// ---- cluster labelling (reference find.py:72-93): which features are fitted together ----
// Features of one frame closer than `separation` (per-axis scaled Euclidean distance <= 1,
// the criterion of cKDTree(pos / separation).query_pairs(1)) share a cluster.  One workgroup
// per frame; label propagation to the smallest row index of the cluster until nothing
// changes (label_frame, stage_common.h).  The label is canonical (the reference's ids depend
// on Python set order); the PARTITION is the reference's.
constexpr int FC_THREADS = 256;

// (scaled_dist2, the no-contraction distance of the pair test, lives in device_common.h: the
// relocation kernels share it)
template <int ND>
__global__ void __launch_bounds__(FC_THREADS) find_clusters_kernel(const double* __restrict__ pos,
                                                                   const int32_t* __restrict__ frame_offset,
                                                                   double s0, double s1, double s2,
                                                                   double* __restrict__ spos, int32_t* label,
                                                                   int32_t* __restrict__ count,
                                                                   int32_t* __restrict__ size_out) {
  __shared__ double s_pos[FC_THREADS * ND];
  const int f = blockIdx.x;
  const int r0 = frame_offset[f], r1 = frame_offset[f + 1];
  const double sep[3] = {s0, s1, s2};
  for (int i = r0 + threadIdx.x; i < r1; i += FC_THREADS) {
#pragma unroll
    for (int a = 0; a < ND; ++a) spos[(size_t)i * ND + a] = pos[(size_t)i * ND + a] / sep[a];
    label[i] = i;
  }
  __syncthreads();
  label_frame<ND, FC_THREADS>(spos, label, r0, r1, s_pos);
  // labels of this frame are final: root = smallest row index; count members, then sizes
  for (int i = r0 + threadIdx.x; i < r1; i += FC_THREADS) atomicAdd(&count[label[i]], 1);
  __syncthreads();
  for (int i = r0 + threadIdx.x; i < r1; i += FC_THREADS) size_out[i] = ld_agent(&count[label[i]]);
}

#include "frame_max_kernels.h"

// ctr_batch.done_flag: one store, queued behind everything else of the call
__global__ void done_flag_kernel(int64_t* flag, int64_t value) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    __threadfence_system();
    __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

#endif  // CTREFINE_AUX_KERNELS_H
