// link_predict_kernels.h -- linking with prediction (ctr_link_predict_device).
// Included by tu_link.hip after link_kernels.h.  include/ctrefine.h states the rule: every row gets a
// velocity w once its level is linked, and a source is offered to the next level at the position
// that velocity predicts.
//
// The call is queued level by level, as ctr_link_device with memory > 0, whatever the memory: level
// t + 1 is searched from the velocities that level t ended with.  Per level t = 0 .. n_levels - 1,
// after link_solve_kernel (or the adaptive one) of that level:
//   link_velocity_kernel  (CTR_LINK_PREDICT_VELOCITY) grid-stride over the source window of level
//                         t + 1, one lane per row.  A row of level t first gets its w: its own
//                         velocity, or for a birth that of the nearest linked row of the level
//                         (brute force over the level; the other row's velocity is formed again
//                         from its link, not read, so no lane waits for another).  Then every row
//                         of the window that no level has linked yet gets its predicted scaled
//                         position for level t + 1.
//   link_drift_kernel     (CTR_LINK_PREDICT_DRIFT) one workgroup: the 256 partial sums of the rule,
//                         one per thread, the halving in LDS, u_t; then w = u_t for the rows of the
//                         level and the predicted scaled positions of the window, as above.
//   link_cand_predict_kernel  link_cand_kernel with the sources read from those positions.
// Every value has one owner lane, or the stated order: no float atomics, no hand-off inside a launch.
#ifndef CTREFINE_LINK_PREDICT_KERNELS_H
#define CTREFINE_LINK_PREDICT_KERNELS_H

static_assert(LNK_THREADS == 256, "the drift sum of the rule has 256 partial sums, one per thread");

// q of row i of level t, linked to source row src (the rule: one subtraction, one division)
template <int ND>
__device__ __forceinline__ void lnk_own_velocity(const LinkArgs& a, long long i, int t, int src, double* q) {
  const double dt = (double)(t - lnk_level_of(a.off, a.n_levels, src));
#pragma unroll
  for (int d = 0; d < ND; ++d) q[d] = (a.pos[i * ND + d] - a.pos[(long long)src * ND + d]) / dt;
}

// row s of level ts, with velocity v, as a source of level t_next: ppos = (p + v * age) / sr
template <int ND>
__device__ __forceinline__ void lnk_offer(const LinkArgs& a, const LinkPredictArgs& pr, long long s, int t_next,
                                          const double* v) {
  const double age = (double)(t_next - lnk_level_of(a.off, a.n_levels, s));
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    const double moved = v[d] * age;
    const double p = a.pos[s * ND + d] + moved;
    pr.ppos[s * ND + d] = p / a.sr[d];
  }
}

// the source window of level t + 1 (which holds the rows of level t, also where t + 1 is no level)
__device__ __forceinline__ long long lnk_next_window(const LinkArgs& a, int t) {
  const long long tw = (long long)t - a.memory;
  return a.off[tw > 0 ? tw : 0];
}

template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void link_velocity_kernel(LinkArgs a, LinkPredictArgs pr, int t) {
  const long long d0 = a.off[t], d1 = a.off[t + 1];
  const long long s0 = lnk_next_window(a, t);
  const bool offer = t + 1 < a.n_levels;
  const long long stride = (long long)gridDim.x * LNK_THREADS;
  for (long long s = s0 + (long long)blockIdx.x * LNK_THREADS + threadIdx.x; s < d1; s += stride) {
    double w[ND];
    if (s >= d0) {   // a row of level t: its velocity is decided now
#pragma unroll
      for (int d = 0; d < ND; ++d) w[d] = pr.v0[d];
      if (t > 0) {
        long long from = s;
        int src = a.link[s];
        if (src < 0) {   // a birth: the nearest linked row of the level, the lower row at a tie
          double best = INFINITY;
          from = -1;
          for (long long j = d0; j < d1; ++j) {
            if (a.link[j] < 0) continue;
            double d2 = 0.;
#pragma unroll
            for (int d = 0; d < ND; ++d) {
              const double df = a.spos[s * ND + d] - a.spos[j * ND + d];
              d2 += df * df;
            }
            if (from < 0 || d2 < best) { best = d2; from = j; }
          }
          if (from >= 0) src = a.link[from];
        }
        if (from >= 0) lnk_own_velocity<ND>(a, from, t, src, w);
      }
#pragma unroll
      for (int d = 0; d < ND; ++d) pr.w[s * ND + d] = w[d];
    } else {         // a remembered row: an earlier launch wrote its velocity
#pragma unroll
      for (int d = 0; d < ND; ++d) w[d] = pr.w[s * ND + d];
    }
    if (offer && !(a.memory > 0 && a.used[s])) lnk_offer<ND>(a, pr, s, t + 1, w);
  }
}

// one workgroup
template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void link_drift_kernel(LinkArgs a, LinkPredictArgs pr, int t) {
  __shared__ double s_part[ND][LNK_THREADS];
  __shared__ int s_count[LNK_THREADS];
  const int tid = threadIdx.x;
  const long long d0 = a.off[t], d1 = a.off[t + 1];
  double u[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) u[d] = pr.v0[d];
  if (t > 0) {
    double part[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) part[d] = 0.;
    int count = 0;
    for (long long i = d0 + tid; i < d1; i += LNK_THREADS) {
      const int src = a.link[i];
      if (src < 0) continue;
      double q[ND];
      lnk_own_velocity<ND>(a, i, t, src, q);
#pragma unroll
      for (int d = 0; d < ND; ++d) part[d] += q[d];
      ++count;
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) s_part[d][tid] = part[d];
    s_count[tid] = count;
    __syncthreads();
    for (int h = LNK_THREADS / 2; h > 0; h >>= 1) {
      if (tid < h) {
#pragma unroll
        for (int d = 0; d < ND; ++d) s_part[d][tid] += s_part[d][tid + h];
        s_count[tid] += s_count[tid + h];
      }
      __syncthreads();
    }
    const int m = s_count[0];
#pragma unroll
    for (int d = 0; d < ND; ++d) u[d] = m > 0 ? s_part[d][0] / (double)m : pr.u[(long long)(t - 1) * ND + d];
  }
  if (tid == 0) {
#pragma unroll
    for (int d = 0; d < ND; ++d) pr.u[(long long)t * ND + d] = u[d];
  }
  const bool offer = t + 1 < a.n_levels;
  for (long long s = lnk_next_window(a, t) + tid; s < d1; s += LNK_THREADS) {
    if (s >= d0) {
#pragma unroll
      for (int d = 0; d < ND; ++d) pr.w[s * ND + d] = u[d];
    }
    if (offer && !(a.memory > 0 && a.used[s])) lnk_offer<ND>(a, pr, s, t + 1, u);
  }
}

template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void link_cand_predict_kernel(LinkArgs a, LinkPredictArgs pr, int t_begin,
                                                                        int t_end) {
  lnk_cand<ND>(a, pr.ppos, t_begin, t_end);
}

#endif  // CTREFINE_LINK_PREDICT_KERNELS_H
