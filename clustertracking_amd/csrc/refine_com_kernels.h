// refine_com_kernels.h -- centre-of-mass refinement of features (ctr_refine_com_device and the
// per-level step of ctr_find_link_refine_device; the rule: include/ctrefine.h).
// Included by tu_refine_com.hip inside its anonymous namespace, after device_common.h and
// characterize_kernels.h (the accumulator types, the mask rule and the group reduction are its).
//
// A group of G lanes (a 16-lane DPP row, or the wavefront) takes one feature and walks its window
// until the centre of mass stays within shift_thresh of the window's centre: the lanes stride the
// window in C order, keep partial sums of I and I * j[a] in int64 (integer frames: exact, so the
// result does not depend on G or the launch) or in float64 (float frames) and all-reduce them
// inside the group.  Every lane of a group then holds the same bits, so the decision to stop or to
// move is uniform in the group; the groups of a wavefront finish after different numbers of
// windows, which the row-local DPP steps of G = 16 allow (a lane only reads lanes of its own row,
// and a row leaves the loop as a whole).  The cross-row exchange of chr_reduce runs for G = 64
// alone, where the group is the wavefront.
#ifndef CTREFINE_REFINE_COM_KERNELS_H
#define CTREFINE_REFINE_COM_KERNELS_H

constexpr int RFC_THREADS = 256;

struct RfcArgs {
  const void* frames;
  long long frame_elems;
  int n_frames;
  int shape[3];          // frame extent per axis, (z,) y, x in slots 0 .. ND-1
  int radius[3];
  int max_iterations;
  double shift_thresh;
  // the rows: [0, n_features) with their frame from frame_offset, or (level_cnt != nullptr) the rows
  // [*level_start, *level_start + *level_cnt) of a table, all of frame `frame`
  long long n_features;
  const long long* frame_offset;
  const long long* level_start;
  const int* level_cnt;
  int frame;
  const double* pos;
  double* pos_out;       // may be pos
  double* mass;
  int* n_iter;           // or nullptr
  double* spos;          // or nullptr: pos_out / sr, the linker's scaled copy
  double sr[3];
};

template <int ND, typename T, int G>
__global__ __launch_bounds__(RFC_THREADS) void refine_com_kernel(RfcArgs a) {
  typedef typename ChrAcc<T>::type A;
  constexpr bool INTEGER = std::is_integral<T>::value;
  const int lane = threadIdx.x % G;
  const long long first = a.level_cnt ? *a.level_start : 0;
  const long long n = a.level_cnt ? (long long)*a.level_cnt : a.n_features;
  const long long stride = (long long)gridDim.x * (RFC_THREADS / G);

  int radius[ND], wshape[ND];
  double rel_w[ND], inv_r2[ND];
  int vol = 1;
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    radius[d] = a.radius[d];
    rel_w[d] = (double)radius[d];
    inv_r2[d] = 1. / ((double)radius[d] * (double)radius[d]);
    wshape[d] = 2 * radius[d] + 1;
    vol *= wshape[d];
  }

  // a group whose rows are used up leaves as a whole DPP row / wavefront (G is 16 or 64): the
  // reductions of the others never read it
  for (long long g = (long long)blockIdx.x * (RFC_THREADS / G) + threadIdx.x / G; g < n; g += stride) {
    const long long feat = first + g;
    int t = a.frame;
    if (!a.level_cnt) {   // the last t with frame_offset[t] <= feat
      int lo = 0, hi = a.n_frames - 1;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.frame_offset[mid] <= feat) lo = mid; else hi = mid - 1;
      }
      t = lo;
    }
    const T* frame = (const T*)a.frames + (size_t)t * a.frame_elems;

    // step 1: the start rounded half to even, inside [r, shape - 1 - r] (2 r + 1 <= shape is checked
    // by the host, so no window leaves the frame; fmax / fmin send a NaN to r)
    int c[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const double lo = (double)radius[d], hi = (double)(a.shape[d] - 1 - radius[d]);
      c[d] = (int)fmin(fmax(rint(a.pos[feat * ND + d]), lo), hi);
    }

    A m = 0, w[ND];
    double off[ND];
    int n_iter = 0;
    for (;;) {
      // step 2
      m = 0;
#pragma unroll
      for (int d = 0; d < ND; ++d) w[d] = 0;
      for (int p = lane; p < vol; p += G) {
        int idx[ND];
        int q = p;
#pragma unroll
        for (int d = ND - 1; d > 0; --d) { idx[d] = q % wshape[d]; q /= wshape[d]; }
        idx[0] = q;
        const bool in = in_mask<ND>(idx, rel_w, inv_r2, radius);
        if (INTEGER && !in) continue;
        size_t at = 0;
#pragma unroll
        for (int d = 0; d < ND; ++d) at = at * (size_t)a.shape[d] + (size_t)(c[d] - radius[d] + idx[d]);
        // float frames: mask * image as NumPy multiplies it (a NaN outside the mask is a NaN)
        const A v = INTEGER ? (A)frame[at] : (A)frame[at] * (in ? (A)1 : (A)0);
        m = chr_add(m, v);
#pragma unroll
        for (int d = 0; d < ND; ++d) w[d] = chr_add(w[d], v * (A)idx[d]);
      }
      m = chr_reduce<G, false>(m);
#pragma unroll
      for (int d = 0; d < ND; ++d) w[d] = chr_reduce<G, false>(w[d]);
      ++n_iter;
      bool nan = false;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const double cm = (double)w[d] / (double)m;
        off[d] = cm - (double)radius[d];
        nan = nan || cm != cm;
      }
      // step 3
      bool stop = true;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        if (nan) off[d] = 0.;
        stop = stop && fabs(off[d]) < a.shift_thresh;
      }
      if (stop || n_iter >= a.max_iterations) break;
      // step 4
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        int moved = c[d] + (off[d] > a.shift_thresh ? 1 : 0) - (off[d] < -a.shift_thresh ? 1 : 0);
        moved = moved < radius[d] ? radius[d] : moved;
        const int hi = a.shape[d] - 1 - radius[d];
        c[d] = moved > hi ? hi : moved;
      }
    }

    if (lane == 0) {
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const double p = off[d] + (double)c[d];
        a.pos_out[feat * ND + d] = p;
        if (a.spos) a.spos[feat * ND + d] = p / a.sr[d];
      }
      a.mass[feat] = (double)m;
      if (a.n_iter) a.n_iter[feat] = n_iter;
    }
  }
}

#endif  // CTREFINE_REFINE_COM_KERNELS_H
