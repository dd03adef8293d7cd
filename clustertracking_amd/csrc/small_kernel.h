// small_kernel.h -- refine_small_kernel: singles and pairs, 16/64 lanes per cluster, registers only
// Part of the MI355X cluster-refinement engine; included by ctrefine.hip inside its
// anonymous namespace (device code only, gfx950).
#ifndef CTREFINE_SMALL_KERNEL_H
#define CTREFINE_SMALL_KERNEL_H

// ---- small clusters: 16 lanes per cluster, everything in registers ------------------
//
// Singles and pairs with the default parameter modes (background per cluster,
// signal and positions per feature, sizes constant: fitfunc.py:356,379-387) are
// >95 % of the clusters of a typical frame.  For them the normal equations are
// tiny (4..9 variables), so four clusters share one wavefront: each 16-lane
// group runs its own LM state machine, accumulates its [J r]^T [J r] in
// registers, all-reduces it inside the 16-lane DPP row (no LDS, no MFMA padding)
// and solves it redundantly in registers.  Groups pull clusters from a global
// work counter, so a slow cluster only delays its own group.
//
// Variable order (fitfunc.py:207-263): [bg, s_0.., pos(axis 0)_0.., pos(axis 1)_0.., ...].


// all-reduce inside a group of SG lanes (8 = half a DPP row, 16 = one row, 64 = the whole wave)
template <int SG>
__device__ __forceinline__ double group_sum(double x) {
  if (SG == 8) {
    x += dpp_f64<0xB1>(x);   // quad_perm [1,0,3,2]
    x += dpp_f64<0x4E>(x);   // quad_perm [2,3,0,1]
    x += dpp_f64<0x141>(x);  // row_half_mirror: the other quad of the same eight lanes
    return x;
  }
  x = row_sum(x);
  if (SG == 64) {
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
  }
  return x;
}

enum { PH_FETCH = 0, PH_EVAL_INIT = 1, PH_EVAL_TRIAL = 2, PH_STEP_ONLY = 3, PH_DONE = 4 };

// LDS of one wavefront of the small kernel, in doubles: per group Mcur[NM] Ucur[NU] v0[NV] lo[NV] hi[NV]
template <int ND, int NF, int SG>
struct SmemS {
  static constexpr int NV = 1 + NF * (1 + ND);
  static constexpr int NR = NV + 1;               // row length incl. the residual
  static constexpr int NM = NR * (NR + 1) / 2;    // packed upper triangle
  static constexpr int NUF = ND * (ND + 1) / 2;   // second-order sums per feature: U[a<=b] = sum res J_pos_a dE/dpos_b
  static constexpr int NA = NM + NF * NUF;        // everything a pass over the window accumulates
  static constexpr int GS = NA + 3 * NV;
  static constexpr int total = (WAVE / SG) * GS;
};

// SG = lanes per cluster: 8 (eight singles per wave), 16 (four pairs per wave) or 64 (pairs: a
// quarter of the per-iteration latency, which is what bounds the slowest pair).
// (singles: at least 3 waves per SIMD = at most 168 VGPRs; measured best of 128 / 168 / 203+ with
//  two pixels per lane in flight, tools/ab_classes.py: 0.375 -> 0.305 ms for the 33 k singles of cfg 2)
//
// The statements of the kernel are in small_kernel_body.inc: the work of one wavefront, whose groups
// fit the entries order[id_begin + j], j = 0, 1, ... below id_end, j pulled from *counter.
// refine_tail_kernel (tail_kernel.h) includes the same text.  It is text and not a function on
// purpose: a fit must give the same bits whichever kernel carries it, and which multiplications
// and additions the compiler fuses follows from how it simplifies the function the code is in --
// as a function of its own, inlined into both kernels, the same statements compiled to other
// roundings than as the kernel's own.  The text expects, in scope: ND, NF, ISO, SG;
// k, counter; lane (of the wavefront); lds (SmemS<ND, NF, SG>::total doubles of the wavefront);
// order, id_begin, id_end.
template <int ND, int NF, bool ISO, int SG>
__global__ void __launch_bounds__(WAVE, NF == 1 ? 3 : 1) refine_small_kernel(const KArgs k, int* __restrict__ counter) {
  __shared__ double lds[SmemS<ND, NF, SG>::total];
  const int lane = threadIdx.x;
  const int32_t* const order = k.order;
  // the part of the bin that the launch takes: kargs.h, KArgs::split
  int id_begin = 0, id_end = k.n_bin;
  if (k.split != nullptr) {
    const int first = *k.split;
    const int skip = first < k.split_cap ? first : k.split_cap;
    id_begin = k.split_part == 2 ? first : skip;
    if (k.split_part == 1) id_end = first;
  }
#include "small_kernel_body.inc"
}

#endif  // CTREFINE_SMALL_KERNEL_H
