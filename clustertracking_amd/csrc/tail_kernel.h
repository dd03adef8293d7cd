// tail_kernel.h -- refine_tail_kernel: the likely slow clusters of three bins in one launch
// Part of the MI355X cluster-refinement engine; included by tu_tail.hip inside its anonymous
// namespace, after block_kernel.h and small_kernel.h (device code only, gfx950).
#ifndef CTREFINE_TAIL_KERNEL_H
#define CTREFINE_TAIL_KERNEL_H

// With CTR_FLAG_THROUGHPUT the step of many batches in flight is set by queue time:
// a launch holds its hardware queue until its last workgroup ends, and the pairs, the 3-4-feature
// and the 5-10-feature bins each end with a handful of clusters that iterate for milliseconds
// while the machine is mostly idle.  Those clusters -- the ones front_load_kernel puts first in
// their bins and counts -- run here instead, in one launch on one queue: the three tails overlap.
// The launch lives as long as the slowest fit of the call and uses a small part of the machine, so
// its workgroups also fit the rest of a block bin that is small (ctrefine.hip: TAIL_ABSORB), and
// every pair that would run at 64 lanes: those bins then have no launch of their own.
//
// One workgroup of two wavefronts per entry of the grid; what a workgroup does is uniform over it
// (kargs.h: TailArgs).  A cluster is fitted by the statements of its bin's own kernel, the same
// text with the same template arguments (small_kernel_body.inc, block_kernel_body.inc):
//   segment 0  pairs          refine_small_kernel<ND, 2, ISO, 64> on wavefront 0 (the other one leaves
//                             before anything: that text has no workgroup barrier)
//   segment 1  block, NT = 1  refine_block_kernel<ND, ISO, 1, 2, false>
//   segment 2  block, NT = 2  refine_block_kernel<ND, ISO, 2, 2, false>
// The workgroups of a segment pull its entries, in the bin's front-loaded order, from a counter of
// the segment (counter[segment]) until the entry is past the segment's range: the whole bin
// (TailArgs::whole) or the close clusters that front_load_kernel has counted.  The pairs' text
// does so itself, as in the bin's launch; around the block text it is the loop below: one thread
// takes the entry, an LDS word and a barrier hand it to the workgroup, and a second barrier keeps
// the next cluster's set-up out of the LDS that the write-back of this one still reads.  No
// workgroup waits for another one; a workgroup that finds its segment's range used up returns.
// Occupancy does not matter for the few hundred workgroups of a call: one per SIMD pair is asked
// for, whatever the three texts need in registers.
template <int ND>
struct SmemT {
  static constexpr size_t b1 = SmemB<1, 2, false>::bytes, b2 = SmemB<2, 2, false>::bytes,
                          bs = sizeof(double) * SmemS<ND, 2, 64>::total;
  static constexpr size_t bytes = b1 > b2 ? (b1 > bs ? b1 : bs) : (b2 > bs ? b2 : bs);
};

template <int ND, bool ISO>
__global__ void __launch_bounds__(2 * WAVE, 1) refine_tail_kernel(const KArgs k, const TailArgs t, int* __restrict__ counter) {
  extern __shared__ double smem[];
  __shared__ int tail_entry;   // the entry that the workgroup fits next (block segments)
  const int b = (int)blockIdx.x;
  // (the segments lie in the grid in the order TailArgs::grid_begin gives them: 1, 2, 0)
  const int seg = b >= t.grid_begin[0] ? 0 : (b >= t.grid_begin[2] ? 2 : 1);
  // (selected, not indexed: the arguments stay in scalar registers)
  const int32_t* close = seg == 2 ? t.close[2] : (seg == 1 ? t.close[1] : t.close[0]);
  const int whole = seg == 2 ? t.whole[2] : (seg == 1 ? t.whole[1] : t.whole[0]);
  const int off = seg == 2 ? t.ord_off[2] : (seg == 1 ? t.ord_off[1] : t.ord_off[0]);
  if (close == nullptr) return;
  const int range = whole > 0 ? whole : *close;
  const int tid = (int)threadIdx.x;
  if (seg == 0) {
    if (tid >= WAVE) return;
    constexpr int NF = 2, SG = 64;
    const int lane = tid;
    double* const lds = smem;
    const int32_t* const order = k.order + off;
    const int id_begin = 0, id_end = range;
#include "small_kernel_body.inc"
  } else if (seg == 1) {
    constexpr int NT = 1, W = 2, FIT = CTR_FIT_GAUSS;
    constexpr bool CONS = false, LP = false;
    for (;;) {
      if (tid == 0) tail_entry = atomicAdd(counter + 1, 1);
      __syncthreads();
      const int tail_next = __builtin_amdgcn_readfirstlane(tail_entry);
      if (tail_next >= range) break;
      const int cl = k.order[off + tail_next];
      {
#include "block_kernel_body.inc"
      }
      __syncthreads();
    }
  } else {
    constexpr int NT = 2, W = 2, FIT = CTR_FIT_GAUSS;
    constexpr bool CONS = false, LP = false;
    for (;;) {
      if (tid == 0) tail_entry = atomicAdd(counter + 2, 1);
      __syncthreads();
      const int tail_next = __builtin_amdgcn_readfirstlane(tail_entry);
      if (tail_next >= range) break;
      const int cl = k.order[off + tail_next];
      {
#include "block_kernel_body.inc"
      }
      __syncthreads();
    }
  }
}

#endif  // CTREFINE_TAIL_KERNEL_H
