// engine_dims.h -- the sizes that the host's launch decision (refine_plan.h) and the kernels share.
// No HIP type: kargs.h includes it for every translation unit, refine_plan.h for the host alone.
#ifndef CTREFINE_ENGINE_DIMS_H
#define CTREFINE_ENGINE_DIMS_H

constexpr int WAVE = 64;
constexpr int MAXF = 64;      // features per cluster
constexpr int MAXNT = 8;      // 16*8 = 128 columns >= CTR_MAX_VARS + 1
constexpr int TAIL_SEGMENTS = 3;   // bins that refine_tail_kernel draws from (kargs.h: TailArgs)

#endif  // CTREFINE_ENGINE_DIMS_H
