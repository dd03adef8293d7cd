// tu_block2d.hip -- the 2D instantiations of refine_block_kernel for the gaussian, default and
// CTR_FLAG_THROUGHPUT wavefront counts (compiled on their own so that the engine builds in
// parallel); see block_kernel.h, block_table.h.
#include <cmath>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "block_kernel.h"
#include "block_table.h"

}  // namespace

KernelInfo ctr_block_kernel_2d(int family, int ndim, int iso, int nt, int cons) {
  if (ndim != 2) return KernelInfo{nullptr, 0, 0};
  if (family == CTR_KFAM_GAUSS) return block_kernel<2, false, false, CTR_FIT_GAUSS>(iso, nt, cons);
  if (family == CTR_KFAM_GAUSS_TP) return block_kernel<2, true, false, CTR_FIT_GAUSS>(iso, nt, cons);
  return KernelInfo{nullptr, 0, 0};
}

#ifdef CTR_STAMPS
// diagnostic build only (make stamps; tests/tools/stamps_run.py): the cycle stamps of the 2D kernels
extern "C" int ctr_debug_stamps(unsigned long long* out16, int reset) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
  if (reset) {
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z) != hipSuccess) return 1;
  }
  return 0;
}
#endif
