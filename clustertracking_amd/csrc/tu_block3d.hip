// tu_block3d.hip -- the 3D instantiations of refine_block_kernel for the gaussian (compiled on
// their own so that the engine builds in parallel); see block_kernel.h, block_table.h.  No
// CTR_FLAG_THROUGHPUT table: a 3D window has thousands of pixels, more wavefronts per cluster
// pay there.
#include <cmath>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "block_kernel.h"
#include "block_table.h"

}  // namespace

KernelInfo ctr_block_kernel_3d(int family, int ndim, int iso, int nt, int cons) {
  if (ndim != 3 || family != CTR_KFAM_GAUSS) return KernelInfo{nullptr, 0, 0};
  return block_kernel<3, false, false, CTR_FIT_GAUSS>(iso, nt, cons);
}
