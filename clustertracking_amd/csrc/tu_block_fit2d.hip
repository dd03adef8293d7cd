// tu_block_fit2d.hip -- the 2D instantiations of refine_block_kernel for the ring and disc
// profiles (FIT = CTR_FIT_RING / CTR_FIT_DISC; fitfunc.py:121-146), see block_kernel.h,
// block_table.h.  One per (isotropic, NT, constrained, profile): these problems take the
// wavefront counts of the default scheduling and have no lowpass variant.
#include <cmath>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "block_kernel.h"
#include "block_table.h"

}  // namespace

KernelInfo ctr_block_kernel_fit2d(int family, int ndim, int iso, int nt, int cons) {
  if (ndim != 2) return KernelInfo{nullptr, 0, 0};
  if (family == CTR_KFAM_RING) return block_kernel<2, false, false, CTR_FIT_RING>(iso, nt, cons);
  if (family == CTR_KFAM_DISC) return block_kernel<2, false, false, CTR_FIT_DISC>(iso, nt, cons);
  return KernelInfo{nullptr, 0, 0};
}
