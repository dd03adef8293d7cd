// tu_block_inv.hip -- the instantiations of refine_block_kernel for the inv_series_<N> profiles
// (FIT = CTR_FIT_INV_SERIES; fitfunc.py:148-154,334-343), 2D and 3D; see block_kernel.h,
// block_table.h.  One per (ndim, isotropic, NT, constrained): these problems are rare, they all
// take the wavefront counts of the default scheduling.
#include <cmath>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "block_kernel.h"
#include "block_table.h"

}  // namespace

KernelInfo ctr_block_kernel_inv(int family, int ndim, int iso, int nt, int cons) {
  if (family != CTR_KFAM_INV_SERIES) return KernelInfo{nullptr, 0, 0};
  if (ndim == 2) return block_kernel<2, false, false, CTR_FIT_INV_SERIES>(iso, nt, cons);
  return block_kernel<3, false, false, CTR_FIT_INV_SERIES>(iso, nt, cons);
}
