// tu_block_lp.hip -- the instantiations of refine_block_kernel for problems with a lowpass of the
// window (ctr_problem.noise_size; LP = true), 2D and 3D; see block_kernel.h, block_table.h.  One
// per (ndim, isotropic, NT, constrained): these problems are rare, they all take the wavefront
// counts of the default scheduling.
#include <cmath>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "block_kernel.h"
#include "block_table.h"

}  // namespace

KernelInfo ctr_block_kernel_lp(int family, int ndim, int iso, int nt, int cons) {
  if (family != CTR_KFAM_LOWPASS) return KernelInfo{nullptr, 0, 0};
  if (ndim == 2) return block_kernel<2, false, true, CTR_FIT_GAUSS>(iso, nt, cons);
  return block_kernel<3, false, true, CTR_FIT_GAUSS>(iso, nt, cons);
}
