// tu_tail.hip -- the instantiations of refine_tail_kernel: 2D, isotropic and anisotropic (compiled
// on their own so that the engine builds in parallel); see tail_kernel.h.
#include <cmath>

#include "kargs.h"

namespace {

#include "device_common.h"
#include "block_kernel.h"
#include "small_kernel.h"
#include "tail_kernel.h"

constexpr size_t LDS_CU = 160 * 1024;  // LDS of one CU

template <bool ISO>
KernelInfo tail_info() {
  static_assert(SmemT<2>::bytes <= LDS_CU, "LDS budget of one CU");
  return KernelInfo{(const void*)refine_tail_kernel<2, ISO>, SmemT<2>::bytes, 2 * WAVE};
}

}  // namespace

KernelInfo ctr_tail_kernel(int ndim, int iso) {
  if (ndim != 2) return KernelInfo{nullptr, 0, 0};
  return iso ? tail_info<true>() : tail_info<false>();
}
