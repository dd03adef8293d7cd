// block_table.h -- how a tu_block*.hip unit instantiates refine_block_kernel for one table of
// the handle (ctrefine.hip): a unit includes it after block_kernel.h, inside its anonymous
// namespace, and exports an entry point of the shape declared in kargs.h.

constexpr size_t LDS_CU = 160 * 1024;  // LDS of one CU

// wavefronts per cluster by NT.  throughput (CTR_FLAG_THROUGHPUT, the GAUSS_TP table): the
// fewest -- a quarter of the LDS and of the wave slots for 3-4 features; two or three workgroups
// per CU instead of one for 5-30 features
constexpr int waves(int nt, bool throughput) {
  return throughput ? (nt <= 2 ? 2 : 1) : (nt <= 2 ? 8 : (nt <= 3 ? 4 : (nt <= 6 ? 2 : 1)));
}

template <int ND, bool ISO, int NT, int W, bool CONS, bool LP, int FIT>
KernelInfo block_info() {
  static_assert(SmemB<NT, W, CONS>::bytes <= LDS_CU, "LDS budget of one CU");
  return KernelInfo{(const void*)refine_block_kernel<ND, ISO, NT, W, CONS, LP, FIT>, SmemB<NT, W, CONS>::bytes, WAVE * W};
}

// nt = 1..8; cons: the instantiation for clusters with equality constraints, nt = 1..2 only
// (at most 4 features: 29 variables, 31 for ring / disc; beyond, status 5: ctrefine.hip)
template <int ND, bool ISO, bool TP, bool LP, int FIT>
KernelInfo block_by_nt(int nt, int cons) {
  if (cons) {
    if (nt == 1) return block_info<ND, ISO, 1, waves(1, TP), true, LP, FIT>();
    if (nt == 2) return block_info<ND, ISO, 2, waves(2, TP), true, LP, FIT>();
    return KernelInfo{nullptr, 0, 0};
  }
  switch (nt) {
    case 1: return block_info<ND, ISO, 1, waves(1, TP), false, LP, FIT>();
    case 2: return block_info<ND, ISO, 2, waves(2, TP), false, LP, FIT>();
    case 3: return block_info<ND, ISO, 3, waves(3, TP), false, LP, FIT>();
    case 4: return block_info<ND, ISO, 4, waves(4, TP), false, LP, FIT>();
    case 5: return block_info<ND, ISO, 5, waves(5, TP), false, LP, FIT>();
    case 6: return block_info<ND, ISO, 6, waves(6, TP), false, LP, FIT>();
    case 7: return block_info<ND, ISO, 7, waves(7, TP), false, LP, FIT>();
    case 8: return block_info<ND, ISO, 8, waves(8, TP), false, LP, FIT>();
    default: return KernelInfo{nullptr, 0, 0};
  }
}

template <int ND, bool TP, bool LP, int FIT>
KernelInfo block_kernel(int iso, int nt, int cons) {
  return iso ? block_by_nt<ND, true, TP, LP, FIT>(nt, cons) : block_by_nt<ND, false, TP, LP, FIT>(nt, cons);
}
