// refine_prepare_kernels.h -- a refine batch from device tables (ctr_refine_prepare_device;
// include/ctrefine.h has the rule): cluster labels, the grouped order, the clusters'
// row ranges, the bounds and the feasibility of the box; and the scatter of the fit's results back
// into input row order.  Included by tu_refine_prepare.hip inside its anonymous namespace, after
// device_common.h and stage_common.h.  The kernel boundary is the only synchronisation between
// workgroups; every loop is bounded by the launch's arguments or, for the rows of a frame, by offsets
// that rp_setup_kernel has checked against them; integer atomicAdd / atomicMin only.
#ifndef CTREFINE_REFINE_PREPARE_KERNELS_H
#define CTREFINE_REFINE_PREPARE_KERNELS_H

constexpr int RP_THREADS = 256;              // a workgroup of every kernel here: 4 wavefronts

struct RpArgs {
  int ndim, np;
  long long T, N, C;             // frames, rows; clusters (scatter)
  double sep[3];
  int modes[CTR_MAX_PARAMS];
  const double* pos;
  const long long* frame_offset;
  const double* params0;
  // scratch: pos / sep, members per root, rank of the row in its frame's grouped order, clusters
  // of the frame before the root's, clusters of the frames before (the scan of the counts)
  double* spos;
  int* count;
  int* rank;
  int* local;
  int* cbase;
  int* label;
  int* size;
  int* order;
  int* feat_offset;
  int* frame_index;
  int* n_clusters;
  double* params;
  double* low;
  double* high;
  int* status;
  // scatter
  const double* fit_params;
  const double* fit_cost;
  const double* fit_std;
  double* params_out;
  double* cost_out;
  double* std_out;
};

// the templates of FitFunctions.validate_bounds: [2][CTR_MAX_PARAMS], NaN = none
struct RpBounds {
  double abs[2 * CTR_MAX_PARAMS], diff[2 * CTR_MAX_PARAMS], rel[2 * CTR_MAX_PARAMS];
};

// The caller's offsets, before any kernel follows one: from 0 to N, never falling.  Every row:
// its scaled position (the division NumPy does for cKDTree(pos / separation)), its own label, no
// member.  status[0] was zeroed in front of this kernel.
__global__ void __launch_bounds__(RP_THREADS) rp_setup_kernel(const RpArgs a) {
  const long long stride = (long long)gridDim.x * RP_THREADS;
  const long long n = a.T + 1 > a.N ? a.T + 1 : a.N;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * RP_THREADS + threadIdx.x; i < n; i += stride) {
    if (i <= a.T)
      bad |= offsets_bad(a.frame_offset, i, a.T, a.N) || (i == 0 && a.frame_offset[0] != 0) ||
             (i == a.T && a.frame_offset[i] != a.N);
    if (i < a.N) {
      for (int d = 0; d < a.ndim; ++d) a.spos[i * a.ndim + d] = a.pos[i * a.ndim + d] / a.sep[d];
      a.label[i] = (int)i;
      a.count[i] = 0;
    }
    if (i == 0) a.status[1] = a.np;
  }
  if (bad) st_agent(a.status, CTR_PREPARE_BAD_TABLE);
}

// One workgroup per frame.  Labels by label_frame (stage_common.h).  Then the members per root, and
// per row its place in the frame's order by (label, row): the rows with a smaller label, or the
// same label and a smaller index (tiles of labels through LDS).
template <int ND>
__global__ void __launch_bounds__(RP_THREADS) rp_label_kernel(const RpArgs a) {
  __shared__ double s_pos[RP_THREADS * ND];
  __shared__ int s_lab[RP_THREADS];
  if (ld_agent(a.status) != CTR_PREPARE_OK) return;
  const int tid = threadIdx.x;
  for (long long f = blockIdx.x; f < a.T; f += gridDim.x) {
    const int r0 = (int)a.frame_offset[f], r1 = (int)a.frame_offset[f + 1];
    label_frame<ND, RP_THREADS>(a.spos, a.label, r0, r1, s_pos);
    for (int i = r0 + tid; i < r1; i += RP_THREADS) atomicAdd(a.count + a.label[i], 1);
    int roots = 0;
    for (int base = r0; base < r1; base += RP_THREADS) {
      const int i = base + tid;
      const bool act = i < r1;
      const int li = act ? a.label[i] : 0;
      int rank = 0, before = 0;
      for (int tb = r0; tb < r1; tb += RP_THREADS) {
        __syncthreads();
        if (tb + tid < r1) s_lab[tid] = a.label[tb + tid];
        __syncthreads();
        const int n = r1 - tb < RP_THREADS ? r1 - tb : RP_THREADS;
        if (act)
          for (int q = 0; q < n; ++q) {
            const int lj = s_lab[q], j = tb + q;
            rank += (lj < li || (lj == li && j < i)) ? 1 : 0;
            before += (lj == j && j < li) ? 1 : 0;
          }
      }
      roots += __syncthreads_count(act && li == i ? 1 : 0);
      if (!act) continue;
      a.size[i] = ld_agent(a.count + li);
      a.rank[i] = rank;
      a.order[r0 + rank] = i;
      if (li == i) a.local[i] = before;
    }
    if (tid == 0) a.cbase[f] = roots;
    __syncthreads();
  }
}

// one workgroup: exclusive scan of the clusters per frame in place, n_clusters = their sum, and the
// end of the last cluster's rows; a refused table has no cluster
__global__ void __launch_bounds__(RP_THREADS) rp_scan_kernel(const RpArgs a) {
  if (ld_agent(a.status) != CTR_PREPARE_OK) {
    if (threadIdx.x == 0) { *a.n_clusters = 0; a.feat_offset[0] = 0; }
    return;
  }
  const int C = workgroup_scan_n<RP_THREADS, int>(
      a.T, [&](long long i) { return a.cbase[i]; }, [&](long long i, int before) { a.cbase[i] = before; });
  if (threadIdx.x == 0) { *a.n_clusters = C; a.feat_offset[C] = (int)a.N; }
}

// np.fmax / np.fmin as NumPy's scalar loop writes them: the other operand where one is NaN
__device__ __forceinline__ double rp_fmax(double x, double y) { return (x >= y || y != y) ? x : y; }
__device__ __forceinline__ double rp_fmin(double x, double y) { return (x <= y || y != y) ? x : y; }

// FitFunctions.feature_bounds for one value, term by term; nothing here may be contracted (p * (1
// - rel) fused with the p - diff beside it would round once where NumPy rounds twice)
__device__ __forceinline__ void rp_bounds(double p, const RpBounds& b, int k, double& low, double& high) {
#pragma clang fp contract(off)
  const double inf = __builtin_inf();
  const double dl = b.diff[k], rl = b.rel[k], al = b.abs[k];
  const double dh = b.diff[CTR_MAX_PARAMS + k], rh = b.rel[CTR_MAX_PARAMS + k], ah = b.abs[CTR_MAX_PARAMS + k];
  const bool lo_terms = dl == dl || rl == rl, hi_terms = dh == dh || rh == rh;
  double lo = __builtin_nan(""), hi = __builtin_nan("");
  if (dl == dl) lo = p - dl;
  if (rl == rl) {
    const double f = 1. - rl;
    const double t = p * f;
    lo = dl == dl ? rp_fmax(lo, t) : t;
  }
  if (dh == dh) hi = p + dh;
  if (rh == rh) {
    const double f = 1. + rh;
    const double t = p * f;
    hi = dh == dh ? rp_fmin(hi, t) : t;
  }
  if (!lo_terms) low = al == al ? al : -inf;
  else {
    if (al == al) lo = rp_fmax(lo, al);
    low = lo == lo ? lo : -inf;
  }
  if (!hi_terms) high = ah == ah ? ah : inf;
  else {
    if (ah == ah) hi = rp_fmin(hi, ah);
    high = hi == hi ? hi : inf;
  }
}

// One workgroup per frame: the roots write their cluster's row range and frame, every value of the
// frame's rows goes to its place in the grouped order with its bounds.
__global__ void __launch_bounds__(RP_THREADS) rp_tables_kernel(const RpArgs a, const RpBounds b) {
  if (ld_agent(a.status) != CTR_PREPARE_OK) return;
  const int tid = threadIdx.x, np = a.np;
  for (long long f = blockIdx.x; f < a.T; f += gridDim.x) {
    const int r0 = (int)a.frame_offset[f], r1 = (int)a.frame_offset[f + 1];
    for (int i = r0 + tid; i < r1; i += RP_THREADS)
      if (a.label[i] == i) {
        const int c = a.cbase[f] + a.local[i];
        a.feat_offset[c] = r0 + a.rank[i];
        a.frame_index[c] = (int)f;
      }
    const long long n = (long long)(r1 - r0) * np;
    for (long long e = tid; e < n; e += RP_THREADS) {
      const int i = r0 + (int)(e / np), k = (int)(e % np);
      const size_t dst = (size_t)(r0 + a.rank[i]) * np + k;
      const double p = a.params0[(size_t)i * np + k];
      double lo, hi;
      rp_bounds(p, b, k, lo, hi);
      a.params[dst] = p;
      a.low[dst] = lo;
      a.high[dst] = hi;
    }
  }
}

// prepare_batch's check of the box: per row for a parameter of mode var, after the loosest bound
// over the cluster for a shared one; the smallest offending parameter goes to status[1]
__global__ void __launch_bounds__(RP_THREADS) rp_feasible_kernel(const RpArgs a) {
  if (ld_agent(a.status) == CTR_PREPARE_BAD_TABLE) return;
  const long long stride = (long long)gridDim.x * RP_THREADS;
  const int C = *a.n_clusters, np = a.np;
  int worst = np;
  for (long long c = (long long)blockIdx.x * RP_THREADS + threadIdx.x; c < C; c += stride) {
    const int g0 = a.feat_offset[c], g1 = a.feat_offset[c + 1];
    for (int k = 0; k < np && k < worst; ++k) {
      const int mode = a.modes[k];
      if (mode == CTR_MODE_CONST) continue;
      bool bad = false;
      if (mode == CTR_MODE_VAR) {
        for (int g = g0; g < g1; ++g) bad |= a.low[(size_t)g * np + k] > a.high[(size_t)g * np + k];
      } else {
        double lo = __builtin_inf(), hi = -__builtin_inf();
        for (int g = g0; g < g1; ++g) {
          lo = fmin(lo, a.low[(size_t)g * np + k]);
          hi = fmax(hi, a.high[(size_t)g * np + k]);
        }
        bad = lo > hi;
      }
      if (bad) worst = k;
    }
  }
  if (worst < np) {
    atomicMin(a.status + 1, worst);
    st_agent(a.status, CTR_PREPARE_INFEASIBLE);
  }
}

// the fit's results (grouped order) back into input row order: a row's values, and from its first
// value the cost of its cluster, found by bisection of feat_offset
__global__ void __launch_bounds__(RP_THREADS) rp_scatter_kernel(const RpArgs a) {
  const long long stride = (long long)gridDim.x * RP_THREADS;
  const long long n = a.N * a.np;
  for (long long e = (long long)blockIdx.x * RP_THREADS + threadIdx.x; e < n; e += stride) {
    const long long g = e / a.np;
    const int k = (int)(e % a.np);
    const long long r = a.order[g];
    if (r < 0 || r >= a.N) continue;      // not an order that CTR_PREPARE_BATCH wrote
    a.params_out[r * a.np + k] = a.fit_params[e];
    if (a.fit_std) a.std_out[r * a.np + k] = a.fit_std[e];
    if (k == 0) {
      long long lo = 0, hi = a.C;         // the last cluster with feat_offset[c] <= g
      while (hi - lo > 1) {
        const long long mid = (lo + hi) / 2;
        if (a.feat_offset[mid] <= g) lo = mid;
        else hi = mid;
      }
      a.cost_out[r] = a.C > 0 ? a.fit_cost[lo] : __builtin_nan("");
    }
  }
}

#endif  // CTREFINE_REFINE_PREPARE_KERNELS_H
