// link_kernels.h -- frame-to-frame linking on the device (ctr_link_device).
// Included by tu_link.hip inside its anonymous namespace, after device_common.h and stage_common.h, and by
// tu_findlink.hip, whose loop (findlink_kernels.h) runs these kernels and the two device functions of
// link_solve_kernel (lnk_components, lnk_hungarian) on a table that grows by the relocated rows.
//
// The rule (reference Linker, find_link.py:579-733, as clustertracking_amd/link.py restates it).
// Per level t >= 1, destinations = the rows of level t, sources = the rows of the levels
// t - 1 - memory .. t - 1 that no earlier level has linked (the previous level and the remembered
// features at their last position), all positions divided per axis by search_range:
//   candidates    per destination its up to 10 nearest sources at squared distance <= (1 + 1e-7)^2;
//   sub-networks  connected components of the candidate graph;
//   links         inside a sub-network the set of links (a source and a destination at most once,
//                 along candidates only) that maximises sum(2 - d^2); more than 30 sources is the
//                 reference's SubnetOversizeException (status 1), more than 64 destinations is
//                 beyond this engine (status 2);
//   ids           level 0 counts its rows; a linked destination takes its source's id; the
//                 unlinked destinations of a level start tracks in lexicographic order of their
//                 unscaled position, numbered from the running count.
//
// A remembered source is a ROW of an earlier level, so "memory" needs no list: `used[row]` says
// that the row has been linked as a source, and the sources of level t are the unused rows of a
// window of levels.  Kernels, all on one stream, a kernel boundary between any two that exchange
// data (no hand-off between workgroups inside a launch):
//   link_prep_kernel    pos / search_range once per row; link = -1
//   link_cand_kernel    one lane per destination: brute force over its source window, the ten
//                       nearest kept sorted in registers.  Cost per level pair: n_dst * n_src
//                       distance evaluations (times memory + 1), whatever the number of features
//   link_solve_kernel   one workgroup per level.  Labels of the candidate graph by min-propagation
//                       (label = smallest destination row of the component) in HBM scratch, so a
//                       level of any size fits; 1 x 1 sub-networks are linked by the lane that owns
//                       the destination; the members of every other one are chained to its root,
//                       and one WAVEFRONT per such sub-network solves the assignment: cost block
//                       30 x 64 in LDS, shortest augmenting paths (Hungarian) with one lane per
//                       column (destinations, then one "no link" column of cost 0 per source)
//   link_rank_kernel    births: lexicographic rank inside the level, count per level
//   link_scan_kernel    running count of the births -> first id of every level, n_tracks
//   link_jump_kernel    pointer jumping along the source rows, ceil(log2(n_levels)) rounds
//   link_ids_kernel     id = first id of the root's level + the root's rank
// memory == 0: every kernel is launched once for the whole video.  memory > 0: level t needs the
// `used` flags of level t - 1, so link_cand / link_solve are queued level by level (one workgroup
// each for solve); the host waits for nothing in between.
//
// ctr_link_adaptive_device (include/ctrefine.h states the rule) launches link_solve_adaptive_kernel in
// the place of link_solve_kernel, on either path: the same level solver with the rounds of the
// adaptive search range looped inside the level's workgroup (lnk_solve_level<true>).
// ctr_link_predict_device: link_predict_kernels.h.
#ifndef CTREFINE_LINK_KERNELS_H
#define CTREFINE_LINK_KERNELS_H

constexpr int LNK_THREADS = 256;
constexpr int LNK_WAVES = LNK_THREADS / 64;
constexpr int LNK_MAXC = 10;       // candidates per destination (find_link.py:586)
constexpr int LNK_MAX_SRC = 30;    // sources per sub-network (find_link.py:582)
constexpr int LNK_MAX_DST = 64;    // destinations per sub-network: the solver's capacity
constexpr double LNK_BIG = 1e6;    // cost of a pair that is no candidate
constexpr int LNK_NONE = 0x7fffffff;

struct LinkArgs {
  int ndim, memory, n_levels;
  long long n;
  const double* pos;
  const long long* off;
  double sr[3];
  long long* particle;
  long long* n_tracks;
  int* status;
  // scratch of the handle
  double* spos;     // [N, ndim] pos / search_range
  double* cand_d2;  // [N, 10]
  int* cand_row;    // [N, 10]
  int* ncand;       // [N]
  int* link;        // [N] source row or -1
  int* lab_d;       // [N] label of a destination row
  int* lab_s;       // [N] label of a source row
  int* cnt_s;       // [N] destinations that list this source
  int* head_d;      // [N] by root row: first destination of the component, then next_d
  int* head_s;      // [N] by root row: first source of the component, then next_s
  int* next_d;
  int* next_s;
  int* roots;       // [N] roots of the non-trivial components of a level, from off[t]
  int* used;        // [N] row has been linked as a source (memory > 0)
  int* rank;        // [N] rank of a birth inside its level
  int* anc;         // [N] pointer jumping
  int* nbirth;      // [n_levels]
  long long* base;  // [n_levels + 1]
};

// the level of row i < off[n_levels]: the smallest t with off[t + 1] > i
__device__ __forceinline__ int lnk_level_of(const long long* off, int n_levels, long long i) {
  int lo = 0, hi = n_levels - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid + 1] > i) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ void lnk_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void lnk_report(int* status, int code, int level, int size) {
  if (atomicCAS(&status[0], 0, code) == 0) {
    st_agent(&status[1], level);
    st_agent(&status[2], size);
  }
}

template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void link_prep_kernel(LinkArgs a) {
  const long long stride = (long long)gridDim.x * LNK_THREADS;
  for (long long i = (long long)blockIdx.x * LNK_THREADS + threadIdx.x; i < a.n; i += stride) {
#pragma unroll
    for (int d = 0; d < ND; ++d) a.spos[i * ND + d] = a.pos[i * ND + d] / a.sr[d];
    a.link[i] = -1;
  }
}

// src: the scaled positions the sources are offered at, [N, ND]: a.spos, or the predicted ones
// (link_predict_kernels.h)
template <int ND>
__device__ __forceinline__ void lnk_cand(const LinkArgs& a, const double* src, int t_begin, int t_end) {
  const long long r0 = a.off[t_begin], r1 = a.off[t_end];
  const long long stride = (long long)gridDim.x * LNK_THREADS;
  const double bound = (1. + 1e-7) * (1. + 1e-7);
  for (long long i = r0 + (long long)blockIdx.x * LNK_THREADS + threadIdx.x; i < r1; i += stride) {
    const int t = lnk_level_of(a.off, a.n_levels, i);
    const long long tw = (long long)t - 1 - a.memory;
    const long long s0 = a.off[tw > 0 ? tw : 0], s1 = a.off[t];
    double pd[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) pd[d] = a.spos[i * ND + d];
    double bd[LNK_MAXC];
    int br[LNK_MAXC];
#pragma unroll
    for (int k = 0; k < LNK_MAXC; ++k) { bd[k] = INFINITY; br[k] = LNK_NONE; }
    for (long long s = s0; s < s1; ++s) {
      if (a.memory > 0 && a.used[s]) continue;
      double d2 = 0.;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const double df = pd[d] - src[s * ND + d];
        d2 += df * df;
      }
      if (!(d2 <= bound)) continue;
      double cd = d2;
      int cr = (int)s;
#pragma unroll
      for (int k = 0; k < LNK_MAXC; ++k) {
        if (cd < bd[k] || (cd == bd[k] && cr < br[k])) {
          const double td = bd[k];
          const int tr = br[k];
          bd[k] = cd; br[k] = cr;
          cd = td; cr = tr;
        }
      }
    }
    int n = 0;
#pragma unroll
    for (int k = 0; k < LNK_MAXC; ++k) {
      a.cand_d2[i * LNK_MAXC + k] = bd[k];
      a.cand_row[i * LNK_MAXC + k] = br[k];
      n += br[k] != LNK_NONE;
    }
    a.ncand[i] = n;
  }
}

template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void link_cand_kernel(LinkArgs a, int t_begin, int t_end) {
  lnk_cand<ND>(a, a.spos, t_begin, t_end);
}

// The sub-networks of one level: destinations [d0, d1), source window [w0, w1).  Every thread of the
// workgroup calls it; s_changed: one word of LDS.  After it lab_d / lab_s hold the label of the
// component (its smallest destination row; LNK_NONE: a source no destination lists) and cnt_s the
// destinations that list a source; the last thing it does is a barrier.  ncand: the edges of
// destination row i are the first ncand[i] entries of its candidate list (a.ncand: all of them; a
// round of the adaptive linker: the prefix within its range, 0 for a row that is settled).
__device__ __forceinline__ void lnk_components_of(const LinkArgs& a, const int* ncand, long long d0, long long d1,
                                                  long long w0, long long w1, int tid, int* s_changed) {
  // ---- initial state of this level's words
  for (long long s = w0 + tid; s < w1; s += LNK_THREADS) {
    st_agent(&a.lab_s[s], LNK_NONE);
    st_agent(&a.cnt_s[s], 0);
  }
  for (long long i = d0 + tid; i < d1; i += LNK_THREADS) {
    st_agent(&a.lab_d[i], (int)i);
    st_agent(&a.head_d[i], -1);
    st_agent(&a.head_s[i], -1);
  }
  __syncthreads();
  for (long long i = d0 + tid; i < d1; i += LNK_THREADS) {
    const int nc = ncand[i];
    for (int k = 0; k < nc; ++k) atomicAdd(&a.cnt_s[a.cand_row[i * LNK_MAXC + k]], 1);
  }
  __syncthreads();

  // ---- components: every edge pulls both ends to the smaller label until a pass changes nothing
  for (;;) {
    if (tid == 0) *s_changed = 0;
    __syncthreads();
    bool changed = false;
    for (long long i = d0 + tid; i < d1; i += LNK_THREADS) {
      const int nc = ncand[i];
      if (nc == 0) continue;
      const int mine = ld_agent(&a.lab_d[i]);
      int m = mine;
      for (int k = 0; k < nc; ++k) {
        const int l = ld_agent(&a.lab_s[a.cand_row[i * LNK_MAXC + k]]);
        m = l < m ? l : m;
      }
      for (int k = 0; k < nc; ++k)
        if (atomicMin(&a.lab_s[a.cand_row[i * LNK_MAXC + k]], m) > m) changed = true;
      if (m < mine) { st_agent(&a.lab_d[i], m); changed = true; }
    }
    if (changed) *s_changed = 1;
    __syncthreads();
    const int again = *s_changed;
    __syncthreads();
    if (!again) break;
  }
}

__device__ __forceinline__ void lnk_components(const LinkArgs& a, long long d0, long long d1, long long w0,
                                               long long w1, int tid, int* s_changed) {
  lnk_components_of(a, a.ncand, d0, d1, w0, w1, tid, s_changed);
}

// The assignment of one sub-network by one wavefront: shortest augmenting paths (Hungarian), one lane
// per column.  cost: [ns][LNK_MAX_DST] in LDS, columns 1..nd the destinations, nd+1..nd+ns one "no
// link" column of cost 0 per source; u [ns + 1], p and way [nd + ns + 1] zeroed by the caller.
// After it p[c] is the row (1-based source) of column c, 0: none.
__device__ __forceinline__ void lnk_hungarian(const double* cost, double* u, unsigned char* p, unsigned char* way,
                                              int ns, int nd, int lane) {
  const int m = nd + ns;
  const int c0 = lane + 1, c1 = lane + 65;   // this lane's columns (c1 is always a "no link" one)
  double v0 = 0., v1 = 0.;
  for (int i = 1; i <= ns; ++i) {
    if (lane == 0) p[0] = (unsigned char)i;
    lnk_wave_sync();
    int j0 = 0;
    double mv0 = INFINITY, mv1 = INFINITY;
    bool us0 = false, us1 = false;
    for (;;) {
      if (j0 == c0) us0 = true;
      if (j0 == c1) us1 = true;
      const int i0 = p[j0];
      const double ui0 = u[i0];
      double delta = INFINITY;
      int j1 = LNK_NONE;
      if (c0 <= m && !us0) {
        const double cst = c0 <= nd ? cost[(i0 - 1) * LNK_MAX_DST + lane] : 0.;
        const double cur = cst - ui0 - v0;
        if (cur < mv0) { mv0 = cur; way[c0] = (unsigned char)j0; }
        delta = mv0; j1 = c0;
      }
      if (c1 <= m && !us1) {
        const double cur = 0. - ui0 - v1;
        if (cur < mv1) { mv1 = cur; way[c1] = (unsigned char)j0; }
        if (mv1 < delta) { delta = mv1; j1 = c1; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(delta, o);
        const int oj = __shfl_xor(j1, o);
        if (od < delta || (od == delta && oj < j1)) { delta = od; j1 = oj; }
      }
      lnk_wave_sync();   // ui0 is read by every lane before a row's u moves
      if (lane == 0) u[p[0]] += delta;
      if (c0 <= m) {
        if (us0) { u[p[c0]] += delta; v0 -= delta; }
        else mv0 -= delta;
      }
      if (c1 <= m) {
        if (us1) { u[p[c1]] += delta; v1 -= delta; }
        else mv1 -= delta;
      }
      j0 = j1;
      lnk_wave_sync();
      if (p[j0] == 0) break;
    }
    if (lane == 0) {
      do {
        const int j1 = way[j0];
        p[j0] = p[j1];
        j0 = j1;
      } while (j0);
    }
    lnk_wave_sync();
  }
}

// The adaptive search range (include/ctrefine.h: ctr_link_adaptive): what the adaptive
// instantiation of the level solver takes besides LinkArgs.
struct LinkAdaptiveArgs {
  double stop_rel, step;
  int max_rounds;
  int* around;      // [N] out or null: the round a destination row was settled in (zeroed by the call)
  // scratch of the handle
  int* nc_k;        // [N] a destination row's edges in the current round: a prefix of its candidates
  int* over;        // [N] by root row: k + 1 where the root's sub-network was oversize in round k (zeroed by the call)
};

// One level: destinations [off[t], off[t + 1]), every thread of the workgroup.  ADAPTIVE: rounds
// k = 0, 1, .. inside the workgroup.  Round 0 is the plain linker's.  A wavefront that meets an
// oversize sub-network at rho_k > stop_rel stamps its root (over[root] = k + 1) and raises the LDS
// word s_over; in round k + 1 the rows whose label carries that stamp are the active ones, their
// edges are the prefix of their sorted candidates with d2 <= (rho_{k+1} (1 + 1e-7))^2 (nc_k; every
// other row: 0, so labelling, chaining and solving pass it by), and a row that keeps no edge is
// settled by its owner lane.  Every barrier is uniform: s_over is read by all after a barrier.
template <bool ADAPTIVE>
__device__ __forceinline__ void lnk_solve_level(const LinkArgs& a, const LinkAdaptiveArgs& ad, int t) {
  __shared__ double s_cost[LNK_WAVES][LNK_MAX_SRC * LNK_MAX_DST];
  __shared__ double s_u[LNK_WAVES][LNK_MAX_SRC + 2];
  __shared__ int s_src[LNK_WAVES][LNK_MAX_SRC];
  __shared__ int s_dst[LNK_WAVES][LNK_MAX_DST];
  __shared__ unsigned char s_p[LNK_WAVES][LNK_MAX_SRC + LNK_MAX_DST + 2];
  __shared__ unsigned char s_way[LNK_WAVES][LNK_MAX_SRC + LNK_MAX_DST + 2];
  __shared__ int s_changed, s_nroots, s_over;

  const int tid = threadIdx.x;
  const long long d0 = a.off[t], d1 = a.off[t + 1];
  const long long tw = (long long)t - 1 - a.memory;
  const long long w0 = a.off[tw > 0 ? tw : 0], w1 = d0;
  if (d0 == d1 || w0 == w1) return;   // no destination or no source: nothing links (uniform)

  double rho = 1.;
  for (int round = 0;; ++round) {
    const int* ncand = ADAPTIVE && round ? ad.nc_k : a.ncand;
    if (tid == 0) {
      s_nroots = 0;
      if (ADAPTIVE) s_over = 0;
    }
    lnk_components_of(a, ncand, d0, d1, w0, w1, tid, &s_changed);

    // ---- 1 x 1 sub-networks link here; the others are chained to their root
    for (long long i = d0 + tid; i < d1; i += LNK_THREADS) {
      const int nc = ncand[i];
      if (nc == 0) continue;
      const int c = a.cand_row[i * LNK_MAXC];
      if (nc == 1 && ld_agent(&a.cnt_s[c]) == 1) {
        a.link[i] = c;
        if (a.memory > 0) a.used[c] = 1;
        st_agent(&a.cnt_s[c], 0);          // not a member of a chained component
        if (ADAPTIVE && round && ad.around) ad.around[i] = round;
        continue;
      }
      const int root = ld_agent(&a.lab_d[i]);
      if (root == (int)i) st_agent(&a.roots[d0 + atomicAdd(&s_nroots, 1)], (int)i);
      st_agent(&a.next_d[i], atomicExch(&a.head_d[root], (int)i));
    }
    __syncthreads();   // the 1 x 1 sources are marked (cnt_s = 0) before the sources are chained
    for (long long s = w0 + tid; s < w1; s += LNK_THREADS) {
      if (ld_agent(&a.cnt_s[s]) == 0) continue;
      const int root = ld_agent(&a.lab_s[s]);
      st_agent(&a.next_s[s], atomicExch(&a.head_s[root], (int)s));
    }
    __syncthreads();

    // ---- one wavefront per non-trivial sub-network
    const int w = tid >> 6, lane = tid & 63;
    const int nroots = s_nroots;
    for (int ri = w; ri < nroots; ri += LNK_WAVES) {
      const int root = ld_agent(&a.roots[d0 + ri]);
      int ns = 0, nd = 0;
      if (lane == 0) {   // members in ascending row order, whatever order they were chained in
        for (int j = ld_agent(&a.head_s[root]); j >= 0; j = ld_agent(&a.next_s[j])) {
          if (ns < LNK_MAX_SRC) {
            int q = ns;
            for (; q > 0 && s_src[w][q - 1] > j; --q) s_src[w][q] = s_src[w][q - 1];
            s_src[w][q] = j;
          }
          ++ns;
        }
        for (int j = ld_agent(&a.head_d[root]); j >= 0; j = ld_agent(&a.next_d[j])) {
          if (nd < LNK_MAX_DST) {
            int q = nd;
            for (; q > 0 && s_dst[w][q - 1] > j; --q) s_dst[w][q] = s_dst[w][q - 1];
            s_dst[w][q] = j;
          }
          ++nd;
        }
      }
      ns = __shfl(ns, 0);
      nd = __shfl(nd, 0);
      if (ADAPTIVE && (ns > LNK_MAX_SRC || nd > LNK_MAX_DST) && rho > ad.stop_rel && round < ad.max_rounds) {
        if (lane == 0) {   // its members come back in the next round, at a smaller range
          st_agent(&ad.over[root], round + 1);
          s_over = 1;
        }
        continue;
      }
      if (ns > LNK_MAX_SRC) { if (lane == 0) lnk_report(a.status, 1, t, ns); continue; }
      if (nd > LNK_MAX_DST) { if (lane == 0) lnk_report(a.status, 2, t, nd); continue; }
      lnk_wave_sync();
      for (int q = lane; q < ns * LNK_MAX_DST; q += 64) s_cost[w][q] = LNK_BIG;
      const int m = nd + ns;   // columns 1..nd: destinations; nd+1..m: "no link", cost 0
      for (int q = lane; q <= m; q += 64) { s_p[w][q] = 0; s_way[w][q] = 0; }
      if (lane <= ns) s_u[w][lane] = 0.;
      lnk_wave_sync();
      if (lane < nd) {
        const long long i = s_dst[w][lane];
        const int nc = ADAPTIVE ? ld_agent(&ncand[i]) : ncand[i];   // nc_k[i] is another lane's word
        for (int k = 0; k < nc; ++k) {
          const int c = a.cand_row[i * LNK_MAXC + k];
          int sl = 0;
          while (sl < ns && s_src[w][sl] != c) ++sl;
          if (sl < ns) s_cost[w][sl * LNK_MAX_DST + lane] = a.cand_d2[i * LNK_MAXC + k] - (ADAPTIVE ? 2. * (rho * rho) : 2.);
        }
        if (ADAPTIVE && round && ad.around) ad.around[i] = round;
      }
      lnk_wave_sync();

      lnk_hungarian(s_cost[w], s_u[w], s_p[w], s_way[w], ns, nd, lane);
      const int c0 = lane + 1;
      if (lane < nd) {
        const int r = s_p[w][c0];
        if (r && s_cost[w][(r - 1) * LNK_MAX_DST + lane] < 0.5 * LNK_BIG) {
          const int src = s_src[w][r - 1];
          a.link[s_dst[w][lane]] = src;
          if (a.memory > 0) a.used[src] = 1;
        }
      }
      lnk_wave_sync();
    }
    if (!ADAPTIVE) break;

    __syncthreads();
    const int over = s_over;
    __syncthreads();    // every thread has read the word before thread 0 clears it for the next round
    if (!over) break;   // uniform: every thread read the same word after the barrier
    // ---- the cut to rho_{k+1}: only the rows of the stamped roots stay active
    rho *= ad.step;
    const double b = rho * (1. + 1e-7);
    const double b2 = b * b;
    for (long long i = d0 + tid; i < d1; i += LNK_THREADS) {
      const int prev = ncand[i];
      int n = 0;
      if (prev > 0 && ld_agent(&ad.over[ld_agent(&a.lab_d[i])]) == round + 1) {
        while (n < prev && a.cand_d2[i * LNK_MAXC + n] <= b2) ++n;
        if (n == 0 && ad.around) ad.around[i] = round + 1;   // the cut took its last edge
      }
      ad.nc_k[i] = n;
    }
    // the next thing another lane reads of these rows comes after the barriers of lnk_components_of
  }
}

// One workgroup per level t = t_begin + blockIdx.x.
__global__ __launch_bounds__(LNK_THREADS) void link_solve_kernel(LinkArgs a, int t_begin) {
  lnk_solve_level<false>(a, LinkAdaptiveArgs{}, t_begin + (int)blockIdx.x);
}

__global__ __launch_bounds__(LNK_THREADS) void link_solve_adaptive_kernel(LinkArgs a, LinkAdaptiveArgs ad, int t_begin) {
  lnk_solve_level<true>(a, ad, t_begin + (int)blockIdx.x);
}

// row j comes before row i: positions compared axis by axis; equal positions keep their row order
// (a stable sort)
template <int ND>
__device__ __forceinline__ bool lnk_row_before(const double* pos, long long j, long long i) {
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    const double q = pos[j * ND + d], p = pos[i * ND + d];
    if (q != p) return q < p;
  }
  return j < i;
}

template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void link_rank_kernel(LinkArgs a) {
  const long long stride = (long long)gridDim.x * LNK_THREADS;
  for (long long i = (long long)blockIdx.x * LNK_THREADS + threadIdx.x; i < a.n; i += stride) {
    const int src = a.link[i];
    a.anc[i] = src < 0 ? (int)i : src;
    if (src >= 0) continue;
    const int t = lnk_level_of(a.off, a.n_levels, i);
    const long long d0 = a.off[t], d1 = a.off[t + 1];
    int rank = 0;
    if (t == 0) {
      rank = (int)(i - d0);        // level 0 counts its rows (find_link.py:620-623)
    } else {
      for (long long j = d0; j < d1; ++j)
        if (a.link[j] < 0 && j != i) rank += lnk_row_before<ND>(a.pos, j, i) ? 1 : 0;
    }
    a.rank[i] = rank;
    atomicAdd(&a.nbirth[t], 1);
  }
}

// one workgroup: base[t] = births of the levels before t; base[n_levels] = number of tracks
__global__ __launch_bounds__(LNK_THREADS) void link_scan_kernel(LinkArgs a) {
  const long long n = workgroup_scan_n<LNK_THREADS, long long>(
      a.n_levels, [&](long long t) { return a.nbirth[t]; }, [&](long long t, long long before) { a.base[t] = before; });
  if (threadIdx.x == 0) {
    a.base[a.n_levels] = n;
    *a.n_tracks = n;
  }
}

// anc[i] is always an ancestor of i (or i, a root): a value read while another lane replaces it
// is an ancestor too, so the rounds need no second buffer
__global__ __launch_bounds__(LNK_THREADS) void link_jump_kernel(LinkArgs a) {
  const long long stride = (long long)gridDim.x * LNK_THREADS;
  for (long long i = (long long)blockIdx.x * LNK_THREADS + threadIdx.x; i < a.n; i += stride) {
    const int p = ld_agent(&a.anc[i]);
    const int q = ld_agent(&a.anc[p]);
    if (q != p) st_agent(&a.anc[i], q);
  }
}

__global__ __launch_bounds__(LNK_THREADS) void link_ids_kernel(LinkArgs a) {
  const long long stride = (long long)gridDim.x * LNK_THREADS;
  for (long long i = (long long)blockIdx.x * LNK_THREADS + threadIdx.x; i < a.n; i += stride) {
    const int root = a.anc[i];
    a.particle[i] = a.base[lnk_level_of(a.off, a.n_levels, root)] + a.rank[root];
  }
}

// ---- host: the scratch of a call
// lays the scratch arrays of LinkArgs out from `base` (nullptr: only the size is wanted; else the
// bytes at the front that every call zeroes); ad: the adaptive linker's scratch too
// Prediction (include/ctrefine.h: ctr_link_predict): what the kernels of link_predict_kernels.h take
// besides LinkArgs.
struct LinkPredictArgs {
  int predictor;    // CTR_LINK_PREDICT_*
  double v0[3];
  double* w;        // [N, ndim] the velocity of every row: the caller's array, or scratch
  // scratch of the handle
  double* w_own;    // [N, ndim] w when the caller passes no array
  double* ppos;     // [N, ndim] the predicted scaled position of a row as a source of the current level
  double* u;        // [n_levels, ndim] the drift of every level (CTR_LINK_PREDICT_DRIFT)
};

inline size_t lnk_layout(LinkArgs& a, char* base, long long n, int ndim, long long n_levels,
                         LinkAdaptiveArgs* ad = nullptr, LinkPredictArgs* pr = nullptr) {
  size_t at = 0;
  const size_t N = (size_t)(n > 0 ? n : 1), L = (size_t)n_levels + 1;
  // the words that every call zeroes come first, in one block
  a.used = (int*)(base + carve(at, N * sizeof(int)));
  a.nbirth = (int*)(base + carve(at, L * sizeof(int)));
  if (ad) ad->over = (int*)(base + carve(at, N * sizeof(int)));
  const size_t zeroed = at;
  a.spos = (double*)(base + carve(at, N * ndim * sizeof(double)));
  a.cand_d2 = (double*)(base + carve(at, N * LNK_MAXC * sizeof(double)));
  a.cand_row = (int*)(base + carve(at, N * LNK_MAXC * sizeof(int)));
  int** per_row[] = {&a.ncand, &a.link, &a.lab_d, &a.lab_s, &a.cnt_s, &a.head_d, &a.head_s,
                     &a.next_d, &a.next_s, &a.roots, &a.rank, &a.anc};
  for (int** p : per_row) *p = (int*)(base + carve(at, N * sizeof(int)));
  a.base = (long long*)(base + carve(at, L * sizeof(long long)));
  if (ad) ad->nc_k = (int*)(base + carve(at, N * sizeof(int)));
  if (pr) {
    pr->w_own = (double*)(base + carve(at, N * ndim * sizeof(double)));
    pr->ppos = (double*)(base + carve(at, N * ndim * sizeof(double)));
    pr->u = (double*)(base + carve(at, L * ndim * sizeof(double)));
  }
  if (!base) return at;
  return zeroed;
}

#endif  // CTREFINE_LINK_KERNELS_H
