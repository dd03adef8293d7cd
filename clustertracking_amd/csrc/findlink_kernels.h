// findlink_kernels.h -- find and link with relocation (include/ctrefine.h: ctr_find_link_device;
// DESIGN.md 7b): the loop of the reference's FindLinker.assign_links (find_link.py:869-911) with
// Subnets.merge_lost_subnets (:329-370) around the linker's kernels (link_kernels.h) and the
// relocation kernel (relocate_kernels.h, through ctr_relocate_launch).  Included by tu_findlink.hip
// inside its anonymous namespace, after device_common.h and link_kernels.h.
//
// The table.  The host knows how many rows every frame was located with (n_loc[t]) but not how many
// relocated rows a level will claim, so level t owns rows [start[t], start[t] + n_loc[t] + R) of a
// padded table, start[t] = loc_off[t] + t R: its located rows, then up to R claimed ones.  A row
// nobody has claimed has a NaN position -- no distance test takes it as a source or a destination
// -- and links to itself, so it is neither a birth.  The linker's kernels run on that table
// unchanged (LinkArgs.off = start): candidates, births, ids, memory (`used`).
//
// Per level t >= 1, four launches on one stream, no word crosses to the host:
//   link_cand_kernel   candidates of the located rows of level t
//   fl_merge_kernel    one workgroup: sub-networks (lnk_components); a source without candidate is
//                      one of its own; shortage per sub-network; the 10 nearest sources within 2 of
//                      every source of a short one; union by min-propagation over those pairs; the
//                      sub-networks still short, in row order of their root, are the level's queries:
//                      source_offset, query_frame, source_pos
//   relocate_kernel    max_queries workgroups; one without sources ends at once with n_found = 0
//   fl_solve_kernel    one workgroup: 1 x 1 sub-networks link directly; one wavefront per other
//                      sub-network: cost block from the located destinations and the first `shortage`
//                      candidates of its query, lnk_hungarian; the claimed candidates are appended to
//                      the level in (query, mass) order; the coupled test
// then link_rank / link_scan / link_jump / link_ids over the grown table and fl_emit_kernel, which
// packs the live rows: located rows in their order, then the level's relocated rows in C order.
// Limits are reported through lnk_report into status[0..2], never by stopping: the levels after a
// failing one compute on, inside their bounds, and are not a result.
#ifndef CTREFINE_FINDLINK_KERNELS_H
#define CTREFINE_FINDLINK_KERNELS_H

struct FlArgs {
  LinkArgs l;             // the padded table as the linker sees it
  int n_levels, R, Q, K, nsz;
  long long ncap;
  double max_dist2;
  // located rows (the descriptor's)
  const long long* loc_off;
  const double* loc_pos;
  const double* loc_mass;
  const double* loc_signal;
  const double* loc_size;
  // padded table
  long long* start;       // [T + 1]
  int* cnt;               // [T] live rows of a level
  double* ppos;           // [ncap, ndim] (== l.pos)
  double* pmass;
  double* psignal;
  double* psize;          // [ncap, nsz]
  int* preloc;            // [ncap]
  int* pquery;            // [ncap] query a claimed row came from
  long long* pparticle;   // [ncap] (== l.particle)
  // merging, per row
  int* sn_ns;             // sources / destinations of a sub-network, by its root
  int* sn_nd;
  int* mrg;               // by root: root of the merged sub-network
  int* m_ns;              // by merged root
  int* m_nd;
  int* qof;               // by merged root: its query or -1
  int* nmnb;              // neighbours within 2 of a short source
  int* mnb;               // [ncap, 10]
  // the level's queries
  long long* q_soff;      // [Q + 1]
  long long* q_frame;     // [Q]
  double* q_spos;         // [Q * 30, ndim]
  int* q_root;            // [Q]
  int* q_short;           // [Q] shortage
  int* q_fill;            // [Q]
  int* n_q;               // [1]
  int* r_found;           // [Q] relocate's outputs
  int* r_pos;             // [Q, K, ndim]
  double* r_mass;
  double* r_signal;
  double* r_size;
  int* r_status;
  int* claim;             // [Q, K] source row that claimed the candidate or -1
  // outputs
  double* o_pos;
  long long* o_off;
  long long* o_particle;
  double* o_mass;
  double* o_signal;
  double* o_size;
  unsigned char* o_reloc;
  int* coupled;           // [T]
};

enum { FL_OVERSIZE = 1, FL_CAPACITY = 2, FL_RELOCATE = 3, FL_QUERIES = 4, FL_ROWS = 5 };

__device__ __forceinline__ double fl_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// one workgroup
__global__ __launch_bounds__(LNK_THREADS) void fl_start_kernel(FlArgs a) {
  for (int t = threadIdx.x; t <= a.n_levels; t += LNK_THREADS) {
    a.start[t] = a.loc_off[t] + (long long)t * a.R;
    if (t < a.n_levels) a.cnt[t] = (int)(a.loc_off[t + 1] - a.loc_off[t]);
  }
}

template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void fl_fill_kernel(FlArgs a) {
  const long long stride = (long long)gridDim.x * LNK_THREADS;
  for (long long i = (long long)blockIdx.x * LNK_THREADS + threadIdx.x; i < a.ncap; i += stride) {
    const int t = lnk_level_of(a.start, a.n_levels, i);
    const long long local = i - a.start[t], j = a.loc_off[t] + local;
    const bool live = local < a.loc_off[t + 1] - a.loc_off[t];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const double p = live ? a.loc_pos[j * ND + d] : fl_nan();
      a.ppos[i * ND + d] = p;
      a.l.spos[i * ND + d] = p / a.l.sr[d];
    }
    a.pmass[i] = live ? a.loc_mass[j] : fl_nan();
    a.psignal[i] = live ? a.loc_signal[j] : fl_nan();
    for (int d = 0; d < a.nsz; ++d) a.psize[i * a.nsz + d] = live ? a.loc_size[j * a.nsz + d] : fl_nan();
    a.preloc[i] = 0;
    a.pquery[i] = -1;
    a.l.link[i] = live ? -1 : (int)i;
  }
}

// a row of the source window that is a source of this level
template <int ND>
__device__ __forceinline__ bool fl_live(const LinkArgs& l, long long s) {
  return !(l.memory > 0 && l.used[s]) && l.spos[s * ND] == l.spos[s * ND];
}

__device__ __forceinline__ int fl_root(const LinkArgs& l, long long s) {
  const int lab = ld_agent(&l.lab_s[s]);
  return lab != LNK_NONE ? lab : (int)s;
}

struct FlLevel {
  long long d0, dl, w0, w1;   // located destinations [d0, dl), source window [w0, w1)
};

__device__ __forceinline__ FlLevel fl_level(const FlArgs& a, int t) {
  FlLevel v;
  v.d0 = a.l.off[t];
  v.dl = v.d0 + (a.loc_off[t + 1] - a.loc_off[t]);
  const long long tw = (long long)t - 1 - a.l.memory;
  v.w0 = a.l.off[tw > 0 ? tw : 0];
  v.w1 = v.d0;
  return v;
}

// One workgroup: the queries of level t.
template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void fl_merge_kernel(FlArgs a, int t) {
  __shared__ int s_changed, s_total;
  __shared__ int s_wcount[LNK_WAVES];
  const LinkArgs& l = a.l;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const FlLevel v = fl_level(a, t);

  lnk_components(l, v.d0, v.dl, v.w0, v.w1, tid, &s_changed);
  for (long long r = v.w0 + tid; r < v.dl; r += LNK_THREADS) {
    st_agent(&a.sn_ns[r], 0);
    st_agent(&a.sn_nd[r], 0);
    st_agent(&a.mrg[r], (int)r);
    st_agent(&a.m_ns[r], 0);
    st_agent(&a.m_nd[r], 0);
    a.qof[r] = -1;
  }
  if (tid == 0) s_total = 0;
  __syncthreads();

  // ---- sources and destinations per sub-network
  for (long long s = v.w0 + tid; s < v.w1; s += LNK_THREADS)
    if (fl_live<ND>(l, s)) atomicAdd(&a.sn_ns[fl_root(l, s)], 1);
  for (long long i = v.d0 + tid; i < v.dl; i += LNK_THREADS)
    if (l.ncand[i] > 0) atomicAdd(&a.sn_nd[ld_agent(&l.lab_d[i])], 1);
  __syncthreads();

  // ---- the 10 nearest sources within 2 of every source of a short sub-network (itself included)
  const double bound = (2. + 1e-7) * (2. + 1e-7);
  for (long long s = v.w0 + tid; s < v.w1; s += LNK_THREADS) {
    int n = 0;
    if (fl_live<ND>(l, s)) {
      const int root = fl_root(l, s);
      if (ld_agent(&a.sn_ns[root]) - ld_agent(&a.sn_nd[root]) > 0) {
        double pd[ND], bd[LNK_MAXC];
        int br[LNK_MAXC];
#pragma unroll
        for (int d = 0; d < ND; ++d) pd[d] = l.spos[s * ND + d];
#pragma unroll
        for (int k = 0; k < LNK_MAXC; ++k) { bd[k] = INFINITY; br[k] = LNK_NONE; }
        for (long long o = v.w0; o < v.w1; ++o) {
          if (l.memory > 0 && l.used[o]) continue;
          double d2 = 0.;
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            const double df = pd[d] - l.spos[o * ND + d];
            d2 += df * df;
          }
          if (!(d2 <= bound)) continue;     // (a row nobody claimed: NaN)
          double cd = d2;
          int cr = (int)o;
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
#pragma unroll
        for (int k = 0; k < LNK_MAXC; ++k) {
          a.mnb[s * LNK_MAXC + k] = br[k];
          n += br[k] != LNK_NONE;
        }
      }
    }
    a.nmnb[s] = n;
  }
  __syncthreads();

  // ---- union: every pair pulls both sub-networks to the smaller root until a pass changes nothing
  for (;;) {
    if (tid == 0) s_changed = 0;
    __syncthreads();
    bool changed = false;
    for (long long s = v.w0 + tid; s < v.w1; s += LNK_THREADS) {
      const int n = a.nmnb[s];
      if (n == 0) continue;
      const int rs = fl_root(l, s);
      int m = ld_agent(&a.mrg[rs]);
      for (int k = 0; k < n; ++k) {
        const int o = ld_agent(&a.mrg[fl_root(l, a.mnb[s * LNK_MAXC + k])]);
        m = o < m ? o : m;
      }
      if (atomicMin(&a.mrg[rs], m) > m) changed = true;
      for (int k = 0; k < n; ++k)
        if (atomicMin(&a.mrg[fl_root(l, a.mnb[s * LNK_MAXC + k])], m) > m) changed = true;
    }
    if (changed) s_changed = 1;
    __syncthreads();
    const int again = s_changed;
    __syncthreads();
    if (!again) break;
  }
  // (at rest both ends of every pair hold the same root, the smallest of their union)

  // ---- sources and destinations per merged sub-network
  for (long long s = v.w0 + tid; s < v.w1; s += LNK_THREADS)
    if (fl_live<ND>(l, s)) atomicAdd(&a.m_ns[ld_agent(&a.mrg[fl_root(l, s)])], 1);
  for (long long i = v.d0 + tid; i < v.dl; i += LNK_THREADS)
    if (l.ncand[i] > 0) atomicAdd(&a.m_nd[ld_agent(&a.mrg[ld_agent(&l.lab_d[i])])], 1);
  __syncthreads();

  // ---- the short ones, in row order of their root, are the queries
  for (long long base = v.w0; base < v.dl; base += LNK_THREADS) {
    const long long r = base + tid;
    int ns = 0, nd = 0;
    bool is = false;
    if (r < v.dl) {
      ns = ld_agent(&a.m_ns[r]);
      nd = ld_agent(&a.m_nd[r]);
      is = ns - nd > 0;
    }
    const unsigned long long bal = __ballot(is);
    if (lane == 0) s_wcount[wave] = __popcll(bal);
    __syncthreads();
    int before = s_total, total = 0;
    for (int w = 0; w < LNK_WAVES; ++w) { if (w < wave) before += s_wcount[w]; total += s_wcount[w]; }
    const int q = before + __popcll(bal & ((1ull << lane) - 1ull));
    if (is && q < a.Q) {
      a.q_root[q] = (int)r;
      a.q_short[q] = ns - nd;
      a.qof[r] = q;
      if (ns > LNK_MAX_SRC) lnk_report(l.status, FL_OVERSIZE, t, ns);
    }
    __syncthreads();
    if (tid == 0) s_total += total;
    __syncthreads();
  }
  if (tid == 0) {
    const int total = s_total;
    if (total > a.Q) lnk_report(l.status, FL_QUERIES, t, total);
    const int nq = total < a.Q ? total : a.Q;
    a.n_q[0] = nq;
    long long at = 0;
    a.q_soff[0] = 0;
    for (int q = 0; q < a.Q; ++q) {
      if (q < nq) {
        const int ns = ld_agent(&a.m_ns[a.q_root[q]]);
        at += ns <= LNK_MAX_SRC ? ns : 0;      // an oversize one asks nothing
      }
      a.q_soff[q + 1] = at;
      a.q_frame[q] = t;
      a.q_fill[q] = 0;
    }
  }
  __syncthreads();
  for (long long s = v.w0 + tid; s < v.w1; s += LNK_THREADS) {
    if (!fl_live<ND>(l, s)) continue;
    const int mr = ld_agent(&a.mrg[fl_root(l, s)]);
    const int q = a.qof[mr];
    if (q < 0 || ld_agent(&a.m_ns[mr]) > LNK_MAX_SRC) continue;
    const long long slot = a.q_soff[q] + atomicAdd(&a.q_fill[q], 1);
#pragma unroll
    for (int d = 0; d < ND; ++d) a.q_spos[slot * ND + d] = l.pos[s * ND + d];
  }
}

// One workgroup: the links of level t, its claimed rows, the coupled flag.
template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void fl_solve_kernel(FlArgs a, int t) {
  __shared__ double s_cost[LNK_WAVES][LNK_MAX_SRC * LNK_MAX_DST];
  __shared__ double s_u[LNK_WAVES][LNK_MAX_SRC + 2];
  __shared__ int s_src[LNK_WAVES][LNK_MAX_SRC];
  __shared__ int s_dst[LNK_WAVES][LNK_MAX_DST];
  __shared__ unsigned char s_p[LNK_WAVES][LNK_MAX_SRC + LNK_MAX_DST + 2];
  __shared__ unsigned char s_way[LNK_WAVES][LNK_MAX_SRC + LNK_MAX_DST + 2];
  __shared__ int s_nroots, s_nclaimed;

  const LinkArgs& l = a.l;
  const int tid = threadIdx.x;
  const FlLevel v = fl_level(a, t);
  const int nq = a.n_q[0];

  for (long long r = v.w0 + tid; r < v.dl; r += LNK_THREADS) {
    st_agent(&l.head_d[r], -1);
    st_agent(&l.head_s[r], -1);
  }
  for (int c = tid; c < a.Q * a.K; c += LNK_THREADS) a.claim[c] = -1;
  if (tid == 0) { s_nroots = 0; s_nclaimed = 0; }
  __syncthreads();

  // ---- 1 x 1 sub-networks link here; the members of the others are chained to their root
  for (long long i = v.d0 + tid; i < v.dl; i += LNK_THREADS) {
    if (l.ncand[i] == 0) continue;
    const int mr = ld_agent(&a.mrg[ld_agent(&l.lab_d[i])]);
    if (ld_agent(&a.m_ns[mr]) == 1 && ld_agent(&a.m_nd[mr]) == 1) {
      const int c = l.cand_row[i * LNK_MAXC];
      l.link[i] = c;
      if (l.memory > 0) l.used[c] = 1;
      continue;
    }
    st_agent(&l.next_d[i], atomicExch(&l.head_d[mr], (int)i));
  }
  for (long long s = v.w0 + tid; s < v.w1; s += LNK_THREADS) {
    if (!fl_live<ND>(l, s)) continue;
    const int mr = ld_agent(&a.mrg[fl_root(l, s)]);
    const int ns = ld_agent(&a.m_ns[mr]), nd = ld_agent(&a.m_nd[mr]);
    if (ns == 1 && nd == 1) continue;
    st_agent(&l.next_s[s], atomicExch(&l.head_s[mr], (int)s));
  }
  for (long long r = v.w0 + tid; r < v.dl; r += LNK_THREADS) {
    const int ns = ld_agent(&a.m_ns[r]), nd = ld_agent(&a.m_nd[r]);
    if (ns < 1 || (ns == 1 && nd == 1)) continue;
    if (nd < 1 && a.qof[r] < 0) continue;      // short, but beyond the level's queries: lost
    st_agent(&l.roots[v.w0 + atomicAdd(&s_nroots, 1)], (int)r);
  }
  __syncthreads();

  // ---- one wavefront per other sub-network
  const int w = tid >> 6, lane = tid & 63;
  const int nroots = s_nroots;
  const double bound = (1. + 1e-7) * (1. + 1e-7);
  for (int ri = w; ri < nroots; ri += LNK_WAVES) {
    const int root = ld_agent(&l.roots[v.w0 + ri]);
    int ns = 0, nd = 0;
    if (lane == 0) {   // members in ascending row order, whatever order they were chained in
      for (int j = ld_agent(&l.head_s[root]); j >= 0; j = ld_agent(&l.next_s[j])) {
        if (ns < LNK_MAX_SRC) {
          int q = ns;
          for (; q > 0 && s_src[w][q - 1] > j; --q) s_src[w][q] = s_src[w][q - 1];
          s_src[w][q] = j;
        }
        ++ns;
      }
      for (int j = ld_agent(&l.head_d[root]); j >= 0; j = ld_agent(&l.next_d[j])) {
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
    if (ns > LNK_MAX_SRC) { if (lane == 0) lnk_report(l.status, FL_OVERSIZE, t, ns); continue; }
    const int q = a.qof[root];
    int nc = 0;       // candidates of its query that join the destinations
    if (q >= 0) {
      if (a.r_status[q] != 0) { if (lane == 0) lnk_report(l.status, FL_RELOCATE, t, a.r_status[q]); continue; }
      nc = a.q_short[q] < a.r_found[q] ? a.q_short[q] : a.r_found[q];
      nc = nc < a.K ? nc : a.K;
    }
    if (nd + nc > LNK_MAX_DST) { if (lane == 0) lnk_report(l.status, FL_CAPACITY, t, nd + nc); continue; }
    lnk_wave_sync();
    for (int c = lane; c < ns * LNK_MAX_DST; c += 64) s_cost[w][c] = LNK_BIG;
    const int m = nd + nc + ns;
    for (int c = lane; c <= m; c += 64) { s_p[w][c] = 0; s_way[w][c] = 0; }
    if (lane <= ns) s_u[w][lane] = 0.;
    lnk_wave_sync();
    if (lane < nd) {
      const long long i = s_dst[w][lane];
      const int n = l.ncand[i];
      for (int k = 0; k < n; ++k) {
        const int c = l.cand_row[i * LNK_MAXC + k];
        int sl = 0;
        while (sl < ns && s_src[w][sl] != c) ++sl;
        if (sl < ns) s_cost[w][sl * LNK_MAX_DST + lane] = l.cand_d2[i * LNK_MAXC + k] - 2.;
      }
    } else if (lane < nd + nc) {
      // a relocated candidate is a link candidate of every source of the sub-network within 1
      const size_t row = (size_t)q * a.K + (lane - nd);
      double pc[ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) pc[d] = (double)a.r_pos[row * ND + d] / l.sr[d];
      for (int sl = 0; sl < ns; ++sl) {
        const long long s = s_src[w][sl];
        double d2 = 0.;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          const double df = pc[d] - l.spos[s * ND + d];
          d2 += df * df;
        }
        if (d2 <= bound) s_cost[w][sl * LNK_MAX_DST + lane] = d2 - 2.;
      }
    }
    lnk_wave_sync();

    lnk_hungarian(s_cost[w], s_u[w], s_p[w], s_way[w], ns, nd + nc, lane);
    if (lane < nd + nc) {
      const int r = s_p[w][lane + 1];
      if (r && s_cost[w][(r - 1) * LNK_MAX_DST + lane] < 0.5 * LNK_BIG) {
        const int src = s_src[w][r - 1];
        if (lane < nd) l.link[s_dst[w][lane]] = src;
        else a.claim[(size_t)q * a.K + (lane - nd)] = src;
        if (l.memory > 0) l.used[src] = 1;
      }
    }
    lnk_wave_sync();
  }
  __syncthreads();

  // ---- the claimed candidates become rows of the level, in (query, mass) order
  if (tid == 0) {
    const int n_loc = (int)(v.dl - v.d0);
    int n = 0, over = 0;
    for (int q = 0; q < nq; ++q) {
      int nc = a.q_short[q] < a.r_found[q] ? a.q_short[q] : a.r_found[q];
      nc = nc < a.K ? nc : a.K;
      for (int j = 0; j < nc; ++j) {
        const size_t c = (size_t)q * a.K + j;
        const int src = a.claim[c];
        if (src < 0) continue;
        if (n >= a.R) { ++over; continue; }
        const long long row = v.dl + n;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          const double p = (double)a.r_pos[c * ND + d];
          a.ppos[row * ND + d] = p;
          l.spos[row * ND + d] = p / l.sr[d];
        }
        a.pmass[row] = a.r_mass[c];
        a.psignal[row] = a.r_signal[c];
        for (int d = 0; d < a.nsz; ++d) a.psize[row * a.nsz + d] = a.r_size[c * a.nsz + d];
        a.preloc[row] = 1;
        a.pquery[row] = q;
        l.link[row] = src;
        ++n;
      }
    }
    if (over) lnk_report(l.status, FL_ROWS, t, n + over);
    a.cnt[t] = n_loc + n;
    s_nclaimed = n;
  }
  __syncthreads();

  // ---- coupled: a claimed candidate within max_dist of a source of another query
  const int n_claimed = s_nclaimed;
  if (n_claimed > 0 && nq > 1) {
    const long long n_slots = a.q_soff[nq];
    bool hit = false;
    for (long long sl = tid; sl < n_slots && !hit; sl += LNK_THREADS) {
      int q = 0;
      while (q + 1 < nq && a.q_soff[q + 1] <= sl) ++q;
      double sq[ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) sq[d] = a.q_spos[sl * ND + d] / l.sr[d];
      for (int k = 0; k < n_claimed && !hit; ++k) {
        const long long row = v.dl + k;
        if (a.pquery[row] == q) continue;
        double d2 = 0.;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          const double df = l.spos[row * ND + d] - sq[d];
          d2 += df * df;
        }
        hit = d2 <= a.max_dist2;
      }
    }
    if (hit) a.coupled[t] = 1;     // (every writer writes the same word)
  }
}

// With the refinement, behind link_rank_kernel: that kernel ranks the births of a level by the
// table's positions, which are the refined ones by then, but a level is linked before it is refined
// and its births are numbered where they were located.  A birth is always a located row, and its
// whole-pixel position is still in the descriptor's table: the rank among the births of its level by
// those.  (Two births of one pixel row whose refined positions come in the other order did swap ids.)
template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void fl_birth_rank_kernel(FlArgs a) {
  const long long stride = (long long)gridDim.x * LNK_THREADS;
  for (long long i = (long long)blockIdx.x * LNK_THREADS + threadIdx.x; i < a.ncap; i += stride) {
    if (a.l.link[i] >= 0) continue;
    const int t = lnk_level_of(a.start, a.n_levels, i);
    const long long s0 = a.start[t], l0 = a.loc_off[t], n_loc = a.loc_off[t + 1] - l0, local = i - s0;
    if (t == 0 || local >= n_loc) continue;      // level 0 counts its rows
    int rank = 0;
    for (long long j = 0; j < n_loc; ++j)
      if (j != local && a.l.link[s0 + j] < 0) rank += lnk_row_before<ND>(a.loc_pos, l0 + j, l0 + local) ? 1 : 0;
    a.l.rank[i] = rank;
  }
}

// one workgroup: o_off[t] = live rows of the levels before t
__global__ __launch_bounds__(LNK_THREADS) void fl_offsets_kernel(FlArgs a) {
  const long long n = workgroup_scan_n<LNK_THREADS, long long>(
      a.n_levels, [&](long long t) { return a.cnt[t]; }, [&](long long t, long long before) { a.o_off[t] = before; });
  if (threadIdx.x == 0) a.o_off[a.n_levels] = n;
}

template <int ND>
__global__ __launch_bounds__(LNK_THREADS) void fl_emit_kernel(FlArgs a) {
  const long long stride = (long long)gridDim.x * LNK_THREADS;
  for (long long i = (long long)blockIdx.x * LNK_THREADS + threadIdx.x; i < a.ncap; i += stride) {
    const int t = lnk_level_of(a.start, a.n_levels, i);
    const long long s0 = a.start[t], local = i - s0;
    if (local >= a.cnt[t]) continue;
    const long long n_loc = a.loc_off[t + 1] - a.loc_off[t];
    long long out = a.o_off[t] + local;
    if (local >= n_loc) {       // a relocated row: its rank in C order among those of the level
      int rank = 0;
      for (long long j = s0 + n_loc; j < s0 + a.cnt[t]; ++j)
        if (j != i) rank += lnk_row_before<ND>(a.ppos, j, i) ? 1 : 0;
      out = a.o_off[t] + n_loc + rank;
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) a.o_pos[out * ND + d] = a.ppos[i * ND + d];
    a.o_particle[out] = a.pparticle[i];
    a.o_mass[out] = a.pmass[i];
    a.o_signal[out] = a.psignal[i];
    for (int d = 0; d < a.nsz; ++d) a.o_size[out * a.nsz + d] = a.psize[i * a.nsz + d];
    a.o_reloc[out] = (unsigned char)a.preloc[i];
  }
}

#endif  // CTREFINE_FINDLINK_KERNELS_H
