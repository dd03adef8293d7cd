// twopoint_kernels.h -- two-point displacement correlations of linked particles: for every lag the
// mean over the pairs of a frame, binned by their distance, of the products of their displacements
// (ctr_twopoint_device; include/ctrefine.h has the rule).  Included by tu_twopoint.hip
// inside its anonymous namespace, after stage_common.h, pair_walk.h (the table, the work items and
// the walk over a frame's rows) and particle_match.h (the LDS table particle -> row of drift); here
// are the partner of a row, its displacement, the payload of a candidate tile, the fixed-point sums
// of a pair, their flush into 128-bit words, and the means.  The kernel boundary is the only
// synchronisation between workgroups; every loop is bounded by the launch's arguments or by row
// ranges of a frame_offset that twopt_check_kernel has passed.  Integer atomics only (LDS and the
// int64 words, where the order cannot matter); there is no sum of doubles at all.
#ifndef CTREFINE_TWOPOINT_KERNELS_H
#define CTREFINE_TWOPOINT_KERNELS_H

constexpr int TP_THREADS = PAIR_THREADS;         // a workgroup of every kernel here: 4 wavefronts
constexpr int TP_TILE = PAIR_TILE;               // rows of a work item, and candidates staged at a time
constexpr int TP_MAX_BINS = CTR_TP_MAX_BINS;     // edge2, the counts and the sums of a workgroup are in LDS
constexpr int TP_MAX_LAGS = CTR_TP_MAX_LAGS;
constexpr int TP_SUMS = 3;                       // dot, L, c
constexpr int TP_FLUSH_TILES = 32;               // 2^41 per pair * 2^16 pairs per tile * 32 = 2^62 in an int64 of LDS
constexpr int TP_ROWS = 8;                       // rows of frame t per thread and chunk of twopt_partner_kernel

static_assert(CTR_TP_OK == 0, "status[0] == 0: the table of a pair stage was not refused");
static_assert((TP_TILE & (TP_TILE - 1)) == 0, "a candidate's place in its tile is a mask");

struct TwoptArgs {
  PairTable tab;
  int K;
  long long B, P;
  long long lag[TP_MAX_LAGS];
  double dr, max2;
  double unit, inv_unit;      // 2^(e - 40) and its inverse: clause 8
  const long long* particle;
  const double* edge2;        // [B + 1]
  // scratch
  int* partner;               // [K, N]: the partner's row of a row that has moved, else -1
  // out
  long long* n;               // [K, B]
  double* dot;
  double* longitudinal;
  double* transverse;
  double* cosine;
  long long* sums;            // [K, B, TP_SUMS, 2]: hi, lo
  long long* n_moved;
  long long* beyond;
};

// clause 11: the offsets (pair_check) and particle < P, before any kernel follows either.
// status[0] was zeroed in front of the kernel.
__global__ void __launch_bounds__(TP_THREADS) twopt_check_kernel(const TwoptArgs a) {
  pair_check(a.tab, CTR_TP_BAD_TABLE);
  const long long stride = (long long)gridDim.x * TP_THREADS;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * TP_THREADS + threadIdx.x; i < a.tab.N; i += stride) bad |= a.particle[i] >= a.P;
  if (bad) st_agent(a.tab.status, CTR_TP_BAD_TABLE);
}

// the integer outputs zeroed, whatever the status: a refused table leaves them so
__global__ void __launch_bounds__(TP_THREADS) twopt_defaults_kernel(const TwoptArgs a) {
  const long long stride = (long long)gridDim.x * TP_THREADS;
  const long long cells = (long long)a.K * a.B, words = cells * TP_SUMS * 2;
  for (long long e = (long long)blockIdx.x * TP_THREADS + threadIdx.x; e < words; e += stride) {
    a.sums[e] = 0;
    if (e < cells) a.n[e] = 0;
    if (e < a.K) { a.n_moved[e] = 0; a.beyond[e] = 0; }
  }
}

// clause 5 for row i and its partner j: u, u2, and whether the row has moved or lies beyond
struct TwoptMove {
  double u[CTR_MAX_NDIM];
  double u2;
  bool moved, beyond;
};

__device__ __forceinline__ TwoptMove twopt_move(const TwoptArgs& a, const PairRow& qi, const PairRow& qj) {
  TwoptMove o;
  bool finite = true;
  o.u2 = 0.;
#pragma unroll
  for (int d = 0; d < CTR_MAX_NDIM; ++d) {
    o.u[d] = 0.;
    if (d < a.tab.ndim) {
      const double u = qj.q[d] - qi.q[d];
      const double uu = u * u;                 // the unit is compiled without contraction
      o.u[d] = u;
      o.u2 = d == 0 ? uu : o.u2 + uu;
      finite = finite && fabs(u) < __builtin_inf();      // false for a NaN; a finite u: both rows exist
    }
  }
  o.moved = finite && o.u2 <= a.max2;
  o.beyond = finite && o.u2 > a.max2;
  return o;
}

// One workgroup per item (lag k, frame t), striding past the grid: partner[k, i] of every row i of
// frame t, n_moved[k] and beyond[k].  The rows of frame t + lag go through LDS in tiles of DR_TILE,
// in ascending row order, each an open-addressing table particle -> row (counted from the frame's
// first row) that keeps the lowest row of a repeated particle; a row of frame t without a match yet
// probes the tile, so the first tile that answers gives the lowest row of all: the matching of
// drift_pairs_kernel.  A frame without a frame `lag` on has no partner.
__global__ void __launch_bounds__(TP_THREADS) twopt_partner_kernel(const TwoptArgs a) {
  __shared__ unsigned long long s_tab[DR_SLOTS];
  __shared__ int s_cnt[2];
  if (!pair_ok(a.tab)) return;
  const int tid = threadIdx.x;
  const long long items = (long long)a.K * a.tab.T;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int k = (int)(it / a.tab.T);
    const long long t = it % a.tab.T, tc = t + a.lag[k];          // no overflow: T and the lags are below 2^31
    const long long r0 = a.tab.frame_offset[t], r1 = a.tab.frame_offset[t + 1];
    const long long q0 = tc < a.tab.T ? a.tab.frame_offset[tc] : 0, q1 = tc < a.tab.T ? a.tab.frame_offset[tc + 1] : 0;
    int* partner = a.partner + (long long)k * a.tab.N;
    __syncthreads();                           // the counters of the item before are read
    if (tid < 2) s_cnt[tid] = 0;
    int moved = 0, beyond = 0;
    for (long long base = r0; base < r1; base += TP_THREADS * TP_ROWS) {
      int pk[TP_ROWS], jrel[TP_ROWS];
#pragma unroll
      for (int m = 0; m < TP_ROWS; ++m) {
        const long long i = base + m * TP_THREADS + tid;
        const long long p = i < r1 ? a.particle[i] : -1;
        pk[m] = p < 0 ? -1 : (int)p;           // p < P <= 2^31 - 2 (twopt_check_kernel)
        jrel[m] = -1;
      }
      for (long long tb = q0; tb < q1; tb += DR_TILE) {
        __syncthreads();                       // the lookups of the tile before are done
        for (int s = tid; s < DR_SLOTS; s += TP_THREADS) s_tab[s] = DR_EMPTY;
        __syncthreads();
        const int n = q1 - tb < DR_TILE ? (int)(q1 - tb) : DR_TILE;
        for (int q = tid; q < n; q += TP_THREADS) {
          const long long p = a.particle[tb + q];
          if (p >= 0) drift_insert(s_tab, (int)p, (unsigned)(tb - q0 + q));
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < TP_ROWS; ++m)
          if (pk[m] >= 0 && jrel[m] < 0) jrel[m] = drift_lookup(s_tab, pk[m]);
      }
#pragma unroll
      for (int m = 0; m < TP_ROWS; ++m) {
        const long long i = base + m * TP_THREADS + tid;
        if (i >= r1) continue;
        int row = -1;
        if (jrel[m] >= 0) {
          const long long j = q0 + jrel[m];
          const TwoptMove mv = twopt_move(a, pair_row(a.tab, i), pair_row(a.tab, j));
          if (mv.moved) { row = (int)j; ++moved; }       // N <= 2^31 - 1
          if (mv.beyond) ++beyond;
        }
        partner[i] = row;
      }
    }
    __syncthreads();                           // the counters are zero
    if (moved) atomicAdd(&s_cnt[0], moved);    // at most N < 2^31
    if (beyond) atomicAdd(&s_cnt[1], beyond);
    __syncthreads();
    if (tid == 0 && s_cnt[0]) atomicAdd((unsigned long long*)(a.n_moved + k), (unsigned long long)s_cnt[0]);
    if (tid == 1 && s_cnt[1]) atomicAdd((unsigned long long*)(a.beyond + k), (unsigned long long)s_cnt[1]);
  }
}

__global__ void __launch_bounds__(TP_THREADS) twopt_items_kernel(const TwoptArgs a) { pair_items(a.tab); }

// the displacements of a tile of candidate rows in LDS, beside their positions in PairTile: 8192 B
struct TwoptTile {
  double u[CTR_MAX_NDIM][TP_TILE];
  double u2[TP_TILE];
};

// clause 5 for row r of a frame at lag k from partner[]: its position, its displacement, and
// .exists: whether it has moved.  What twopt_partner_kernel computed, from the same operations.
struct TwoptRow : PairRow {
  double u[CTR_MAX_NDIM];
  double u2;
};

__device__ __forceinline__ TwoptRow twopt_row(const TwoptArgs& a, const int* partner, long long r) {
  TwoptRow o = {pair_row(a.tab, r), {0., 0., 0.}, 0.};
  const int j = partner[r];
  o.exists = j >= 0;
  if (j >= 0) {
    const TwoptMove mv = twopt_move(a, o, pair_row(a.tab, j));
#pragma unroll
    for (int d = 0; d < CTR_MAX_NDIM; ++d) o.u[d] = mv.u[d];
    o.u2 = mv.u2;
  }
  return o;
}

// clause 8: x as the integer rint(x * inv_unit), ties to even; the scaling by a power of two is exact
__device__ __forceinline__ long long twopt_fixed(double x, double inv_unit) { return (long long)rint(x * inv_unit); }

// The counts and sums of the workgroup added to the words of lag k, and zeroed by the thread that
// read them.  A sum v enters the 128-bit (hi, lo) as: lo += v, returning the old lo; hi += the sign
// extension of v plus the carry, which is whether the new lo is below the old one (unsigned).
__device__ __forceinline__ void twopt_flush(const TwoptArgs& a, unsigned* s_hist, long long* s_acc, int k) {
  for (int b = threadIdx.x; b < a.B; b += TP_THREADS) {
    const unsigned c = s_hist[b];
    if (!c) continue;                          // no pair: the sums are zero
    const long long cell = (long long)k * a.B + b;
    atomicAdd((unsigned long long*)(a.n + cell), (unsigned long long)c);
    s_hist[b] = 0;
#pragma unroll
    for (int s = 0; s < TP_SUMS; ++s) {
      const long long v = s_acc[b * TP_SUMS + s];
      s_acc[b * TP_SUMS + s] = 0;
      if (v == 0) continue;
      unsigned long long* word = (unsigned long long*)(a.sums + (cell * TP_SUMS + s) * 2);
      const unsigned long long add = (unsigned long long)v;
      const unsigned long long old = atomicAdd(word + 1, add);
      const long long up = (v < 0 ? -1LL : 0LL) + (old + add < old ? 1LL : 0LL);
      if (up) atomicAdd(word, (unsigned long long)up);
    }
  }
}

// One workgroup per item (lag k, work item w of pair_walk), striding past the grid: frame t and a
// tile of TP_TILE of its rows, found in item_start; workgroups beyond the number of items leave.  A
// thread owns row i and keeps q_i, u_i and u2_i in registers; the candidates are the rows of its own
// frame, and one "exists" when it has moved (pair_walk: a row that has not is staged as NaN).  The
// row functor also stages u_j and u2_j of the candidate it loads into s_move; the pair callback reads
// them, and the differences R that d2 squared, by j's place in the tile.  Clause 7 per pair, then one
// 32-bit and three 64-bit LDS integer adds; the flush at the end of a work item and every
// TP_FLUSH_TILES candidate tiles.
__global__ void __launch_bounds__(TP_THREADS) twopt_pairs_kernel(const TwoptArgs a) {
  __shared__ double s_edge2[TP_MAX_BINS + 1];
  __shared__ unsigned s_hist[TP_MAX_BINS];
  __shared__ long long s_acc[TP_MAX_BINS * TP_SUMS];
  __shared__ PairTile s_tile;
  __shared__ TwoptTile s_move;
  if (!pair_ok(a.tab)) return;
  const long long total = a.tab.item_start[a.tab.T], items = (long long)a.K * total;
  if ((long long)blockIdx.x >= items) return;
  const int tid = threadIdx.x, B = (int)a.B, nd = a.tab.ndim;
  const double inv_dr = 1. / a.dr, inv_unit = a.inv_unit, inv_cos = 1099511627776.;       // 2^40
  for (int b = tid; b <= B; b += TP_THREADS) s_edge2[b] = a.edge2[b];
  for (int b = tid; b < B; b += TP_THREADS) s_hist[b] = 0;
  for (int b = tid; b < B * TP_SUMS; b += TP_THREADS) s_acc[b] = 0;
  const double e2_max = a.edge2[B];
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int k = (int)(it / total);
    const long long w = it % total;
    const long long t = pair_item_frame(a.tab, w);
    if (t + a.lag[k] >= a.tab.T) continue;     // no row of this frame has moved; the same for the whole workgroup
    const long long r0 = a.tab.frame_offset[t], r1 = a.tab.frame_offset[t + 1];
    const long long i = r0 + (w - a.tab.item_start[t]) * TP_TILE + tid;
    const int* partner = a.partner + (long long)k * a.tab.N;
    TwoptRow me = {};
    long long gi = -1;
    if (i < r1) {
      me = twopt_row(a, partner, i);
      if (a.tab.group) gi = a.tab.group[i];
    }
    long long tiles = 0;
    pair_walk(                                 // its first barrier: the counts and sums are zero
        a.tab, s_tile, r0, r1, me.exists, me.q, gi, i, e2_max,
        [&](long long j) {
          const TwoptRow r = twopt_row(a, partner, j);
#pragma unroll
          for (int d = 0; d < CTR_MAX_NDIM; ++d)
            if (d < nd) s_move.u[d][tid] = r.u[d];
          s_move.u2[tid] = r.u2;
          return r;
        },
        [&](long long j, double d2) {
          if (!(d2 > 0.)) return;              // coincident rows are not pairs
          const int jj = (int)(j - r0) & (TP_TILE - 1);
          double dot = 0., ai = 0., aj = 0.;
#pragma unroll
          for (int d = 0; d < CTR_MAX_NDIM; ++d)
            if (d < nd) {
              const double R = s_tile.q[d][jj] - me.q[d], uj = s_move.u[d][jj];
              const double p_dot = me.u[d] * uj, p_i = me.u[d] * R, p_j = uj * R;
              dot = d == 0 ? p_dot : dot + p_dot;
              ai = d == 0 ? p_i : ai + p_i;
              aj = d == 0 ? p_j : aj + p_j;
            }
          const double along = (ai * aj) / d2;
          const double uu = me.u2 * s_move.u2[jj];
          const double c = uu > 0. ? dot / sqrt(uu) : 0.;
          int b = (int)fmin(sqrt(d2) * inv_dr, (double)(B - 1));      // clause 7 of g(r): a guess, corrected against the edges
          while (b > 0 && d2 < s_edge2[b]) --b;
          while (d2 >= s_edge2[b + 1]) ++b;    // ends below B: d2 < edge2[B]
          atomicAdd(&s_hist[b], 1u);
          unsigned long long* acc = (unsigned long long*)(s_acc + b * TP_SUMS);
          atomicAdd(acc + 0, (unsigned long long)twopt_fixed(dot, inv_unit));
          atomicAdd(acc + 1, (unsigned long long)twopt_fixed(along, inv_unit));
          atomicAdd(acc + 2, (unsigned long long)twopt_fixed(c, inv_cos));
        },
        [&]() {
          if (++tiles % TP_FLUSH_TILES == 0) {
            __syncthreads();
            twopt_flush(a, s_hist, s_acc, k);
          }
        });
    __syncthreads();
    twopt_flush(a, s_hist, s_acc, k);
  }
}

// clause 10: the 128-bit (hi, lo) as a double
__device__ __forceinline__ double twopt_double(long long hi, long long lo) {
  if (hi == (lo >> 63)) return (double)lo;     // it fits int64: one rounding
  const double high = (double)hi * 18446744073709551616.;       // 2^64: exact scaling
  return high + (double)(unsigned long long)lo;
}

// One thread per (k, b): clause 10.  A refused table has n == 0 everywhere: NaN.
__global__ void __launch_bounds__(TP_THREADS) twopt_finish_kernel(const TwoptArgs a) {
  const long long stride = (long long)gridDim.x * TP_THREADS;
  const double nan = __builtin_nan(""), unit_cos = 1. / 1099511627776.;
  for (long long e = (long long)blockIdx.x * TP_THREADS + threadIdx.x; e < (long long)a.K * a.B; e += stride) {
    const long long n = a.n[e];
    double dot = nan, along = nan, across = nan, c = nan;
    if (n > 0) {
      const long long* w = a.sums + e * TP_SUMS * 2;
      const double count = (double)n;
      dot = (twopt_double(w[0], w[1]) * a.unit) / count;
      along = (twopt_double(w[2], w[3]) * a.unit) / count;
      c = (twopt_double(w[4], w[5]) * unit_cos) / count;
      const unsigned long long lo = (unsigned long long)w[1] - (unsigned long long)w[3];     // S_dot - S_L, 128 bits
      const long long hi = (long long)((unsigned long long)w[0] - (unsigned long long)w[2] - ((unsigned long long)w[1] < (unsigned long long)w[3] ? 1ull : 0ull));
      across = ((twopt_double(hi, (long long)lo) * a.unit) / count) / (double)(a.tab.ndim - 1);
    }
    a.dot[e] = dot;
    a.longitudinal[e] = along;
    a.transverse[e] = across;
    a.cosine[e] = c;
  }
}

#endif  // CTREFINE_TWOPOINT_KERNELS_H
