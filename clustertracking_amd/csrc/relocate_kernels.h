// relocate_kernels.h -- relocation candidates of lost features (include/ctrefine.h:
// ctr_relocate_device): the rule of the reference's
// FindLinker.get_relocate_candidates (find_link.py:811-867).  Included by tu_relocate.hip inside
// its anonymous namespace, after device_common.h (in_mask, ellipse_sum, scaled_dist2),
// locate_kernels.h (loc_above: the threshold comparison of ctr_locate) and characterize_kernels.h
// (the accumulators and the wavefront reduction of ctr_characterize).  No floating-point
// contraction anywhere in the unit: every ellipse and every distance rounds as NumPy's does.
//
// One workgroup takes one query, start to end:
//   sources -> LDS; lane 0 derives the box; the known features of the query's frame that lie
//   within max_dist of a source -> LDS (box coordinates);
//   the masked value m (0 where not visible, hidden or beyond the box) is staged into the LDS tile
//   in the pixel type, slab after slab along axis 0 -- a box that fits the tile is one slab, a
//   larger one is walked in slabs with the dilation box as halo; a box so wide that not even one
//   slab fits (dilation box x the other axes of the box > tile) is not staged: m is recomputed
//   from the frame in global memory for every pixel and every neighbour it is compared with;
//   maxima of the slab's own rows, compacted in C order by ballot and prefix into a list of
//   CTR_RELOCATE_MAX_MAXIMA entries;
//   reach and drop-close on the list; one wavefront per survivor characterises it on m (from the
//   tile when the box was one slab, else recomputed from the frame); rank by mass, write.
// Nothing is shared between workgroups and there is no floating-point atomic: a query gives the
// same bytes alone and in any batch.
#ifndef CTREFINE_RELOCATE_KERNELS_H
#define CTREFINE_RELOCATE_KERNELS_H

constexpr int RL_THREADS = 256;
constexpr int RL_WAVES = RL_THREADS / 64;
constexpr int RL_MAX_SOURCES = CTR_LINK_MAX_SOURCES;
constexpr int RL_MAX_BG = CTR_RELOCATE_MAX_BACKGROUND;
constexpr int RL_LIST = CTR_RELOCATE_MAX_MAXIMA;
static_assert(RL_LIST <= RL_THREADS, "one thread per list entry");

struct RlArgs {
  const void* frames;
  long long frame_elems;
  long long n_frames;
  int shape[3];          // frame extent per axis, (z,) y, x in slots 0 .. ND-1
  int radius[3];         // characterisation
  int slice_radius[3];   // visible ellipse, box
  double inv_slr2[3];    // 1 / slice_radius^2
  int box[3], lo[3];     // dilation box and its lower reach (box - 1) / 2
  double sep[3], inv_sep2[3];
  double sr[3];
  int sr_equal;          // all search ranges equal: the unscaled form of the reach test
  int isotropic;
  double max_dist2;      // max_dist * max_dist
  double minmass, scale_factor;
  const double* threshold;
  const double* known_pos;
  const long long* known_offset;
  long long n_known;
  long long n_queries;
  const long long* query_frame;
  const long long* source_offset;
  const double* source_pos;
  int K;
  int tile_elems;        // pixels the LDS tile holds (the plan's decision)
  int* n_found;
  int* cand_pos;
  double* mass;
  double* signal;
  double* size;
  int* status;
};

// what a query's threads share
template <int ND>
struct RlCtx {
  double rel[RL_MAX_SOURCES][ND];   // sources in box coordinates
  double bg[RL_MAX_BG][ND];         // background in box coordinates
  int org[ND], ext[ND];             // the box in the frame
  int n_src, n_bg;
};

// the masked value of box pixel p; 0 beyond the box
template <int ND, typename T>
__device__ __forceinline__ T rl_masked(const RlArgs& a, const RlCtx<ND>& c, const T* frame, const int (&p)[ND]) {
  size_t off = 0;
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    if (p[d] < 0 || p[d] >= c.ext[d]) return T(0);
    off = off * (size_t)a.shape[d] + (size_t)(c.org[d] + p[d]);
  }
  int slr[ND];
  double inv_slr2[ND], sep[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    slr[d] = a.slice_radius[d];
    inv_slr2[d] = a.inv_slr2[d];
    sep[d] = a.sep[d];
  }
  bool visible = false;
  for (int s = 0; s < c.n_src && !visible; ++s) visible = in_mask<ND>(p, c.rel[s], inv_slr2, slr);
  if (!visible) return T(0);
  for (int b = 0; b < c.n_bg; ++b) {
    // strictly inside the separation ellipse of a known feature: hidden.  Cheap form first, NumPy's
    // where the two could disagree
    double s = 0.;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const double dd = (double)p[d] - c.bg[b][d];
      s += dd * dd * a.inv_sep2[d];
    }
    const bool hidden = fabs(s - 1.) > 1e-9 ? s < 1. : ellipse_sum<ND, double>(p, c.bg[b], sep) < 1.;
    if (hidden) return T(0);
  }
  return frame[off];
}

// rows [ts, ts + trows) of the box, all of its other axes
template <int ND, typename T>
__device__ __forceinline__ T rl_tile_at(const T* tile, const RlCtx<ND>& c, int ts, int trows, const int (&p)[ND]) {
  const int r = p[0] - ts;
  if (p[0] < 0 || p[0] >= c.ext[0] || r < 0 || r >= trows) return T(0);
  int off = r;
#pragma unroll
  for (int d = 1; d < ND; ++d) {
    if (p[d] < 0 || p[d] >= c.ext[d]) return T(0);
    off = off * c.ext[d] + p[d];
  }
  return tile[off];
}

template <int ND>
__device__ __forceinline__ void rl_decode(int lin, const int (&ext)[ND], int (&p)[ND]) {
#pragma unroll
  for (int d = ND - 1; d > 0; --d) { p[d] = lin % ext[d]; lin /= ext[d]; }
  p[0] = lin;
}

template <int ND, typename T>
__global__ __launch_bounds__(RL_THREADS) void relocate_kernel(RlArgs a) {
  typedef typename ChrAcc<T>::type A;
  constexpr bool INTEGER = std::is_integral<T>::value;
  extern __shared__ __align__(16) unsigned char rl_smem[];
  T* tile = (T*)rl_smem;
  __shared__ RlCtx<ND> c;
  __shared__ double s_src[RL_MAX_SOURCES][ND];   // sources in frame coordinates
  __shared__ int s_state[4];                     // [0] box exists, [1] background found, [2] maxima listed, [3] survivors
  __shared__ int s_wcount[RL_WAVES];
  __shared__ int l_idx[RL_LIST];                 // box pixel of a maximum (C-order index)
  __shared__ T l_val[RL_LIST];
  __shared__ unsigned char l_reach[RL_LIST], l_keep[RL_LIST];
  __shared__ int l_surv[RL_LIST];
  __shared__ double r_mass[RL_LIST], r_signal[RL_LIST], r_size[RL_LIST][ND];

  const long long q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long t = a.query_frame[q];
  const long long s0 = a.source_offset[q], n_src_ll = a.source_offset[q + 1] - s0;
  int status = CTR_RELOCATE_OK;
  if (t < 0 || t >= a.n_frames) status = CTR_RELOCATE_BAD_FRAME;
  else if (n_src_ll > RL_MAX_SOURCES) status = CTR_RELOCATE_CAPACITY;
  const int n_src = status == CTR_RELOCATE_OK && n_src_ll > 0 ? (int)n_src_ll : 0;
  bool live = n_src > 0;      // the same in every thread, here and below
  int n_surv = 0;
  bool single = false;

  const T* frame = nullptr;
  double thr = 0.;
  if (live) {
    frame = (const T*)a.frames + (size_t)t * (size_t)a.frame_elems;
    thr = a.threshold[t];
    for (int i = tid; i < n_src * ND; i += RL_THREADS) s_src[i / ND][i % ND] = a.source_pos[s0 * ND + i];
    if (tid == 0) { c.n_src = n_src; c.n_bg = 0; s_state[1] = 0; s_state[2] = 0; }
  }
  __syncthreads();

  // ---- 1. the box: sources rounded half to even, those beyond the frame by more than the slice
  // radius dropped (masks._in_bounds)
  if (live && tid == 0) {
    long long mn[ND], mx[ND];
    bool any = false;
    for (int s = 0; s < n_src; ++s) {
      long long r[ND];
      bool in = true;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const double v = rint(s_src[s][d]);
        in = in && v >= -(double)a.slice_radius[d] && v < (double)a.shape[d] + (double)a.slice_radius[d];
        r[d] = in ? (long long)v : 0;
      }
      if (!in) continue;
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        mn[d] = any ? (r[d] < mn[d] ? r[d] : mn[d]) : r[d];
        mx[d] = any ? (r[d] > mx[d] ? r[d] : mx[d]) : r[d];
      }
      any = true;
    }
    s_state[0] = any;
    if (any) {
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const long long lo = mn[d] - a.slice_radius[d], hi = mx[d] + a.slice_radius[d] + 1;
        c.org[d] = (int)(lo < 0 ? 0 : lo);
        c.ext[d] = (int)(hi > a.shape[d] ? a.shape[d] : hi) - c.org[d];
      }
    }
  }
  __syncthreads();
  live = live && s_state[0] != 0;

  // ---- 2./3. sources into box coordinates; the background of the query
  if (live) {
    for (int i = tid; i < n_src * ND; i += RL_THREADS) c.rel[i / ND][i % ND] = s_src[i / ND][i % ND] - (double)c.org[i % ND];
    // (the offsets are the caller's and trusted; the range is only kept inside the table)
    const long long kb = a.known_offset[t] < 0 ? 0 : a.known_offset[t];
    const long long ke = a.known_offset[t + 1] > a.n_known ? a.n_known : a.known_offset[t + 1];
    for (long long i = kb + tid; i < ke; i += RL_THREADS) {
      double k[ND], kq[ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) { k[d] = a.known_pos[i * ND + d]; kq[d] = k[d] / a.sr[d]; }
      bool hit = false;
      for (int s = 0; s < n_src && !hit; ++s) {
        double sq[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) sq[d] = s_src[s][d] / a.sr[d];
        hit = scaled_dist2<ND>(kq, sq) <= a.max_dist2;
      }
      if (hit) {
        const int slot = atomicAdd(&s_state[1], 1);   // integer, LDS: the order in the list decides nothing
        if (slot < RL_MAX_BG) {
#pragma unroll
          for (int d = 0; d < ND; ++d) c.bg[slot][d] = k[d] - (double)c.org[d];
        }
      }
    }
  }
  __syncthreads();
  if (live && s_state[1] > RL_MAX_BG) { status = CTR_RELOCATE_CAPACITY; live = false; }
  if (live && tid == 0) c.n_bg = s_state[1];
  __syncthreads();

  // ---- 4.-6. m, slab after slab, and its maxima in C order
  if (live) {
    int tv = 1;
#pragma unroll
    for (int d = 1; d < ND; ++d) tv *= c.ext[d];
    const int rows0 = c.ext[0];
    single = (long long)rows0 * tv <= (long long)a.tile_elems;
    // rows of a slab; none fits (a box wider than the tile / dilation box): m is read from the
    // frame pixel by pixel instead, the whole box in one pass
    const int th_slab = a.tile_elems / tv - (a.box[0] - 1);
    const bool direct = !single && th_slab < 1;
    const int th = single || direct ? rows0 : th_slab;
    int ext1[ND];      // the box without axis 0
    ext1[0] = 1;
#pragma unroll
    for (int d = 1; d < ND; ++d) ext1[d] = c.ext[d];
    for (int r0 = 0; r0 < rows0 && s_state[2] <= RL_LIST; r0 += th) {
      const int ts = single ? 0 : r0 - a.lo[0];
      const int trows = single ? rows0 : th + a.box[0] - 1;
      if (!direct) {
        for (int i = tid; i < trows * tv; i += RL_THREADS) {
          int p[ND];
          rl_decode<ND>(i, ext1, p);     // p[0] = row of the tile
          p[0] += ts;
          tile[i] = rl_masked<ND, T>(a, c, frame, p);
        }
      }
      __syncthreads();
      const int rend = r0 + th < rows0 ? r0 + th : rows0;
      const int n_int = (rend - r0) * tv;
      for (int base = 0; base < n_int && s_state[2] <= RL_LIST; base += RL_THREADS) {
        const int i = base + tid;
        bool is = false;
        T v = T(0);
        if (i < n_int) {
          int p[ND];
          rl_decode<ND>(i, ext1, p);
          p[0] += r0;
          v = direct ? rl_masked<ND, T>(a, c, frame, p) : rl_tile_at<ND, T>(tile, c, ts, trows, p);
          if (loc_above<T>(v, thr)) {
            // a maximum: no pixel of the dilation box is larger (offsets -lo .. box - 1 - lo, 0 beyond the box)
            is = true;
            int o[3] = {0, 0, 0}, n[3] = {1, 1, 1};
#pragma unroll
            for (int d = 0; d < ND; ++d) n[3 - ND + d] = a.box[d];
            for (o[0] = 0; o[0] < n[0] && is; ++o[0])
              for (o[1] = 0; o[1] < n[1] && is; ++o[1])
                for (o[2] = 0; o[2] < n[2]; ++o[2]) {
                  int pn[ND];
#pragma unroll
                  for (int d = 0; d < ND; ++d) pn[d] = p[d] - a.lo[d] + o[3 - ND + d];
                  const T nb = direct ? rl_masked<ND, T>(a, c, frame, pn) : rl_tile_at<ND, T>(tile, c, ts, trows, pn);
                  if (v < nb) { is = false; break; }
                }
          }
        }
        const unsigned long long bal = __ballot(is);
        if (lane == 0) s_wcount[wave] = __popcll(bal);
        __syncthreads();
        int before = s_state[2], total = 0;
        for (int w = 0; w < RL_WAVES; ++w) { if (w < wave) before += s_wcount[w]; total += s_wcount[w]; }
        const int slot = before + __popcll(bal & ((1ull << lane) - 1ull));
        if (is && slot < RL_LIST) { l_idx[slot] = r0 * tv + i; l_val[slot] = v; }
        __syncthreads();
        if (tid == 0) s_state[2] += total;
        __syncthreads();
      }
      __syncthreads();   // the next slab overwrites the tile
    }
    if (s_state[2] > RL_LIST) { status = CTR_RELOCATE_CAPACITY; live = false; }
  }

  // ---- 7. within reach of a source; 8. drop close
  if (live) {
    const int n = s_state[2];
    int p[ND];
    double pd[ND], qi[ND], si = 0.;
    bool reach = false;
    if (tid < n) {
      rl_decode<ND>(l_idx[tid], c.ext, p);
#pragma unroll
      for (int d = 0; d < ND; ++d) { pd[d] = (double)p[d]; qi[d] = pd[d] / a.sep[d]; si = si + qi[d]; }
      for (int s = 0; s < n_src && !reach; ++s) {
        if (a.sr_equal) {
          reach = scaled_dist2<ND>(pd, c.rel[s]) <= a.sr[0] * a.sr[0];
        } else {
          double pq[ND], rq[ND];
#pragma unroll
          for (int d = 0; d < ND; ++d) { pq[d] = pd[d] / a.sr[d]; rq[d] = c.rel[s][d] / a.sr[d]; }
          reach = scaled_dist2<ND>(pq, rq) <= 1.;
        }
      }
      l_reach[tid] = reach;
    }
    __syncthreads();
    if (tid < n) {
      bool keep = reach;
      if (keep) {
        const double r = 1. - 1e-7, r2 = r * r;
        const T vi = l_val[tid];
        for (int j = 0; j < n && keep; ++j) {
          if (j == tid || !l_reach[j]) continue;
          int pj[ND];
          rl_decode<ND>(l_idx[j], c.ext, pj);
          double qj[ND], sj = 0.;
#pragma unroll
          for (int d = 0; d < ND; ++d) { qj[d] = (double)pj[d] / a.sep[d]; sj = sj + qj[d]; }
          if (!(scaled_dist2<ND>(qi, qj) <= r2)) continue;
          const T vj = l_val[j];
          if (vj > vi || (vj == vi && (sj > si || (sj == si && j > tid)))) keep = false;
        }
      }
      l_keep[tid] = keep;
    }
    __syncthreads();
    if (tid == 0) {
      int m = 0;
      for (int i = 0; i < n; ++i) if (l_keep[i]) l_surv[m++] = i;
      s_state[3] = m;
    }
    __syncthreads();
    n_surv = s_state[3];
  }

  // ---- 9. characterise every survivor on m: a wavefront each (the rule of characterize_kernel
  // for an integer centre: the window's corner is centre - radius, the mask centre is the radius)
  if (live && n_surv > 0) {
    int radius[ND], wshape[ND], ext1[ND];
    double rel_w[ND], inv_r2[ND];
    int vol = 1, tv = 1;
    ext1[0] = 1;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      radius[d] = a.radius[d];
      rel_w[d] = (double)radius[d];
      inv_r2[d] = 1. / ((double)radius[d] * (double)radius[d]);
      wshape[d] = 2 * radius[d] + 1;
      vol *= wshape[d];
      if (d > 0) { tv *= c.ext[d]; ext1[d] = c.ext[d]; }
    }
    for (int k = wave; k < n_surv; k += RL_WAVES) {
      int ctr[ND];
      rl_decode<ND>(l_idx[l_surv[k]], c.ext, ctr);
      A mass = 0, mx = 0, w[ND];
      bool any = false;
#pragma unroll
      for (int d = 0; d < ND; ++d) w[d] = 0;
      for (int pw = lane; pw < vol; pw += 64) {
        int idx[ND], g[ND];
        rl_decode<ND>(pw, wshape, idx);
#pragma unroll
        for (int d = 0; d < ND; ++d) g[d] = ctr[d] - radius[d] + idx[d];
        const T px = single ? rl_tile_at<ND, T>(tile, c, 0, c.ext[0], g) : rl_masked<ND, T>(a, c, frame, g);
        const bool inside = in_mask<ND>(idx, rel_w, inv_r2, radius);
        A v;
        if (INTEGER) v = inside ? (A)px : (A)0;
        else v = (A)px * (inside ? (A)1 : (A)0);
        mass = chr_add(mass, v);
        mx = any ? chr_max(mx, v) : v;
        any = true;
        if (inside) {
#pragma unroll
          for (int d = 0; d < ND; ++d) {
            const int kk = idx[d] - radius[d];
            w[d] = chr_add(w[d], (A)(kk * kk) * v);
          }
        } else if (!INTEGER) {
#pragma unroll
          for (int d = 0; d < ND; ++d) w[d] = chr_add(w[d], (A)0 * v);
        }
      }
      const A first = __shfl(mx, 0);
      if (!any) mx = first;
      mass = chr_reduce<64, false>(mass);
      mx = chr_reduce<64, true>(mx);
#pragma unroll
      for (int d = 0; d < ND; ++d) w[d] = chr_reduce<64, false>(w[d]);
      if (lane == 0) {
        r_mass[k] = (double)mass / a.scale_factor;
        r_signal[k] = (double)mx / a.scale_factor;
        if (a.isotropic) {
          A s = w[0];
#pragma unroll
          for (int d = 1; d < ND; ++d) s = chr_add(s, w[d]);
          r_size[k][0] = sqrt((double)s / (double)mass);
        } else {
#pragma unroll
          for (int d = 0; d < ND; ++d) r_size[k][d] = sqrt((double)((A)ND * w[d]) / (double)mass);
        }
      }
    }
  }
  __syncthreads();

  // ---- 10. mass >= minmass, by mass descending, equal masses in C order; the rest of the K rows
  // -1 / NaN
  bool pass = false;
  double my_mass = 0.;
  if (live && tid < n_surv) {
    my_mass = r_mass[tid];
    pass = my_mass >= a.minmass;
  }
  const int n_found = __syncthreads_count(pass ? 1 : 0);
  const int n_size = a.isotropic ? 1 : ND;
  const size_t row0 = (size_t)q * (size_t)a.K;
  if (pass) {
    int rank = 0;
    for (int j = 0; j < n_surv; ++j) {
      const double mj = r_mass[j];
      if (mj >= a.minmass && (mj > my_mass || (mj == my_mass && j < tid))) ++rank;
    }
    if (rank < a.K) {
      int ctr[ND];
      rl_decode<ND>(l_idx[l_surv[tid]], c.ext, ctr);
      const size_t row = row0 + rank;
#pragma unroll
      for (int d = 0; d < ND; ++d) a.cand_pos[row * ND + d] = ctr[d] + c.org[d];
      a.mass[row] = my_mass;
      a.signal[row] = r_signal[tid];
      for (int d = 0; d < n_size; ++d) a.size[row * n_size + d] = r_size[tid][d];
    }
  }
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int r = (n_found < a.K ? n_found : a.K) + tid; r < a.K; r += RL_THREADS) {
    const size_t row = row0 + r;
#pragma unroll
    for (int d = 0; d < ND; ++d) a.cand_pos[row * ND + d] = -1;
    a.mass[row] = nan;
    a.signal[row] = nan;
    for (int d = 0; d < n_size; ++d) a.size[row * n_size + d] = nan;
  }
  if (tid == 0) {
    a.n_found[q] = n_found;
    a.status[q] = status;
  }
}

#endif  // CTREFINE_RELOCATE_KERNELS_H
