// cluster_track_kernels.h -- cluster tracks: from linked features to the motion stage's input
// (ctr_cluster_tracks_device, ctr_track_positions_device; include/ctrefine.h has the rule, DESIGN.md
// 7b).  Included by tu_cluster_tracks.hip inside its anonymous namespace, after stage_common.h.
// Integers and copies of doubles only.  The kernel boundary is the only synchronisation between
// workgroups; every loop is bounded by the launch's arguments or, for the rows of a frame, by
// offsets that ctk_setup_kernel has checked against them; integer atomicMin / atomicAdd only.
#ifndef CTREFINE_CLUSTER_TRACK_KERNELS_H
#define CTREFINE_CLUSTER_TRACK_KERNELS_H

constexpr int CTK_THREADS = 256;        // a workgroup of every kernel here: 4 wavefronts

struct CtkArgs {
  int cs, ndim;
  long long min_frames;
  long long T, N, P, M;      // frames, rows, particles, key slots = N (cs - 1)
  const long long* frame_offset;
  const long long* particle;
  const long long* cluster;
  long long* keys;
  // components: labels at the round's start / being hooked and flattened, members per root,
  // track number per root, roots per block of CTK_THREADS particles, the words of the rounds
  int* A;
  int* B;
  int* size;
  int* num;
  int* blocksum;
  int* flags;                // [R][J + 1]: the hook of round r, then its jumps, changed anything
  int R, J;
  int* track_of;
  int* n_tracks;
  int* n_members;
  int* status;
  int* n_rounds;
  // positions
  long long n_trk;
  const int* track_in;
  const double* pos;
  int* present;
  double* pos_out;
};

// The caller's tables, before any kernel follows an index: offsets monotone and within N,
// particle < P, track < n_tracks (positions only; track_in null otherwise).  fill_keys: every key
// slot starts as CTR_TRACKS_NO_KEY.  status[0] was zeroed in front of this kernel.
__global__ void __launch_bounds__(CTK_THREADS) ctk_setup_kernel(const CtkArgs a, int fill_keys) {
  const long long stride = (long long)gridDim.x * CTK_THREADS;
  long long n = a.T + 1 > a.N ? a.T + 1 : a.N;
  n = a.P > n ? a.P : n;
  if (fill_keys && a.M > n) n = a.M;
  bool bad = false;
  for (long long i = (long long)blockIdx.x * CTK_THREADS + threadIdx.x; i < n; i += stride) {
    if (i <= a.T) bad |= offsets_bad(a.frame_offset, i, a.T, a.N);
    if (i < a.N) bad |= a.particle[i] >= a.P;
    if (a.track_in && i < a.P) bad |= (long long)a.track_in[i] >= a.n_trk;
    if (fill_keys && i < a.M) a.keys[i] = CTR_TRACKS_NO_KEY;
  }
  if (bad) st_agent(a.status, CTR_TRACKS_BAD_TABLE);
}

// One workgroup per frame.  Every row counts the rows of the frame with its `cluster` value (tiles
// of CTK_THREADS rows through LDS), keeps the particles of the first four, decides whether the group
// is complete and writes one key per member of higher rank (= larger particle: they are pairwise
// different in a complete group).
__global__ void __launch_bounds__(CTK_THREADS) ctk_groups_kernel(const CtkArgs a) {
  __shared__ long long s_cl[CTK_THREADS], s_pt[CTK_THREADS];
  if (ld_agent(a.status) != CTR_TRACKS_OK) return;
  const int tid = threadIdx.x, cs = a.cs;
  for (long long f = blockIdx.x; f < a.T; f += gridDim.x) {
    const long long r0 = a.frame_offset[f], r1 = a.frame_offset[f + 1];
    for (long long base = r0; base < r1; base += CTK_THREADS) {
      const long long i = base + tid;
      const bool act = i < r1;
      const long long ci = act ? a.cluster[i] : 0, pi = act ? a.particle[i] : -1;
      int cnt = 0;
      long long mp[4] = {-1, -1, -1, -1};
      for (long long tb = r0; tb < r1; tb += CTK_THREADS) {
        __syncthreads();
        if (tb + tid < r1) { s_cl[tid] = a.cluster[tb + tid]; s_pt[tid] = a.particle[tb + tid]; }
        __syncthreads();
        const int n = r1 - tb < CTK_THREADS ? (int)(r1 - tb) : CTK_THREADS;
        if (act)
          for (int q = 0; q < n; ++q)
            if (s_cl[q] == ci) {
#pragma unroll
              for (int m = 0; m < 4; ++m)
                if (cnt == m) mp[m] = s_pt[q];
              ++cnt;
            }
      }
      if (!act) continue;
      bool complete = cnt == cs;
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (m < cs) {
          complete &= mp[m] >= 0;
#pragma unroll
          for (int m2 = 0; m2 < m; ++m2) complete &= mp[m] != mp[m2];
        }
      if (!complete) continue;       // its slots keep CTR_TRACKS_NO_KEY
      long long* slot = a.keys + i * (cs - 1);
      int k = 0;
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (m < cs && mp[m] > pi) slot[k++] = (pi << 32) | mp[m];
    }
  }
}

__global__ void __launch_bounds__(CTK_THREADS) ctk_init_kernel(const CtkArgs a) {
  const long long stride = (long long)gridDim.x * CTK_THREADS;
  for (long long i = (long long)blockIdx.x * CTK_THREADS + threadIdx.x; i < a.P; i += stride) {
    a.A[i] = a.B[i] = (int)i;
    a.size[i] = 0;
  }
}

// slot e of the sorted keys is an edge: the first of a run of at least min_frames equal keys (one
// edge per bonded pair, however many frames repeat it: a pair seen in every frame would otherwise
// send a thousand atomics to one word), and both ids are below P (CTR_TRACKS_NO_KEY is not)
__device__ __forceinline__ bool ctk_edge(const CtkArgs& a, long long e, int& lo, int& hi) {
  const long long k = a.keys[e], last = e + a.min_frames - 1;
  if (last >= a.M || a.keys[last] != k || (e > 0 && a.keys[e - 1] == k)) return false;
  const unsigned long long l = (unsigned long long)k >> 32, h = (unsigned long long)k & 0xffffffffull;
  if (l >= (unsigned long long)a.P || h >= (unsigned long long)a.P) return false;
  lo = (int)l;
  hi = (int)h;
  return true;
}

// Round r, hook: A holds the labels of the round's start (stars: every label is a root, A == B);
// an edge between two trees hangs the root with the larger id under the smaller in B.  The roots
// then form chains of descending ids, never a cycle.
__global__ void __launch_bounds__(CTK_THREADS) ctk_hook_kernel(const CtkArgs a, int r) {
  if (ld_agent(a.status) != CTR_TRACKS_OK) return;
  if (r > 0 && ld_agent(a.flags + (size_t)(r - 1) * (a.J + 1)) == 0) return;   // the round before hooked nothing: done
  const long long stride = (long long)gridDim.x * CTK_THREADS;
  bool changed = false;
  for (long long e = (long long)blockIdx.x * CTK_THREADS + threadIdx.x; e < a.M; e += stride) {
    int u, v;
    if (!ctk_edge(a, e, u, v)) continue;
    const int ra = a.A[u], rb = a.A[v];
    if (ra == rb) continue;
    atomicMin(a.B + (ra > rb ? ra : rb), ra > rb ? rb : ra);
    changed = true;
  }
  if (changed) st_agent(a.flags + (size_t)r * (a.J + 1), 1);
}

// Round r, jump j: B[i] = B[B[i]], in place -- a label read here is the old one or one further up,
// so the depth of every tree at least halves -- and A[i] = B[i].  Returns at once when the round's
// hook, or the jump before, changed nothing: B is then flat and A == B.
__global__ void __launch_bounds__(CTK_THREADS) ctk_jump_kernel(const CtkArgs a, int r, int j) {
  if (ld_agent(a.status) != CTR_TRACKS_OK) return;
  int* fl = a.flags + (size_t)r * (a.J + 1);
  if (ld_agent(fl) == 0 || (j > 0 && ld_agent(fl + j) == 0)) return;
  const long long stride = (long long)gridDim.x * CTK_THREADS;
  bool changed = false;
  for (long long i = (long long)blockIdx.x * CTK_THREADS + threadIdx.x; i < a.P; i += stride) {
    const int p = ld_agent(a.B + i), g = ld_agent(a.B + p);
    if (g != p) { st_agent(a.B + i, g); changed = true; }
    a.A[i] = g;
  }
  if (changed) st_agent(fl + 1 + j, 1);
}

// Would a further round change anything?  Every edge inside one tree, every tree a star.
__global__ void __launch_bounds__(CTK_THREADS) ctk_verify_kernel(const CtkArgs a) {
  if (ld_agent(a.status) != CTR_TRACKS_OK) return;
  const long long stride = (long long)gridDim.x * CTK_THREADS;
  const long long n = a.M > a.P ? a.M : a.P;
  bool open = false;
  for (long long i = (long long)blockIdx.x * CTK_THREADS + threadIdx.x; i < n; i += stride) {
    int u, v;
    if (i < a.M && ctk_edge(a, i, u, v)) open |= a.A[u] != a.A[v];
    if (i < a.P) open |= a.A[a.A[i]] != a.A[i] || a.B[i] != a.A[i];
  }
  if (open) st_agent(a.status, CTR_TRACKS_ROUNDS);
}

__global__ void __launch_bounds__(CTK_THREADS) ctk_count_kernel(const CtkArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.n_rounds) {
    int used = 0;
    for (int r = 0; r < a.R; ++r) used += ld_agent(a.flags + (size_t)r * (a.J + 1)) != 0;
    *a.n_rounds = used;
  }
  if (ld_agent(a.status) != CTR_TRACKS_OK) return;
  const long long stride = (long long)gridDim.x * CTK_THREADS;
  for (long long i = (long long)blockIdx.x * CTK_THREADS + threadIdx.x; i < a.P; i += stride) atomicAdd(a.size + a.A[i], 1);
}

// particle i is the root of a track: the smallest id of a component of at least two
__device__ __forceinline__ bool ctk_track_root(const CtkArgs& a, long long i, bool ok) {
  return ok && i < a.P && a.A[i] == (int)i && a.size[i] >= 2;
}

// grid = blocks of CTK_THREADS particles
__global__ void __launch_bounds__(CTK_THREADS) ctk_blocksum_kernel(const CtkArgs a) {
  const bool ok = ld_agent(a.status) == CTR_TRACKS_OK;
  const long long i = (long long)blockIdx.x * CTK_THREADS + threadIdx.x;
  const int n = __syncthreads_count(ctk_track_root(a, i, ok) ? 1 : 0);
  if (threadIdx.x == 0) a.blocksum[blockIdx.x] = n;
}

// one workgroup: exclusive scan of the nb block counts in place, n_tracks = their sum
__global__ void __launch_bounds__(CTK_THREADS) ctk_scan_kernel(const CtkArgs a, long long nb) {
  const int n = workgroup_scan_n<CTK_THREADS, int>(
      nb, [&](long long i) { return a.blocksum[i]; }, [&](long long i, int before) { a.blocksum[i] = before; });
  if (threadIdx.x == 0) *a.n_tracks = n;
}

// the roots in ascending order, compacted: number = roots of the blocks before + rank in the block
__global__ void __launch_bounds__(CTK_THREADS) ctk_number_kernel(const CtkArgs a) {
  __shared__ int s_wave[CTK_THREADS / 64];
  const bool ok = ld_agent(a.status) == CTR_TRACKS_OK;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = (long long)blockIdx.x * CTK_THREADS + tid;
  const bool root = ctk_track_root(a, i, ok);
  const unsigned long long mask = __ballot(root);
  if (lane == 0) s_wave[wave] = __popcll(mask);
  __syncthreads();
  if (!root) return;
  int k = a.blocksum[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) k += s_wave[w];
  a.num[i] = k;
  a.n_members[k] = a.size[i];
}

__global__ void __launch_bounds__(CTK_THREADS) ctk_assign_kernel(const CtkArgs a) {
  const bool ok = ld_agent(a.status) == CTR_TRACKS_OK;
  const long long stride = (long long)gridDim.x * CTK_THREADS;
  for (long long i = (long long)blockIdx.x * CTK_THREADS + threadIdx.x; i < a.P; i += stride) {
    int k = -1;
    if (ok) {
      const int r = a.A[i];
      if (a.size[r] >= 2) k = a.num[r];
    }
    a.track_of[i] = k;
  }
}

// ---- positions ----
__global__ void __launch_bounds__(CTK_THREADS) ctk_fill_kernel(const CtkArgs a) {
  const long long stride = (long long)gridDim.x * CTK_THREADS;
  const long long cells = a.n_trk * a.T, n = cells * a.cs * a.ndim;
  for (long long i = (long long)blockIdx.x * CTK_THREADS + threadIdx.x; i < n; i += stride) {
    a.pos_out[i] = __builtin_nan("");
    if (i < cells) a.present[i] = 0;
  }
}

// the track of a row, or -1 (tables checked by ctk_setup_kernel)
__device__ __forceinline__ int ctk_row_track(const CtkArgs& a, long long p) { return p >= 0 ? a.track_in[p] : -1; }

// one workgroup per frame; one integer add per member row
__global__ void __launch_bounds__(CTK_THREADS) ctk_present_kernel(const CtkArgs a) {
  if (ld_agent(a.status) != CTR_TRACKS_OK) return;
  for (long long f = blockIdx.x; f < a.T; f += gridDim.x) {
    const long long r0 = a.frame_offset[f], r1 = a.frame_offset[f + 1];
    for (long long i = r0 + threadIdx.x; i < r1; i += CTK_THREADS) {
      const int k = ctk_row_track(a, a.particle[i]);
      if (k >= 0) atomicAdd(a.present + (long long)k * a.T + f, 1);
    }
  }
}

// one workgroup per frame; a member row of a (track, frame) cell with exactly cluster_size rows
// finds its rank by (particle, row) among the rows of the frame (tiles through LDS) and copies its
// position there: every slot of such a cell is written once
__global__ void __launch_bounds__(CTK_THREADS) ctk_scatter_kernel(const CtkArgs a) {
  __shared__ long long s_pt[CTK_THREADS];
  __shared__ int s_tr[CTK_THREADS];
  if (ld_agent(a.status) != CTR_TRACKS_OK) return;
  const int tid = threadIdx.x;
  for (long long f = blockIdx.x; f < a.T; f += gridDim.x) {
    const long long r0 = a.frame_offset[f], r1 = a.frame_offset[f + 1];
    for (long long base = r0; base < r1; base += CTK_THREADS) {
      const long long i = base + tid;
      const long long pi = i < r1 ? a.particle[i] : -1;
      const int k = i < r1 ? ctk_row_track(a, pi) : -1;
      const bool act = k >= 0 && a.present[(long long)k * a.T + f] == a.cs;
      int rank = 0;
      for (long long tb = r0; tb < r1; tb += CTK_THREADS) {
        __syncthreads();
        if (tb + tid < r1) {
          const long long p = a.particle[tb + tid];
          s_pt[tid] = p;
          s_tr[tid] = ctk_row_track(a, p);
        }
        __syncthreads();
        const int n = r1 - tb < CTK_THREADS ? (int)(r1 - tb) : CTK_THREADS;
        if (act)
          for (int q = 0; q < n; ++q)
            rank += s_tr[q] == k && (s_pt[q] < pi || (s_pt[q] == pi && tb + q < i));
      }
      if (!act) continue;
      double* out = a.pos_out + (((long long)k * a.T + f) * a.cs + rank) * a.ndim;
      for (int d = 0; d < a.ndim; ++d) out[d] = a.pos[i * a.ndim + d];
    }
  }
}

#endif  // CTREFINE_CLUSTER_TRACK_KERNELS_H
