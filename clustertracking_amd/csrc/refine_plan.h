// refine_plan.h -- what a ctr_refine_batch_device call launches.
//
// ctr_plan_create decides here, once per plan: the bin of every cluster, their order, and the list
// of kernel launches -- which kernel, with which grid, gate, work counter and part of its bin
// (kargs.h: KArgs::split*, TailArgs).  A call walks the list and places its chains (lane_sched.h);
// it decides nothing.  Host code only and no HIP type: tests/native/refine_plan_main.cpp checks
// without a device that the launches reading a bin fit every cluster of it exactly once, whatever
// count front_load_kernel writes.
#ifndef CTR_REFINE_PLAN_H
#define CTR_REFINE_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "ctrefine.h"
#include "engine_dims.h"
#include "lane_sched.h"

namespace refine_plan {

// bins: 0..MAXNT-1 generic kernel by NT-1; MAXNT = beyond the engine (see CTR_STATUS_TOO_LARGE);
// MAXNT+1 / MAXNT+2 = singles / pairs with default modes (small kernel); MAXNT+3 = large
// clusters (more than MAXF features or 16 MAXNT columns: refine_large_kernel)
// MAXNT+4 / MAXNT+5 = clusters with equality constraints, NT = 1 / 2 (their own instantiation of
// the block kernel)
constexpr int BIN_TOO_LARGE = MAXNT, BIN_SMALL1 = MAXNT + 1, BIN_SMALL2 = MAXNT + 2, BIN_LARGE = MAXNT + 3,
              BIN_CONS1 = MAXNT + 4, BIN_CONS2 = MAXNT + 5, NBINS = MAXNT + 6;
static_assert(NBINS <= 16, "FrontArgs (aux_kernels.h) holds 16 bins");
// slots of the handle's kernel table (ctr_handle::kernels): a block family's NT 1..8 at nt - 1 and
// its constrained NT 1..2 at MAXNT + nt - 1; the small kernel's tiers; the large kernel's one at 0
constexpr int NSLOT = MAXNT + 2;
constexpr int SLOT_SINGLES8 = 0, SLOT_SINGLES64 = 1, SLOT_PAIRS64 = 2, SLOT_PAIRS16 = 3;
// pixels of a single-feature window up to which singles take 8 lanes (else 64) and a bin of pairs
// may run in two tiers
constexpr int64_t NARROW_WINDOW = 600;
// launches of a call that are chains of their own on the lanes: one per bin, the bulk tier of
// the pairs, and the tail launch
constexpr int LAUNCH_PAIRS16 = NBINS, LAUNCH_TAIL = NBINS + 1, NLAUNCH = NBINS + 2;
// Most workgroups that a bin has in the tail launch (tail_kernel.h).  They share the bin's entries
// of that launch, however many, through a counter.  It bounds the grid of a launch whose count is
// known on the device only: the shards of the benchmark (cfg 2) have at most 110 likely slow
// clusters in a bin, and 3 * 256 workgroups that find nothing to do cost a few microseconds.
constexpr int TAIL_CAP = 256;
// A block bin (NT = 1, 2) of at most this many clusters is fitted whole by the tail launch and has
// no launch of its own: its workgroups would run no faster there, and the launch would hold a
// queue as long as the bin's slowest far cluster.  The default of ctr_set_tail_absorb, fixed by
// measurement (profiles/tail_absorb_sweep.json): a bin of 6 440 3-4-feature
// clusters still gains from it, and at about 32 fits of 5-10 features per workgroup the tail
// launch would begin to outlast the slow fits it exists for.
constexpr int TAIL_ABSORB = 32 * TAIL_CAP;
// One tier of pairs (fewer than 64, or wide windows) is fitted whole by the tail launch up to this
// many: beyond it a bin of wide-window pairs is no work for TAIL_CAP wavefronts.
constexpr int TAIL_PAIRS_WHOLE = 8 * TAIL_CAP;
// the bins that a tail launch draws from, in the order of its segments (kargs.h: TailArgs)
constexpr int TAIL_BINS[TAIL_SEGMENTS] = {BIN_SMALL2, 0, 1};
// most workgroups of a small-kernel launch, which pulls its clusters from a work counter; the
// 64-lane pairs beside the 16-lane tier: persistent, a wavefront takes pair after pair
constexpr int64_t SMALL_MAX_GRID = 8192, PAIRS64_TIER_GRID = 2048;

inline int n_vars(const ctr_problem* p, int n) {
  int nv = 0;
  for (int k = 0; k < p->n_params; ++k) {
    if (p->modes[k] == CTR_MODE_VAR) nv += n;
    else if (p->modes[k] != CTR_MODE_CONST) nv += 1;
  }
  return nv;
}

// a lowpass of the window (ctr_problem.noise_size / CTR_FLAG_WINDOW_FILTER; noise_size given
// with every sigma 0: the reference's lowpass is then its threshold alone)
inline bool lowpass_of(const ctr_problem* p) {
  bool lp = (p->flags & CTR_FLAG_WINDOW_FILTER) != 0;
  for (int a = 0; a < p->ndim; ++a) lp = lp || p->noise_size[a] > 0.;
  return lp;
}

// pixels of a single-feature window (and of a mask's bounding box)
inline int64_t window_volume(const ctr_problem* p) {
  int64_t vol = 1;
  for (int a = 0; a < p->ndim; ++a) vol *= 2 * (int64_t)p->radius[a] + 1;
  return vol;
}

// The per-cluster decision: the bin, and the cell of the handle's kernel table that the bin is
// launched with (family, slot).  p is validated, n >= 0.
struct KernelChoice { int bin, family, slot; };

inline KernelChoice choose_kernel(const ctr_problem* p, int64_t n) {
  // singles / pairs with the default modes (fitfunc.py:356,379-387) go to the small kernel
  bool default_modes = p->modes[0] == CTR_MODE_CLUSTER && p->modes[1] == CTR_MODE_VAR;
  for (int a = 0; a < p->ndim; ++a) default_modes = default_modes && p->modes[2 + a] == CTR_MODE_VAR;
  for (int k2 = 2 + p->ndim; k2 < p->n_params; ++k2) default_modes = default_modes && p->modes[k2] == CTR_MODE_CONST;
  const int npf = n_vars(p, 1) - n_vars(p, 0), nsh = n_vars(p, 0);   // per-feature / shared variables
  const bool lowpass = lowpass_of(p);
  // (the lowpass lives in its own instantiations of the block kernel: every cluster goes there)
  if (lowpass) default_modes = false;
  // (so do the ring / disc profiles; clusters beyond the block kernel get status 5 there)
  const bool other_profile = p->fit_function != CTR_FIT_GAUSS;
  if (other_profile) default_modes = false;
  int bin;
  const bool constrained = (p->constraint_kind == CTR_CONS_DIMER && n == 2);
  const bool any_cons = (p->constraint_kind == CTR_CONS_DIMER && n == 2) ||
                        (p->constraint_kind == CTR_CONS_TRIMER && n == 3) ||
                        (p->constraint_kind == CTR_CONS_TETRAMER && n == 4);
  if (n > 0x3fffffLL) bin = BIN_TOO_LARGE;
  else if (n > MAXF) bin = BIN_LARGE;
  else if (default_modes && n == 1) bin = BIN_SMALL1;
  else if (default_modes && n == 2 && !constrained) bin = BIN_SMALL2;
  else {
    const int nv = n_vars(p, (int)n);
    const int nt = (nv + 1 + 15) / 16;
    bin = nt > MAXNT ? BIN_LARGE : (nt < 1 ? 0 : nt - 1);
    if (bin < MAXNT && n > (16 * (bin + 1) < MAXF ? 16 * (bin + 1) : MAXF)) bin = BIN_LARGE;
    if (any_cons && bin < 2) bin = bin == 0 ? BIN_CONS1 : BIN_CONS2;   // (at most 29 variables)
    else if (any_cons && bin < MAXNT) bin = BIN_TOO_LARGE;             // (ring / disc with every column free)
  }
  if (bin == BIN_LARGE) {
    // the large kernel's 16-column row: [r, shared.., own.., r_o, shared_o..]
    bool wide_mask = false;   // (its list of mask pixels packs box coordinates in 10 bits per axis)
    for (int a = 0; a < p->ndim; ++a) wide_mask = wide_mask || p->radius[a] > 500;
    if (npf < 1 || 2 + 2 * nsh + npf > 16 || other_profile || wide_mask) bin = BIN_TOO_LARGE;
  }
  // which table the kernel comes from, and its slot there
  int fam = CTR_KFAM_NONE;
  if (bin == BIN_SMALL1 || bin == BIN_SMALL2) fam = CTR_KFAM_SMALL;
  else if (bin == BIN_LARGE) fam = lowpass ? CTR_KFAM_LARGE_LOWPASS : CTR_KFAM_LARGE;
  else if (bin != BIN_TOO_LARGE) {
    if (p->fit_function == CTR_FIT_RING) fam = CTR_KFAM_RING;
    else if (p->fit_function == CTR_FIT_DISC) fam = CTR_KFAM_DISC;
    else if (p->fit_function == CTR_FIT_INV_SERIES) fam = CTR_KFAM_INV_SERIES;
    else if (lowpass) fam = CTR_KFAM_LOWPASS;
    // (2D only: a 3D window has thousands of pixels, more wavefronts per cluster pay there)
    else if ((p->flags & CTR_FLAG_THROUGHPUT) != 0 && p->ndim == 2) fam = CTR_KFAM_GAUSS_TP;
    else fam = CTR_KFAM_GAUSS;
  }
  int slot = 0;
  if (bin < MAXNT) slot = bin;
  else if (bin == BIN_CONS1 || bin == BIN_CONS2) slot = MAXNT + (bin == BIN_CONS2);
  // singles: 8 lanes per cluster (eight clusters per wavefront: the solve, replicated in the lanes
  // of a group, is shared by as many) while a window is a few passes, 64 once it is thousands of
  // pixels (3D); pairs 64
  else if (bin == BIN_SMALL1) slot = window_volume(p) > NARROW_WINDOW ? SLOT_SINGLES64 : SLOT_SINGLES8;
  else if (bin == BIN_SMALL2) slot = SLOT_PAIRS64;
  return KernelChoice{bin, fam, slot};
}

// One kernel launch of a call, a chain of its own on the lanes.
enum LaunchKind { KIND_BLOCK, KIND_TAIL, KIND_LARGE, KIND_MARK, KIND_SMALL };   // which argument list the kernel takes
struct LaunchSpec {
  int launch;        // index into ctr_plan::timing: the bin, LAUNCH_PAIRS16 or LAUNCH_TAIL
  int kind;          // LaunchKind
  int bin;           // whose order[] range and n_bin it gets (TAIL: -1, n_bin 0, order = the whole call)
  int family, slot;  // cell of the handle's kernel table (TAIL: the tail kernel by iso; MARK: mark_kernel)
  long long grid;    // workgroups
  bool gated, delay_first;   // waits for ev_gate; one more delay_kernel in front (the 16-lane tier)
  int counter;       // index into the handle's work counters, -1: none (TAIL: its segments use counter .. counter + 2)
  bool split;        // KArgs::split = the bin's count of front_load_kernel, else null
  int32_t split_part, split_cap;
  lane_sched::ChainClass cls; long long count; int nt;   // the arguments of static_guess
};

struct RefinePlan {
  int64_t bin_begin[NBINS + 1] = {0};
  int64_t bin_count[NBINS] = {0};
  // choose_kernel's family and table slot of each bin (the same for every cluster of a bin)
  int32_t bin_family[NBINS] = {0};
  int32_t bin_slot[NBINS] = {0};
  bool lowpass = false;       // lowpass_of: it lives in its own instantiations of the block kernel
  // what the launches do besides, decided from the problem and the bin counts
  bool gate = false;          // the small kernels start a little after the others (delay_kernel)
  bool pairs_split = false;   // the pairs bin runs in two tiers, 16 and 64 lanes per pair
  // the likely slow fits of the pairs and of the block bins NT = 1, 2 run in one launch of
  // refine_tail_kernel, of tail_grid workgroups
  bool tail_fused = false;
  int tail_grid = 0;
  // per segment of a fused plan (kargs.h: TailArgs): the tail launch fits the whole bin / the bin's
  // own launch (pairs: the 64-lane one) is queued.  Not fused: none whole, every non-empty bin its own
  bool tail_whole[TAIL_SEGMENTS] = {false, false, false};
  bool tail_own[TAIL_SEGMENTS] = {false, false, false};
  // the segments of the tail launch as TailArgs has them (all 0 where the plan is not fused)
  struct {
    int32_t ord_off[TAIL_SEGMENTS], grid_begin[TAIL_SEGMENTS + 1], whole[TAIL_SEGMENTS];
  } tail = {};
  int large_workgroups = 0;   // per large cluster, leader included
  // every launch of a call, in the order in which its chains are given to the placement
  // (lane_sched::Pool::place breaks ties by it)
  std::vector<LaunchSpec> launches;
};

// Fills *rp from a validated problem and the clusters' feature counts (feat_offset[c + 1] -
// feat_offset[c]); tail_absorb: ctr_set_tail_absorb.  *order: the clusters bin by bin, as the
// device gets them; *bin_of: the bin of every cluster.  Returns null, or what is wrong.
inline const char* make_plan(const ctr_problem* p, int64_t n_clusters, const int32_t* feat_offset, int32_t tail_absorb,
                             RefinePlan* rp, std::vector<int32_t>* order, std::vector<int32_t>* bin_of) {
  *rp = RefinePlan();
  rp->lowpass = lowpass_of(p);
  bin_of->assign((size_t)n_clusters, 0);
  for (int64_t c = 0; c < n_clusters; ++c) {
    const int64_t n = (int64_t)feat_offset[c + 1] - feat_offset[c];
    if (n < 0) return "feat_offset must be non-decreasing";
    const KernelChoice kc = choose_kernel(p, n);
    const int bin = kc.bin;
    // (family and slot depend on the problem alone: the launch takes them from the plan)
    if (rp->bin_count[bin] == 0) { rp->bin_family[bin] = kc.family; rp->bin_slot[bin] = kc.slot; }
    else if (rp->bin_family[bin] != kc.family || rp->bin_slot[bin] != kc.slot)
      return "internal: clusters of one bin with different kernels";
    (*bin_of)[(size_t)c] = bin;
    rp->bin_count[bin]++;
  }
  rp->bin_begin[0] = 0;
  for (int b = 0; b < NBINS; ++b) rp->bin_begin[b + 1] = rp->bin_begin[b] + rp->bin_count[b];
  const bool throughput = (p->flags & CTR_FLAG_THROUGHPUT) != 0;
  // the small kernels start a little later than the block and large kernels, if any (delay_kernel)
  rp->gate = n_clusters > rp->bin_count[BIN_SMALL1] + rp->bin_count[BIN_SMALL2] + rp->bin_count[BIN_TOO_LARGE];
  // Pairs in two tiers (CTR_FLAG_THROUGHPUT: +9 % with four batches in flight, but the
  // one-batch-at-a-time step gets 12 % longer).  One wavefront per pair gives the shortest
  // iteration, which is what the slow fits need; for the rest, four pairs per wavefront cost a
  // third of the machine time.
  rp->pairs_split = throughput && rp->bin_count[BIN_SMALL2] >= 64 && window_volume(p) <= NARROW_WINDOW;
  // One tail launch for the likely slow fits of the pairs and of the block bins NT = 1, 2
  // (tail_kernel.h), where queue time is what counts (CTR_FLAG_THROUGHPUT) and at least two of
  // them would otherwise hold a queue each.  Only the bins whose kernels the tail kernel holds:
  // 2D, no lowpass, the throughput table of the gaussian.
  {
    int nonempty = 0;
    bool family_ok = true;
    for (int sgm = 0; sgm < TAIL_SEGMENTS; ++sgm) {
      const int bin = TAIL_BINS[sgm];
      if (rp->bin_count[bin] == 0) continue;
      ++nonempty;
      if (bin < MAXNT && rp->bin_family[bin] != CTR_KFAM_GAUSS_TP) family_ok = false;
    }
    rp->tail_fused = throughput && p->ndim == 2 && !rp->lowpass && family_ok && nonempty >= 2;
    // What the tail launch takes of a bin, and whether the bin keeps a launch of its own.  Pairs:
    // every pair of the 64-lane tier -- the close ones with two tiers, all of them with one -- so
    // that launch is never queued.  (One tier is for fewer than 64 pairs or wide windows; a bin of
    // more than TAIL_PAIRS_WHOLE wide-window pairs is no work for TAIL_CAP wavefronts and keeps its
    // launch for all but the close ones, whatever the handle's setting.)  A block bin of at most
    // tail_absorb clusters: all of it; a larger one: the close clusters, the bin's launch fits the
    // others.
    for (int sgm = 0; sgm < TAIL_SEGMENTS; ++sgm) {
      const int64_t cnt = rp->bin_count[TAIL_BINS[sgm]];
      const bool whole = sgm == 0 ? !rp->pairs_split && cnt <= TAIL_PAIRS_WHOLE : cnt <= (int64_t)tail_absorb;
      rp->tail_whole[sgm] = rp->tail_fused && cnt > 0 && whole;
      rp->tail_own[sgm] = cnt > 0 && !(rp->tail_fused && (whole || (sgm == 0 && rp->pairs_split)));
    }
    // its grid: at most TAIL_CAP workgroups per segment, the segments in the order 1, 2, 0 (kargs.h)
    if (rp->tail_fused) {
      int32_t at = 0;
      for (int sgm : {1, 2, 0}) {
        const int bin = TAIL_BINS[sgm];
        rp->tail.ord_off[sgm] = (int32_t)rp->bin_begin[bin];
        rp->tail.whole[sgm] = rp->tail_whole[sgm] ? (int32_t)rp->bin_count[bin] : 0;
        rp->tail.grid_begin[sgm] = at;
        at += (int32_t)std::min<int64_t>(rp->bin_count[bin], TAIL_CAP);
      }
      rp->tail.grid_begin[TAIL_SEGMENTS] = rp->tail_grid = at;
    }
  }
  if (rp->bin_count[BIN_LARGE] > 0) {
    // a leader workgroup of 512 threads per cluster + helpers for its pixel passes
    // (large_kernel.h): as many as fill the machine, none when the clusters alone do.
    // (Several batches in flight fill the machine by themselves: a waiting helper would only hold
    //  the compute unit that another batch's leader needs.)
    const int64_t per_cluster = 512 / rp->bin_count[BIN_LARGE];
    rp->large_workgroups = throughput ? 1 : (int)(per_cluster < 1 ? 1 : (per_cluster > 8 ? 8 : per_cluster));
  }

  // ---- the launches ----
  // a launch of its whole bin: ungated, no counter, no split
  auto add = [&](int launch, int kind, int bin, long long grid, lane_sched::ChainClass cls, long long count, int nt) {
    rp->launches.push_back(LaunchSpec{launch, kind, bin, bin < 0 ? 0 : rp->bin_family[bin], bin < 0 ? 0 : rp->bin_slot[bin],
                                      grid, false, false, -1, false, 0, 0, cls, count, nt});
    return &rp->launches.back();
  };
  // block bins: NT 8 -> 1, then the constrained NT 2 -> 1
  for (int i = 0; i < MAXNT + 2; ++i) {
    const int bin = i < MAXNT ? MAXNT - 1 - i : (i == MAXNT ? BIN_CONS2 : BIN_CONS1);
    const int64_t cnt = rp->bin_count[bin];
    if (cnt == 0) continue;
    // (with a tail launch: a bin that it fits whole has no launch; of another, it takes the close
    // clusters, all of them, and the workgroups of those entries return at once)
    const bool in_tail = rp->tail_fused && (bin == TAIL_BINS[1] || bin == TAIL_BINS[2]);
    if (in_tail && !rp->tail_own[bin == TAIL_BINS[1] ? 1 : 2]) continue;
    LaunchSpec* s = add(bin, KIND_BLOCK, bin, cnt, lane_sched::CHAIN_BLOCK, cnt, bin < MAXNT ? bin + 1 : (bin == BIN_CONS2 ? 2 : 1));
    s->split = in_tail;
    s->split_cap = in_tail ? INT32_MAX : 0;
  }
  // the tail launch: ungated, it carries workgroups with much LDS like the block kernels
  if (rp->tail_fused)
    add(LAUNCH_TAIL, KIND_TAIL, -1, rp->tail_grid, lane_sched::CHAIN_TAIL, rp->tail_grid, 1)->counter = 4;
  if (rp->bin_count[BIN_LARGE] > 0)
    add(BIN_LARGE, KIND_LARGE, BIN_LARGE, rp->bin_count[BIN_LARGE] * rp->large_workgroups, lane_sched::CHAIN_LARGE,
        rp->bin_count[BIN_LARGE], 1);
  if (rp->bin_count[BIN_TOO_LARGE] > 0)
    add(BIN_TOO_LARGE, KIND_MARK, BIN_TOO_LARGE, (rp->bin_count[BIN_TOO_LARGE] + 255) / 256, lane_sched::CHAIN_MARK,
        rp->bin_count[BIN_TOO_LARGE], 1);
  // the small kernels start after the others, where there are others (gate)
  if (const int64_t cnt = rp->bin_count[BIN_SMALL2]) {
    if (rp->pairs_split) {
      // front_load_kernel has put the pairs closer than a quarter of the mask radius first and
      // counted them (on the device): the 64-lane tier is exactly those, the 16-lane kernel, a
      // chain of its own, takes the others -- which kernel fits a pair depends on the pair alone.
      // (delay_first: a little later still than the first tier, whose few wavefronts must not
      // queue up behind the thousands of this one)
      LaunchSpec* s = add(LAUNCH_PAIRS16, KIND_SMALL, BIN_SMALL2, std::min<int64_t>((cnt + 3) / 4, SMALL_MAX_GRID),
                          lane_sched::CHAIN_PAIRS16, cnt, 1);
      s->slot = SLOT_PAIRS16; s->gated = rp->gate; s->delay_first = true; s->counter = 3;
      s->split = true; s->split_part = 2;
    }
    // A tail launch fits every pair of the 64-lane tier -- the close ones with two tiers, all of
    // them with one: that tier has no launch of its own then.  (But for one tier of more than
    // TAIL_PAIRS_WHOLE pairs, wide windows: the launch takes all but the close ones.)
    if (rp->tail_own[0]) {
      LaunchSpec* s = add(BIN_SMALL2, KIND_SMALL, BIN_SMALL2, std::min<int64_t>(cnt, rp->pairs_split ? PAIRS64_TIER_GRID : SMALL_MAX_GRID),
                          lane_sched::CHAIN_PAIRS64, cnt, 1);   // (one wavefront per pair)
      s->gated = rp->gate; s->counter = 2;
      s->split = rp->pairs_split || rp->tail_fused;
      s->split_part = rp->pairs_split ? 1 : (rp->tail_fused ? 3 : 0);
      s->split_cap = rp->tail_fused ? INT32_MAX : 0;
    }
  }
  if (const int64_t cnt = rp->bin_count[BIN_SMALL1]) {
    const int64_t waves = rp->bin_slot[BIN_SMALL1] == SLOT_SINGLES64 ? cnt : (cnt + 7) / 8;
    LaunchSpec* s = add(BIN_SMALL1, KIND_SMALL, BIN_SMALL1, std::min(waves, SMALL_MAX_GRID), lane_sched::CHAIN_SINGLES, cnt, 1);
    s->gated = rp->gate; s->counter = 1;
  }

  order->assign((size_t)n_clusters, 0);
  {
    int64_t cursor[NBINS];
    for (int b = 0; b < NBINS; ++b) cursor[b] = rp->bin_begin[b];
    for (int64_t c = 0; c < n_clusters; ++c) (*order)[(size_t)cursor[(*bin_of)[(size_t)c]]++] = (int32_t)c;
    // inside a generic bin the clusters with the most features start first
    for (int b = 0; b < MAXNT; ++b)
      std::stable_sort(order->begin() + rp->bin_begin[b], order->begin() + rp->bin_begin[b + 1],
                       [&](int32_t x, int32_t y) {
                         return feat_offset[x + 1] - feat_offset[x] > feat_offset[y + 1] - feat_offset[y];
                       });
  }
  return nullptr;
}

}  // namespace refine_plan

#endif  // CTR_REFINE_PLAN_H
