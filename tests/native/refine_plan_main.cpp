// The launch decision of a refine plan (clustertracking_amd/csrc/refine_plan.h) without a device.
// Exits non-zero at the first property that does not hold (tests/test_refine_plan_host.py builds
// this with the address and undefined-behaviour sanitizers and runs it).  Nothing below calls the
// header's helpers or names its constants beyond the bin, slot and launch indices: the expected
// bins, flags and launches are restated here with literal numbers.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "refine_plan.h"

using namespace refine_plan;
using lane_sched::ChainClass;

static int g_failed = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (g_failed < 20) {                                 \
        std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                          \
        std::printf("\n");                                 \
      }                                                    \
      ++g_failed;                                          \
    }                                                      \
  } while (0)

// one case of the sweep
struct Case {
  bool throughput, lowpass, wide;
  int ndim;
  int32_t tail_absorb;
  int64_t singles, pairs, n3, n5, large, too_large;   // clusters of 1, 2, 3, 5, 65 and 2^22 features
  void print() const {
    std::printf("  [tp %d ndim %d lowpass %d wide %d absorb %d | singles %lld pairs %lld n3 %lld n5 %lld large %lld too_large %lld]\n",
                (int)throughput, ndim, (int)lowpass, (int)wide, (int)tail_absorb, (long long)singles, (long long)pairs,
                (long long)n3, (long long)n5, (long long)large, (long long)too_large);
  }
};

static const int FEATURES[6] = {1, 2, 3, 5, 65, 0x400000};

// gaussian, isotropic, the default parameter modes, no constraint
static ctr_problem problem_of(const Case& c) {
  ctr_problem p = {};
  p.ndim = c.ndim;
  p.isotropic = 1;
  p.fit_function = CTR_FIT_GAUSS;
  p.n_params = 2 + c.ndim + 1;
  p.modes[0] = CTR_MODE_CLUSTER;
  for (int k = 1; k < 2 + c.ndim; ++k) p.modes[k] = CTR_MODE_VAR;
  p.modes[2 + c.ndim] = CTR_MODE_CONST;
  // windows of 81 / 343 pixels (<= 600) and of 729 / 1331 (> 600)
  for (int a = 0; a < c.ndim; ++a) p.radius[a] = c.ndim == 2 ? (c.wide ? 13 : 4) : (c.wide ? 5 : 3);
  p.constraint_kind = CTR_CONS_NONE;
  p.max_iter = 10;
  p.solver_maxiter = 100;
  p.flags = (c.throughput ? CTR_FLAG_THROUGHPUT : 0) | (c.lowpass ? CTR_FLAG_WINDOW_FILTER : 0);
  p.residual_factor = 1e5;
  if (c.lowpass) p.noise_size[c.ndim - 1] = 1.;
  return p;
}

// Where a cluster of FEATURES[type] features goes in these problems.  1 + n (1 + ndim) variables,
// 16 columns (variables + 1) per tile: 3 features are 10 / 13 variables (NT 1), 5 are 16 / 21
// (NT 2).  Singles and pairs go to the small kernel, except with a lowpass, where they are 4-5 and
// 7-9 variables of the block kernel (NT 1).  65 features: the large kernel; 2^22: beyond the engine.
static int bin_of_type(const Case& c, int type) {
  switch (type) {
    case 0: return c.lowpass ? 0 : BIN_SMALL1;
    case 1: return c.lowpass ? 0 : BIN_SMALL2;
    case 2: return 0;
    case 3: return 1;
    case 4: return BIN_LARGE;
    default: return BIN_TOO_LARGE;
  }
}

static LaunchSpec spec(int launch, int kind, int bin, int family, int slot, long long grid, ChainClass cls, long long count, int nt) {
  return LaunchSpec{launch, kind, bin, family, slot, grid, false, false, -1, false, 0, 0, cls, count, nt};
}

// ---- (a) the flags, the tail segments and the launch list, restated ---------------------------
static void check_decision(const Case& c, const RefinePlan& rp) {
  const int before = g_failed;
  int64_t cnt[NBINS] = {0};
  const int64_t of_type[6] = {c.singles, c.pairs, c.n3, c.n5, c.large, c.too_large};
  for (int t = 0; t < 6; ++t) cnt[bin_of_type(c, t)] += of_type[t];
  const int64_t n1 = cnt[0], n2 = cnt[1], pairs = cnt[BIN_SMALL2], singles = cnt[BIN_SMALL1];
  const int block_family = c.lowpass ? CTR_KFAM_LOWPASS : (c.throughput && c.ndim == 2 ? CTR_KFAM_GAUSS_TP : CTR_KFAM_GAUSS);
  for (int b = 0; b < NBINS; ++b) {
    CHECK(rp.bin_count[b] == cnt[b], "bin %d: %lld clusters, expected %lld", b, (long long)rp.bin_count[b], (long long)cnt[b]);
    if (cnt[b] == 0) continue;
    const int family = b < 2 ? block_family : b == BIN_LARGE ? (c.lowpass ? CTR_KFAM_LARGE_LOWPASS : CTR_KFAM_LARGE)
                     : b == BIN_TOO_LARGE ? CTR_KFAM_NONE : CTR_KFAM_SMALL;
    const int slot = b < 2 ? b : b == BIN_SMALL1 ? (c.wide ? SLOT_SINGLES64 : SLOT_SINGLES8) : b == BIN_SMALL2 ? SLOT_PAIRS64 : 0;
    CHECK(rp.bin_family[b] == family && rp.bin_slot[b] == slot, "bin %d: family %d slot %d", b, rp.bin_family[b], rp.bin_slot[b]);
  }
  const bool gate = n1 + n2 + cnt[BIN_LARGE] > 0;
  const bool pairs_split = c.throughput && pairs >= 64 && !c.wide;
  const bool fused = c.throughput && c.ndim == 2 && !c.lowpass && (pairs > 0) + (n1 > 0) + (n2 > 0) >= 2;
  const bool pairs_whole = fused && pairs > 0 && !pairs_split && pairs <= 2048;
  const bool whole1 = fused && n1 > 0 && n1 <= c.tail_absorb, whole2 = fused && n2 > 0 && n2 <= c.tail_absorb;
  const bool own[3] = {pairs > 0 && !(fused && (pairs_split || pairs_whole)), n1 > 0 && !whole1, n2 > 0 && !whole2};
  const bool whole[3] = {pairs_whole, whole1, whole2};
  CHECK(rp.lowpass == c.lowpass && rp.gate == gate && rp.pairs_split == pairs_split && rp.tail_fused == fused,
        "lowpass %d gate %d pairs_split %d tail_fused %d", (int)rp.lowpass, (int)rp.gate, (int)rp.pairs_split, (int)rp.tail_fused);
  for (int s = 0; s < 3; ++s)
    CHECK(rp.tail_whole[s] == whole[s] && rp.tail_own[s] == own[s], "segment %d: whole %d own %d", s, (int)rp.tail_whole[s], (int)rp.tail_own[s]);
  // the tail launch: at most 256 workgroups per bin, in the grid order NT 1, NT 2, pairs
  const int64_t g1 = std::min<int64_t>(n1, 256), g2 = std::min<int64_t>(n2, 256), g0 = std::min<int64_t>(pairs, 256);
  const int64_t tail_grid = fused ? g1 + g2 + g0 : 0;
  CHECK(rp.tail_grid == tail_grid, "tail grid %d, expected %lld", rp.tail_grid, (long long)tail_grid);
  if (fused) {
    const int64_t begin[4] = {g1 + g2, 0, g1, g1 + g2 + g0};   // by segment: pairs, NT 1, NT 2, the end
    const int64_t off[3] = {n1 + n2 + cnt[BIN_TOO_LARGE] + singles, 0, n1};   // bins 0..7, too large, singles, pairs
    const int64_t full[3] = {pairs, n1, n2};
    for (int s = 0; s < 3; ++s)
      CHECK(rp.tail.grid_begin[s] == begin[s] && rp.tail.ord_off[s] == off[s] && rp.tail.whole[s] == (whole[s] ? full[s] : 0),
            "segment %d: grid_begin %d ord_off %d whole %d", s, rp.tail.grid_begin[s], rp.tail.ord_off[s], rp.tail.whole[s]);
    CHECK(rp.tail.grid_begin[3] == begin[3], "grid end %d", rp.tail.grid_begin[3]);
  }
  const int large_workgroups = cnt[BIN_LARGE] == 0 ? 0 : c.throughput ? 1 : 8;   // (512 / 1 cluster, at most 8)
  CHECK(rp.large_workgroups == large_workgroups, "large workgroups %d", rp.large_workgroups);

  // the launches, in chain order: block NT 2, NT 1, tail, large, too large, pairs 16, pairs 64, singles
  std::vector<LaunchSpec> want;
  for (int b = 1; b >= 0; --b) {
    if (cnt[b] == 0 || (fused && !own[b + 1])) continue;
    LaunchSpec s = spec(b, KIND_BLOCK, b, block_family, b, cnt[b], lane_sched::CHAIN_BLOCK, cnt[b], b + 1);
    if (fused) { s.split = true; s.split_cap = INT32_MAX; }
    want.push_back(s);
  }
  if (fused) {
    LaunchSpec s = spec(LAUNCH_TAIL, KIND_TAIL, -1, 0, 0, tail_grid, lane_sched::CHAIN_TAIL, tail_grid, 1);
    s.counter = 4;
    want.push_back(s);
  }
  if (cnt[BIN_LARGE] > 0)
    want.push_back(spec(BIN_LARGE, KIND_LARGE, BIN_LARGE, c.lowpass ? CTR_KFAM_LARGE_LOWPASS : CTR_KFAM_LARGE, 0,
                        cnt[BIN_LARGE] * large_workgroups, lane_sched::CHAIN_LARGE, cnt[BIN_LARGE], 1));
  if (cnt[BIN_TOO_LARGE] > 0)
    want.push_back(spec(BIN_TOO_LARGE, KIND_MARK, BIN_TOO_LARGE, CTR_KFAM_NONE, 0, (cnt[BIN_TOO_LARGE] + 255) / 256,
                        lane_sched::CHAIN_MARK, cnt[BIN_TOO_LARGE], 1));
  if (pairs > 0) {
    // the table of the pairs: (fused, split, few) -> launches
    LaunchSpec p16 = spec(LAUNCH_PAIRS16, KIND_SMALL, BIN_SMALL2, CTR_KFAM_SMALL, SLOT_PAIRS16, std::min<int64_t>((pairs + 3) / 4, 8192),
                          lane_sched::CHAIN_PAIRS16, pairs, 1);
    p16.gated = gate; p16.delay_first = true; p16.counter = 3; p16.split = true; p16.split_part = 2; p16.split_cap = 0;
    LaunchSpec p64 = spec(BIN_SMALL2, KIND_SMALL, BIN_SMALL2, CTR_KFAM_SMALL, SLOT_PAIRS64, std::min<int64_t>(pairs, 8192),
                          lane_sched::CHAIN_PAIRS64, pairs, 1);
    p64.gated = gate; p64.counter = 2;
    if (!fused && !pairs_split) want.push_back(p64);                    // no split, part 0, cap 0
    else if (!fused && pairs_split) {
      want.push_back(p16);
      p64.split = true; p64.split_part = 1; p64.split_cap = 0; p64.grid = std::min<int64_t>(pairs, 2048);
      want.push_back(p64);
    }
    else if (pairs_split) want.push_back(p16);                          // the tail takes the close pairs
    else if (pairs > 2048) {
      p64.split = true; p64.split_part = 3; p64.split_cap = INT32_MAX;
      want.push_back(p64);
    }                                                                   // else: the tail fits the bin whole
  }
  if (singles > 0) {
    LaunchSpec s = spec(BIN_SMALL1, KIND_SMALL, BIN_SMALL1, CTR_KFAM_SMALL, c.wide ? SLOT_SINGLES64 : SLOT_SINGLES8,
                        std::min<int64_t>(c.wide ? singles : (singles + 7) / 8, 8192), lane_sched::CHAIN_SINGLES, singles, 1);
    s.gated = gate; s.counter = 1;
    want.push_back(s);
  }
  CHECK(rp.launches.size() == want.size(), "%zu launches, expected %zu", rp.launches.size(), want.size());
  for (size_t i = 0; i < std::min(rp.launches.size(), want.size()); ++i) {
    const LaunchSpec &g = rp.launches[i], &w = want[i];
    CHECK(g.launch == w.launch && g.kind == w.kind && g.bin == w.bin, "launch %zu: launch %d kind %d bin %d, expected %d %d %d", i,
          g.launch, g.kind, g.bin, w.launch, w.kind, w.bin);
    CHECK(g.family == w.family && g.slot == w.slot, "launch %zu (%d): family %d slot %d, expected %d %d", i, w.launch, g.family, g.slot, w.family, w.slot);
    CHECK(g.grid == w.grid, "launch %zu (%d): grid %lld, expected %lld", i, w.launch, g.grid, w.grid);
    CHECK(g.gated == w.gated && g.delay_first == w.delay_first && g.counter == w.counter, "launch %zu (%d): gated %d delay %d counter %d", i,
          w.launch, (int)g.gated, (int)g.delay_first, g.counter);
    CHECK(g.split == w.split && g.split_part == w.split_part && g.split_cap == w.split_cap, "launch %zu (%d): split %d part %d cap %d, expected %d %d %d",
          i, w.launch, (int)g.split, g.split_part, g.split_cap, (int)w.split, w.split_part, w.split_cap);
    CHECK(g.cls == w.cls && g.count == w.count && g.nt == w.nt, "launch %zu (%d): class %d count %lld nt %d", i, w.launch, (int)g.cls, g.count, g.nt);
  }
  if (g_failed != before) c.print();
}

// ---- (b) the launches that read a bin fit each of its clusters exactly once --------------------
// The entries [lo, hi) of its bin that a launch takes, for `first` close clusters counted on the
// device (kargs.h: KArgs::split*): all of the bin without a split; else, with skip = min(first,
// split_cap): a block launch [skip, n), a small launch part 1 [skip, first), part 2 [first, n),
// part 3 [skip, n).  A tail segment with workgroups (kargs.h: TailArgs): [0, whole) where whole is
// positive, else [0, first).
static void check_partition(const Case& c, const RefinePlan& rp) {
  const int before = g_failed;
  for (int b = 0; b < NBINS; ++b) {
    const int64_t n = rp.bin_count[b];
    if (n == 0) continue;
    for (int64_t first : {(int64_t)0, std::min<int64_t>(1, n), n - 1, n}) {
      std::vector<std::pair<int64_t, int64_t>> parts;
      for (const LaunchSpec& s : rp.launches) {
        if (s.kind == KIND_TAIL || s.bin != b) continue;
        int64_t lo = 0, hi = n;
        if (s.split) {
          const int64_t skip = std::min<int64_t>(first, s.split_cap);
          if (s.kind == KIND_BLOCK || (s.kind == KIND_SMALL && s.split_part == 3)) lo = skip;
          else if (s.kind == KIND_SMALL && s.split_part == 1) { lo = skip; hi = first; }
          else if (s.kind == KIND_SMALL && s.split_part == 2) lo = first;
          else CHECK(false, "bin %d: a split launch of kind %d, part %d", b, s.kind, s.split_part);
        }
        parts.push_back({lo, hi});
      }
      if (rp.tail_fused)
        for (int sgm = 0; sgm < 3; ++sgm) {
          if (b != (sgm == 0 ? BIN_SMALL2 : sgm - 1)) continue;
          const int next = sgm == 1 ? 2 : sgm == 2 ? 0 : 3;   // (the grid holds the segments in the order 1, 2, 0)
          const int64_t workgroups = rp.tail.grid_begin[next] - rp.tail.grid_begin[sgm];
          CHECK(workgroups >= 0 && workgroups <= 256, "segment %d: %lld workgroups", sgm, (long long)workgroups);
          CHECK(rp.tail.ord_off[sgm] == rp.bin_begin[b], "segment %d begins at %d, its bin at %lld", sgm, rp.tail.ord_off[sgm], (long long)rp.bin_begin[b]);
          if (workgroups > 0) parts.push_back({0, rp.tail.whole[sgm] > 0 ? rp.tail.whole[sgm] : first});
        }
      std::sort(parts.begin(), parts.end());
      int64_t at = 0;
      for (const auto& part : parts) {
        CHECK(part.first <= part.second, "bin %d, %lld close: entries [%lld, %lld)", b, (long long)first, (long long)part.first, (long long)part.second);
        if (part.first == part.second) continue;
        CHECK(part.first == at, "bin %d, %lld close: entries [%lld, %lld) after %lld", b, (long long)first, (long long)part.first, (long long)part.second, (long long)at);
        at = std::max(at, part.second);
      }
      CHECK(at == n, "bin %d of %lld, %lld close: fitted up to %lld", b, (long long)n, (long long)first, (long long)at);
    }
  }
  if (g_failed != before) c.print();
}

// ---- (c) the order of the clusters -------------------------------------------------------------
static void check_order(const Case& c, const RefinePlan& rp, const std::vector<int32_t>& feat_offset,
                        const std::vector<int32_t>& type_of, const std::vector<int32_t>& order, const std::vector<int32_t>& bin_of) {
  const int before = g_failed;
  const size_t n = type_of.size();
  CHECK(order.size() == n && bin_of.size() == n, "sizes %zu %zu of %zu", order.size(), bin_of.size(), n);
  if (order.size() != n || bin_of.size() != n) return;
  CHECK(rp.bin_begin[0] == 0, "the first bin begins at %lld", (long long)rp.bin_begin[0]);
  for (int b = 0; b < NBINS; ++b)
    CHECK(rp.bin_begin[b + 1] == rp.bin_begin[b] + rp.bin_count[b], "bin %d: begin %lld count %lld next %lld", b,
          (long long)rp.bin_begin[b], (long long)rp.bin_count[b], (long long)rp.bin_begin[b + 1]);
  CHECK(rp.bin_begin[NBINS] == (int64_t)n, "the bins hold %lld of %zu clusters", (long long)rp.bin_begin[NBINS], n);
  if (g_failed != before) { c.print(); return; }
  std::vector<char> seen(n, 0);
  int64_t bad = 0;
  for (int b = 0; b < NBINS; ++b)
    for (int64_t i = rp.bin_begin[b]; i < rp.bin_begin[b + 1]; ++i) {
      const int32_t id = order[(size_t)i];
      if (id < 0 || (size_t)id >= n || seen[(size_t)id]) { ++bad; continue; }
      seen[(size_t)id] = 1;
      if (bin_of[(size_t)id] != b || bin_of_type(c, type_of[(size_t)id]) != b) ++bad;   // each bin contiguous
      if (i == rp.bin_begin[b]) continue;
      const int32_t prev = order[(size_t)i - 1];
      if (prev < 0 || (size_t)prev >= n) continue;
      const int32_t f = feat_offset[(size_t)id + 1] - feat_offset[(size_t)id], fp = feat_offset[(size_t)prev + 1] - feat_offset[(size_t)prev];
      // a block bin: by descending feature count, stably; every other bin: as given
      if (b < MAXNT ? !(fp > f || (fp == f && prev < id)) : !(prev < id)) ++bad;
    }
  CHECK(bad == 0, "%lld entries of the order are wrong", (long long)bad);
  if (g_failed != before) c.print();
}

int main() {
  long long cases = 0;
  std::vector<int32_t> feat_offset, type_of, order, bin_of;
  for (int32_t absorb : {0, 5, (int32_t)(32 * 256)}) {
    CHECK(absorb != 32 * 256 || absorb == TAIL_ABSORB, "the default of ctr_set_tail_absorb is %d", TAIL_ABSORB);
    std::vector<int64_t> block_counts = {0, 1, absorb, (int64_t)absorb + 1};
    std::sort(block_counts.begin(), block_counts.end());
    block_counts.erase(std::unique(block_counts.begin(), block_counts.end()), block_counts.end());
    for (int64_t pairs : {0, 1, 63, 64, 2048, 2049})
      for (int64_t n3 : block_counts)
        for (int64_t n5 : block_counts)
          for (int64_t singles : {0, 1, 9})
            for (int large = 0; large < 2; ++large)
              for (int too_large = 0; too_large < 2; ++too_large) {
                // the clusters of the six kinds, interleaved
                int64_t left[6] = {singles, pairs, n3, n5, large, too_large};
                feat_offset.assign(1, 0);
                type_of.clear();
                for (bool any = true; any;) {
                  any = false;
                  for (int t = 0; t < 6; ++t) {
                    if (left[t] == 0) continue;
                    --left[t];
                    any = true;
                    type_of.push_back(t);
                    feat_offset.push_back(feat_offset.back() + FEATURES[t]);
                  }
                }
                for (int flags = 0; flags < 16; ++flags) {
                  const Case c = {(flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) ? 3 : 2, absorb,
                                  singles, pairs, n3, n5, large, too_large};
                  // Tables of thousands of clusters (the default tail_absorb) cost milliseconds each:
                  // they are swept with the singles, the large and the too-large cluster all absent or
                  // all present (none of them is in a rule with tail_absorb).  A bin's count meets
                  // tail_absorb only where a tail launch is possible -- throughput, 2D, no lowpass:
                  // those problems get every count of pairs.  For the others a big bin is a grid, an
                  // order and the gate: no pairs or the most.
                  const bool big = n3 > 64 || n5 > 64, may_fuse = c.throughput && c.ndim == 2 && !c.lowpass;
                  const bool corner = (singles == 0 && !large && !too_large) || (singles == 9 && large && too_large);
                  if (big && !(corner && (may_fuse || pairs == 0 || pairs == 2049))) continue;
                  const ctr_problem p = problem_of(c);
                  RefinePlan rp;
                  const char* why = make_plan(&p, (int64_t)type_of.size(), feat_offset.data(), absorb, &rp, &order, &bin_of);
                  CHECK(why == nullptr, "make_plan: %s", why);
                  if (why) { c.print(); continue; }
                  check_decision(c, rp);
                  check_partition(c, rp);
                  check_order(c, rp, feat_offset, type_of, order, bin_of);
                  ++cases;
                }
              }
  }
  {
    // the failure that the table of a caller can cause
    const Case c = {false, false, false, 2, 0, 0, 0, 0, 0, 0, 0};
    const ctr_problem p = problem_of(c);
    const int32_t down[3] = {0, 2, 1};
    RefinePlan rp;
    const char* why = make_plan(&p, 2, down, 0, &rp, &order, &bin_of);
    CHECK(why != nullptr && std::string(why) == "feat_offset must be non-decreasing", "a decreasing feat_offset: %s", why ? why : "(accepted)");
  }
  if (g_failed) {
    std::printf("refine_plan: %d check(s) FAILED\n", g_failed);
    return 1;
  }
  std::printf("refine_plan: ok (%lld plans)\n", cases);
  return 0;
}
