// lane_sched.h -- where the chains of a ctr_refine_batch_device call go.
//
// A lane is one in-order stream of the library, one per hardware queue, shared by every handle of
// a device.  A call is a head chain, one chain per kernel launch of a bin and a finish chain; the
// policy here decides the lane of each, longest first onto the least-loaded lane (LPT list
// scheduling), and keeps the books: what is still pending on every lane, and how long a launch
// took the last time it was measured.  Host code only and no HIP type: an event is an opaque id
// with a completion callback (ctrefine.hip supplies hipEventQuery), so that the policy is tested
// without a device (tests/native/lane_sched_main.cpp).
#ifndef CTR_LANE_SCHED_H
#define CTR_LANE_SCHED_H

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <deque>
#include <vector>

namespace lane_sched {

constexpr int MAX_LANES = 32, DEFAULT_LANES = 4;   // (4: HIP's default of GPU_MAX_HW_QUEUES)

// lanes of a pool from the text of GPU_MAX_HW_QUEUES (null: not set): its integer within
// 1..MAX_LANES, DEFAULT_LANES where there is none
inline int lanes_from_env(const char* text) {
  if (!text || !*text) return DEFAULT_LANES;
  char* end = nullptr;
  const long v = std::strtol(text, &end, 10);
  if (end == text) return DEFAULT_LANES;
  return (int)std::min<long>(std::max<long>(v, 1), MAX_LANES);
}

// ---- estimates ---------------------------------------------------------------------------------
// what a chain runs: the guess of its duration before it has been measured depends on it
enum ChainClass { CHAIN_HEAD, CHAIN_FINISH, CHAIN_SINGLES, CHAIN_PAIRS64, CHAIN_PAIRS16, CHAIN_BLOCK, CHAIN_LARGE, CHAIN_MARK, CHAIN_TAIL };

// milliseconds of a launch of `count` clusters, before its first measurement.  A bin lasts as long
// as its slowest fit (the constant) plus its share of the machine (the slope); the orders of
// magnitude of cfg 2 with ten batches in flight (profiles/r03_kernel_stats*.csv).  nt: 16-column
// tiles of the block kernel's normal matrix.
inline double static_guess(ChainClass cls, long long count, int nt = 1) {
  const double n = (double)std::max<long long>(count, 0);
  switch (cls) {
    case CHAIN_HEAD: return 0.05;
    case CHAIN_FINISH: return 0.01;
    case CHAIN_SINGLES: return 0.05 + 1.5e-5 * n;
    case CHAIN_PAIRS64: return 0.3 + 2e-4 * n;
    case CHAIN_PAIRS16: return 0.05 + 6e-5 * n;
    case CHAIN_BLOCK: return (0.3 + 1e-3 * n) * std::max(nt, 1);
    case CHAIN_LARGE: return 2. + 1. * n;
    case CHAIN_MARK: return 0.01;
    // (the tail launch lasts as long as the slowest fit of the call, 3 ms in cfg 2: by this guess it
    // is placed before the bins it was taken from, as it is once it has been measured)
    case CHAIN_TAIL: return 3. + 2e-3 * n;
  }
  return 0.01;
}

// the duration of one launch of a plan: the guess until a reading arrives, then the last valid
// reading (a failed, zero, negative or non-finite one is ignored)
struct Estimate {
  double guess = 0.01, measured = 0.;
  bool has_reading = false;
  double value() const { return has_reading ? measured : guess; }
  void update(double ms) {
    if (std::isfinite(ms) && ms > 0.) { measured = ms; has_reading = true; }
  }
};

// ---- the lanes' books --------------------------------------------------------------------------
typedef void* EventId;
typedef bool (*EventDone)(void* ctx, EventId ev);   // has the event completed?  never blocks

struct Ticket { EventId done; double ms; };

class Pool {
 public:
  explicit Pool(int n_lanes) : pending_((size_t)std::min(std::max(n_lanes, 1), MAX_LANES)), limit_((int)pending_.size()) {}

  int size() const { return (int)pending_.size(); }
  int limit() const { return limit_; }   // lanes that placement uses: the first limit()
  // n in 1..size(), or 0 for all; returns the limit before, -1 (nothing changes) out of range
  int set_limit(int n) {
    if (n < 0 || n > size()) return -1;
    const int before = limit_;
    limit_ = n ? n : size();
    return before;
  }

  // estimated milliseconds enqueued on the lane and not known to have completed
  double load(int lane) const {
    double s = 0.;
    for (const Ticket& t : pending_[(size_t)lane]) s += t.ms;
    return s;
  }
  size_t tickets(int lane) const { return pending_[(size_t)lane].size(); }

  // a chain was enqueued on the lane; `done` is recorded at its end
  void push(int lane, EventId done, double ms) { pending_[(size_t)lane].push_back(Ticket{done, ms > 0. ? ms : 0.}); }

  // drops the tickets whose event has completed, from the front of every lane only (a lane is in
  // order: a ticket behind a pending one stays, whatever its event says); their events go to
  // *retired (may be null), to be recorded again
  void retire(EventDone done, void* ctx, std::vector<EventId>* retired = nullptr) {
    for (auto& q : pending_)
      while (!q.empty() && done(ctx, q.front().done)) {
        if (retired) retired->push_back(q.front().done);
        q.pop_front();
      }
  }

  int least_loaded(const std::vector<double>& load) const {
    int best = 0;
    for (int l = 1; l < limit_; ++l)
      if (load[(size_t)l] < load[(size_t)best]) best = l;
    return best;
  }

  // The lanes of a call.  head_ms < 0: head and finish run on the caller's stream (lane -1), only
  // the bins are placed.  order: the bins by descending estimate (ties: the first given first);
  // that is the order in which they are placed and must be enqueued.  The finish chain takes the
  // lane of the bin with the largest estimate (the head's where there is no bin): its wait for
  // that chain costs the lane nothing.
  struct Placement {
    int head = -1, finish = -1;
    std::vector<int> lane, order;
  };
  Placement place(double head_ms, const std::vector<double>& bin_ms) const {
    Placement p;
    std::vector<double> load((size_t)size());
    for (int l = 0; l < size(); ++l) load[(size_t)l] = this->load(l);
    if (head_ms >= 0.) {
      p.head = least_loaded(load);
      load[(size_t)p.head] += head_ms;
    }
    p.order.resize(bin_ms.size());
    for (size_t i = 0; i < bin_ms.size(); ++i) p.order[i] = (int)i;
    std::stable_sort(p.order.begin(), p.order.end(), [&](int a, int b) { return bin_ms[(size_t)a] > bin_ms[(size_t)b]; });
    p.lane.assign(bin_ms.size(), 0);
    for (int i : p.order) {
      const int l = least_loaded(load);
      p.lane[(size_t)i] = l;
      load[(size_t)l] += bin_ms[(size_t)i] > 0. ? bin_ms[(size_t)i] : 0.;
    }
    if (head_ms >= 0.) p.finish = p.order.empty() ? p.head : p.lane[(size_t)p.order[0]];
    return p;
  }

 private:
  std::vector<std::deque<Ticket>> pending_;
  int limit_;
};

}  // namespace lane_sched

#endif  // CTR_LANE_SCHED_H
