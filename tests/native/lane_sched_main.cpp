// The placement policy and the books of the lanes (clustertracking_amd/csrc/lane_sched.h) without
// a device: events are integers, "completed" is a set.  Exits non-zero at the first property that
// does not hold (tests/test_lane_sched_host.py builds this with the address and undefined-behaviour
// sanitizers and runs it).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <set>
#include <vector>

#include "lane_sched.h"

using lane_sched::Pool;

static int g_failed = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
      ++g_failed;                                          \
    }                                                      \
  } while (0)

static bool in_set(void* ctx, lane_sched::EventId ev) { return ((std::set<intptr_t>*)ctx)->count((intptr_t)ev) != 0; }
static lane_sched::EventId id(intptr_t i) { return (lane_sched::EventId)i; }

// the least makespan of the jobs on L machines: every assignment (symmetric ones cut: a job opens
// at most one new machine)
static double optimum(const std::vector<double>& jobs, int L) {
  std::vector<double> load((size_t)L, 0.);
  double best = std::numeric_limits<double>::infinity();
  struct Rec {
    const std::vector<double>& jobs; std::vector<double>& load; double& best; int L;
    void go(size_t i, int used) {
      double mk = 0.;
      for (double x : load) mk = std::max(mk, x);
      if (mk >= best) return;
      if (i == jobs.size()) { best = mk; return; }
      for (int l = 0; l < std::min(used + 1, L); ++l) {
        load[(size_t)l] += jobs[i];
        go(i + 1, std::max(used, l + 1));
        load[(size_t)l] -= jobs[i];
      }
    }
  } rec{jobs, load, best, L};
  rec.go(0, 0);
  return best;
}

static double makespan(const Pool::Placement& p, const std::vector<double>& jobs, int L) {
  std::vector<double> load((size_t)L, 0.);
  for (size_t i = 0; i < jobs.size(); ++i) load[(size_t)p.lane[i]] += jobs[i];
  double mk = 0.;
  for (double x : load) mk = std::max(mk, x);
  return mk;
}

// 1, 2, 3: every multiset of at most 7 durations from {1, 2, 3, 5, 8, 13}, L = 1..4
static void test_lpt() {
  const double values[] = {1, 2, 3, 5, 8, 13};
  long cases = 0;
  std::vector<double> jobs;
  struct Rec {
    const double* values; std::vector<double>& jobs; long& cases;
    void check() {
      for (int L = 1; L <= 4; ++L) {
        Pool pool(L);
        // (the bins alone, as on a caller's stream, so that the makespan is theirs; then with a head)
        const Pool::Placement p = pool.place(-1., jobs);
        CHECK(p.head == -1 && p.finish == -1, "caller's stream: head and finish are not placed");
        CHECK(p.lane.size() == jobs.size() && p.order.size() == jobs.size(), "sizes");
        for (size_t i = 0; i < jobs.size(); ++i) CHECK(p.lane[i] >= 0 && p.lane[i] < L, "lane %d of %d", p.lane[i], L);
        for (size_t i = 1; i < p.order.size(); ++i)
          CHECK(jobs[(size_t)p.order[i - 1]] >= jobs[(size_t)p.order[i]], "order is not longest first");
        if (!jobs.empty()) {
          const double opt = optimum(jobs, L), mk = makespan(p, jobs, L);
          const double bound = (4. / 3. - 1. / (3. * L)) * opt;
          CHECK(mk <= bound + 1e-12, "L %d: makespan %g, optimum %g, bound %g", L, mk, opt, bound);
        }
        if (L == 1)
          for (int l : p.lane) CHECK(l == 0, "L = 1: lane %d", l);
        const Pool::Placement q = pool.place(0.5, jobs);
        CHECK(q.head >= 0 && q.head < L, "head lane %d", q.head);
        if (L == 1) CHECK(q.head == 0 && q.finish == 0, "L = 1: head %d finish %d", q.head, q.finish);
        if (jobs.empty()) CHECK(q.finish == q.head, "no bin: the finish chain follows the head");
        else {
          size_t longest = 0;
          for (size_t i = 1; i < jobs.size(); ++i)
            if (jobs[i] > jobs[longest]) longest = i;
          CHECK(jobs[(size_t)q.order[0]] == jobs[longest], "order[0] is not a longest bin");
          CHECK(q.finish == q.lane[(size_t)q.order[0]], "finish on lane %d, longest bin on %d", q.finish, q.lane[(size_t)q.order[0]]);
        }
        ++cases;
      }
    }
    void go(int first, int left) {
      check();
      if (!left) return;
      for (int v = first; v < 6; ++v) {
        jobs.push_back(values[v]);
        go(v, left - 1);
        jobs.pop_back();
      }
    }
  } rec{values, jobs, cases};
  rec.go(0, 7);
  CHECK(cases == 4 * 1716, "%ld cases", cases);   // C(6 + 7, 7) multisets of at most 7 out of 6
  // the placement counts what is pending: a loaded lane is avoided
  Pool pool(3);
  pool.push(0, id(1), 10.);
  pool.push(1, id(2), 4.);
  const Pool::Placement p = pool.place(-1., {3., 2., 2.});
  CHECK(p.lane[0] == 2 && p.lane[1] == 2 && p.lane[2] == 1, "pending load: lanes %d %d %d", p.lane[0], p.lane[1], p.lane[2]);
}

// 4: completions in every order that respects lane order
enum { L = 3, per_lane = 3 };
static void test_books() {
  // completion orders: all interleavings of the three lanes' sequences
  std::vector<int> seq;
  long orders = 0;
  struct Rec {
    std::vector<int>& seq; long& orders;
    void run() {
      Pool pool(L);
      std::set<intptr_t> completed;
      double total = 0.;
      for (int l = 0; l < L; ++l)
        for (int j = 0; j < per_lane; ++j) { pool.push(l, id(100 * l + j + 1), 0.1 * (j + 1) + l); total += 0.1 * (j + 1) + l; }
      std::vector<int> next((size_t)L, 0);
      for (int l : seq) {
        // out of lane order first: the LAST ticket of the lane completes; nothing may retire for it
        const intptr_t last = 100 * l + per_lane;
        const bool early = next[(size_t)l] < per_lane - 1;
        if (early) {
          std::set<intptr_t> peek = completed;
          peek.insert(last);
          Pool copy = pool;
          std::vector<lane_sched::EventId> gone;
          copy.retire(in_set, &peek, &gone);
          CHECK(gone.empty(), "a ticket behind a pending one retired");
        }
        const size_t before = pool.tickets(l);
        const double load_before = pool.load(l);
        completed.insert(100 * l + next[(size_t)l] + 1);
        std::vector<lane_sched::EventId> gone;
        pool.retire(in_set, &completed, &gone);
        CHECK(gone.size() == 1 && (intptr_t)gone[0] == 100 * l + next[(size_t)l] + 1, "retired %zu", gone.size());
        CHECK(pool.tickets(l) == before - 1, "tickets");
        CHECK(pool.load(l) < load_before && pool.load(l) >= 0., "load %g -> %g", load_before, pool.load(l));
        next[(size_t)l]++;
        for (int m = 0; m < L; ++m) CHECK(pool.load(m) >= 0., "negative load");
      }
      for (int m = 0; m < L; ++m) CHECK(pool.load(m) == 0. && pool.tickets(m) == 0, "lane %d: load %g", m, pool.load(m));
      (void)total;
      ++orders;
    }
    void go(std::vector<int>& left) {
      bool any = false;
      for (int l = 0; l < L; ++l)
        if (left[(size_t)l]) {
          any = true;
          left[(size_t)l]--; seq.push_back(l);
          go(left);
          seq.pop_back(); left[(size_t)l]++;
        }
      if (!any) run();
    }
  } rec{seq, orders};
  std::vector<int> left((size_t)L, per_lane);
  rec.go(left);
  CHECK(orders == 1680, "%ld orders", orders);   // 9! / (3! 3! 3!)
  // several completions seen at once retire together, in lane order
  Pool pool(2);
  pool.push(0, id(1), 1.); pool.push(0, id(2), 2.); pool.push(0, id(3), 4.);
  std::set<intptr_t> completed = {1, 2};
  std::vector<lane_sched::EventId> gone;
  pool.retire(in_set, &completed, &gone);
  CHECK(gone.size() == 2 && gone[0] == id(1) && gone[1] == id(2) && pool.load(0) == 4., "batch retire");
  // a negative or non-finite estimate never makes a load negative
  pool.push(1, id(9), -3.);
  CHECK(pool.load(1) == 0., "negative estimate booked as %g", pool.load(1));
}

// 5: the estimate of a launch
static void test_estimate() {
  lane_sched::Estimate e;
  e.guess = lane_sched::static_guess(lane_sched::CHAIN_PAIRS64, 95);
  CHECK(e.guess > 0. && std::isfinite(e.guess), "guess %g", e.guess);
  CHECK(e.value() == e.guess, "before a reading: %g", e.value());
  const double bad[] = {0., -1., std::nan(""), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
  for (double x : bad) { e.update(x); CHECK(e.value() == e.guess, "reading %g taken", x); }
  e.update(1.25);
  CHECK(e.value() == 1.25, "first reading: %g", e.value());
  for (double x : bad) { e.update(x); CHECK(e.value() == 1.25, "reading %g taken", x); }
  e.update(0.5);
  CHECK(e.value() == 0.5, "last reading: %g", e.value());
  e.guess = 7.;   // (the guess is set again at every call: it must not come back)
  CHECK(e.value() == 0.5, "guess after a reading: %g", e.value());
  // every class has a positive finite guess that does not fall with the count
  for (int cls = lane_sched::CHAIN_HEAD; cls <= lane_sched::CHAIN_MARK; ++cls)
    for (int nt = 1; nt <= 8; ++nt) {
      const double a = lane_sched::static_guess((lane_sched::ChainClass)cls, 10, nt),
                   b = lane_sched::static_guess((lane_sched::ChainClass)cls, 100000, nt);
      CHECK(a > 0. && std::isfinite(a) && b >= a && std::isfinite(b), "class %d: %g %g", cls, a, b);
    }
  CHECK(lane_sched::static_guess(lane_sched::CHAIN_SINGLES, -5) > 0., "negative count");
}

// 6: the lane limit; and the lanes of a pool
static void test_limit() {
  Pool pool(4);
  CHECK(pool.size() == 4 && pool.limit() == 4, "new pool");
  CHECK(pool.set_limit(5) == -1 && pool.set_limit(-1) == -1 && pool.limit() == 4, "out of range");
  CHECK(pool.set_limit(2) == 4 && pool.limit() == 2, "limit 2");
  const std::vector<double> jobs = {5, 4, 3, 2, 1, 1, 1};
  Pool::Placement p = pool.place(0.1, jobs);
  for (int l : p.lane) CHECK(l < 2, "limit 2: lane %d", l);
  CHECK(p.head < 2 && p.finish < 2, "limit 2: head %d finish %d", p.head, p.finish);
  // (work pending beyond the limit stays in the books and retires as before)
  pool.push(3, id(7), 2.);
  CHECK(pool.set_limit(1) == 2, "limit 1");
  p = pool.place(0.1, jobs);
  for (int l : p.lane) CHECK(l == 0, "limit 1: lane %d", l);
  CHECK(pool.load(3) == 2., "pending beyond the limit");
  CHECK(pool.set_limit(0) == 1 && pool.limit() == 4, "0 restores all");
  std::set<intptr_t> completed = {7};
  pool.retire(in_set, &completed);
  CHECK(pool.load(3) == 0., "retired beyond the limit");
  p = pool.place(-1., {1, 1, 1, 1});
  std::set<int> lanes(p.lane.begin(), p.lane.end());
  CHECK(lanes.size() == 4, "all lanes again: %zu", lanes.size());
  CHECK(Pool(0).size() == 1 && Pool(100).size() == lane_sched::MAX_LANES, "pool sizes are clamped");
  CHECK(lane_sched::lanes_from_env(nullptr) == 4 && lane_sched::lanes_from_env("") == 4 && lane_sched::lanes_from_env("x") == 4, "not set");
  CHECK(lane_sched::lanes_from_env("20") == 20 && lane_sched::lanes_from_env("0") == 1 && lane_sched::lanes_from_env("-3") == 1 &&
        lane_sched::lanes_from_env("64") == 32 && lane_sched::lanes_from_env("99999999999999999999") == 32, "clamped to 1..32");
}

int main() {
  test_lpt();
  test_books();
  test_estimate();
  test_limit();
  if (g_failed) { std::printf("%d check(s) failed\n", g_failed); return 1; }
  std::printf("lane_sched: ok\n");
  return 0;
}
