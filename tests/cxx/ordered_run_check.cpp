// TEST DRIVER: the ordered worker pool under the loops over several contexts (fastq_utils_amd/host/fq_ordered.h),
// alone - no GPU, no library call - and under the sanitizers (tests/test_sanitizers.py).  No arguments.
// Items carry their number; work sleeps longer for lower numbers, so results arrive out of order.  Every case must
// end by itself (the test's time limit is the check for that).  Prints "ok <cases>" or the first violation.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../fastq_utils_amd/host/fq_ordered.h"

namespace {

struct Item {
  uint64_t seq = ~0ull;
  int worked = 0;
};
using Run = fqhost::OrderedRun<Item>;

int g_cases = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      printf("line %d: ", __LINE__);              \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
      return false;                               \
    }                                             \
  } while (0)

void nap_for(uint64_t n, uint64_t seq) { std::this_thread::sleep_for(std::chrono::microseconds(100 * (n > seq ? n - seq : 1))); }

// a source of n items with a gate: fetching item `gate_at` waits until abort() opens the gate, and there is no item
// then - a cutter waiting for a slot that nobody will give back
struct Source {
  uint64_t n, gate_at = ~0ull, window = 0;
  bool flag_last = true;  // false: the end shows only as a fetch that brings nothing
  std::mutex mu;
  std::condition_variable cv;
  bool open = false;
  std::atomic<uint64_t> fetched{0}, finished{0}, exits{0};
  std::atomic<bool> beyond_window{false}, out_of_order{false}, after_end{false};
  bool ended = false;  // (under the pool's fetch lock)

  Run::Fetch fetch() {
    return [this](uint64_t seq, Item& it, bool& last) {
      if (ended) after_end = true;  // nobody fetches again after the last item or after "nothing more"
      if (seq != fetched.load()) out_of_order = true;
      if (window && seq >= finished.load() + window) beyond_window = true;
      if (seq == gate_at) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return open; });
        ended = true;
        return false;
      }
      if (seq >= n) {
        ended = true;
        return false;
      }
      it.seq = seq;
      last = flag_last && seq + 1 == n;
      if (last) ended = true;
      ++fetched;
      return true;
    };
  }
  Run::Work work() {
    return [this](size_t, Item& it) {
      nap_for(n, it.seq);
      ++it.worked;
    };
  }
  std::function<void()> abort() {
    return [this] {
      std::lock_guard<std::mutex> lk(mu);
      open = true;
      cv.notify_all();
    };
  }
  Run::WorkerExit worker_exit() {
    return [this](size_t, const Run::Waits&) { ++exits; };
  }
  bool sound() const { return !beyond_window && !out_of_order && !after_end; }
};

// every item exactly once, in order; the consumer ends by itself
bool whole_run(size_t workers, uint64_t n, uint64_t window, bool flag_last) {
  ++g_cases;
  Source s;
  s.n = n, s.window = window, s.flag_last = flag_last;
  Run run(workers, window, s.fetch(), s.work(), s.abort(), s.worker_exit());
  uint64_t k = 0;
  Item it;
  while (run.next(it)) {
    CHECK(it.seq == k && it.worked == 1, "item %llu came as number %llu, worked on %d times", (unsigned long long)it.seq, (unsigned long long)k, it.worked);
    ++k;
    ++s.finished;  // (before the pool hears of it: what fetch compares with is never behind the pool's own count)
    run.done();
  }
  CHECK(k == n, "%llu of %llu items delivered", (unsigned long long)k, (unsigned long long)n);
  CHECK(!run.next(it), "an item behind the last one");
  run.stop();
  CHECK(s.exits == workers, "%llu of %zu workers ended", (unsigned long long)s.exits.load(), workers);
  CHECK(s.sound(), "fetch: beyond the window %d, out of order %d, after the end %d", (int)s.beyond_window, (int)s.out_of_order, (int)s.after_end);
  return true;
}

// the consumer stops at item k with workers waiting: at the gate inside fetch (by_window false), or for the window
// (the consumer is never done with item k).  how: 0 stop(), 1 stop() twice, 2 the destructor alone
bool early_stop(size_t workers, uint64_t n, uint64_t k, bool by_window, int how) {
  ++g_cases;
  Source s;
  s.n = n;
  if (by_window) s.window = workers + 1;
  else s.gate_at = k + 2;
  uint64_t delivered = 0;
  {
    Run run(workers, s.window, s.fetch(), s.work(), s.abort(), s.worker_exit());
    Item it;
    for (;;) {
      CHECK(run.next(it), "item %llu did not come", (unsigned long long)delivered);
      CHECK(it.seq == delivered, "item %llu came as number %llu", (unsigned long long)it.seq, (unsigned long long)delivered);
      ++delivered;
      if (it.seq == k) break;
      ++s.finished;
      run.done();
    }
    // (until the workers have fetched all they can and wait - or two seconds, which fails nothing: stop() has to end
    // the run wherever they are)
    const uint64_t reach = by_window ? std::min<uint64_t>(n, k + s.window) : std::min<uint64_t>(n, s.gate_at);
    for (int spin = 0; spin < 2000 && s.fetched.load() < reach; ++spin) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    if (how <= 1) {
      run.stop();
      CHECK(s.exits == workers, "%llu of %zu workers ended by stop()", (unsigned long long)s.exits.load(), workers);
      CHECK(!run.next(it), "an item behind the one the consumer stopped at");
      if (how == 1) run.stop();
    }
  }
  CHECK(s.exits == workers, "%llu of %zu workers ended", (unsigned long long)s.exits.load(), workers);
  CHECK(delivered == k + 1, "%llu items delivered, stopped at %llu", (unsigned long long)delivered, (unsigned long long)k);
  CHECK(s.sound(), "fetch: beyond the window %d, out of order %d, after the end %d", (int)s.beyond_window, (int)s.out_of_order, (int)s.after_end);
  return true;
}

}  // namespace

int main() {
  for (size_t workers : {1, 3})
    for (uint64_t n : {0, 1, 50})
      for (uint64_t window : {(uint64_t)0, (uint64_t)workers + 1})
        for (bool flag_last : {true, false})  // (false: fetch brings nothing before any item was marked last, as after an abort)
          if (!whole_run(workers, n, window, flag_last)) return 1;
  for (size_t workers : {1, 3})
    for (uint64_t k : {(uint64_t)7, (uint64_t)19})  // in the middle; the last item
      for (bool by_window : {false, true})
        for (int how : {0, 1, 2})
          if (!early_stop(workers, 20, k, by_window, how)) return 1;
  printf("ok %d\n", g_cases);
  return 0;
}
