// TEST DRIVER: the pool of pinned output buffers (fastq_utils_amd/host/fq_out_pool.h), alone - no GPU, no library:
// the pinned allocator is a stub over malloc that keeps count and can be told to fail.  Also under the sanitizers
// (tests/test_sanitizers.py).  No arguments.  Every case must end by itself (the test's time limit is the check for
// that).  Prints "ok <cases>" or the first violation.
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <chrono>
#include <thread>

#include "../../fastq_utils_amd/host/fq_out_pool.h"

namespace {

std::mutex g_mu;
std::set<void*> g_pinned;  // what the stub has handed out and not taken back
size_t g_max_live = 0, g_released = 0;
bool g_foreign = false;    // a pointer that is not the stub's came to its release
std::atomic<bool> g_fail{false};

void* stub_alloc(fqg_ctx*, size_t bytes) {
  if (g_fail || bytes > ((size_t)1 << 40)) return nullptr;
  void* p = malloc(bytes);
  std::lock_guard<std::mutex> lk(g_mu);
  g_pinned.insert(p);
  g_max_live = std::max(g_max_live, g_pinned.size());
  return p;
}
void stub_release(fqg_ctx*, void* p) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_pinned.erase(p)) g_foreign = true;
    ++g_released;
  }
  free(p);
}
size_t live() {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_pinned.size();
}
void reset() {
  std::lock_guard<std::mutex> lk(g_mu);
  g_max_live = g_released = 0;
  g_fail = false;
}
const fqhost::PinnedAlloc kStub{nullptr, stub_alloc, stub_release};

int g_cases = 0;
#define CHECK(cond, ...)             \
  do {                               \
    if (!(cond)) {                   \
      printf("line %d: ", __LINE__); \
      printf(__VA_ARGS__);           \
      printf("\n");                  \
      return false;                  \
    }                                \
  } while (0)

void nap() { std::this_thread::sleep_for(std::chrono::milliseconds(30)); }

// several threads take buffers of many sizes and give them back: never more than `limit` alive
bool never_more_than_limit(size_t limit, int threads) {
  ++g_cases;
  reset();
  {
    fqhost::OutPool pool(kStub, limit);
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
      th.emplace_back([&, t] {
        for (int i = 0; i < 200; ++i) {
          const size_t want = (size_t)1 + (size_t)((i * 7919 + t * 104729) % 50000);
          size_t cap = 0;
          char* p = pool.take(want, &cap);
          if (!p || cap < want) ++bad;
          else p[0] = p[want - 1] = (char)i;
          pool.give(p, cap);
        }
      });
    for (auto& x : th) x.join();
    CHECK(bad == 0, "%d takes brought nothing or too little", bad.load());
    CHECK(g_max_live <= limit, "%zu buffers alive, limit %zu", g_max_live, limit);
  }
  CHECK(live() == 0 && !g_foreign, "%zu buffers left behind the pool", live());
  return true;
}

// with every buffer out, take waits: for give (it gets that buffer), or for stop (it gets nothing)
bool take_waits(bool stopped) {
  ++g_cases;
  reset();
  fqhost::OutPool pool(kStub, 1);
  size_t cap = 0, cap2 = 0;
  char* p = pool.take(1000, &cap);
  CHECK(p && cap >= 1000, "the first take");
  std::atomic<bool> back{false};
  char* q = nullptr;
  std::thread waiter([&] {
    q = pool.take(500, &cap2);
    back = true;
  });
  nap();
  CHECK(!back, "take came back with the only buffer out");  // (a waiter that has not started yet fails nothing)
  if (stopped) pool.stop();
  else pool.give(p, cap);
  waiter.join();
  if (stopped) {
    CHECK(q == nullptr, "take after stop() brought a buffer");
    pool.give(p, cap);
  } else {
    CHECK(q == p && cap2 == cap, "take did not get the buffer that was given back");
    pool.give(q, cap2);
  }
  CHECK(g_max_live == 1, "%zu buffers made, limit 1", g_max_live);
  return true;
}

// a free buffer that is too small makes room for a larger one: it is released, not counted beside it
bool small_one_is_replaced() {
  ++g_cases;
  reset();
  fqhost::OutPool pool(kStub, 1);
  size_t cap = 0;
  char* p = pool.take(100, &cap);
  pool.give(p, cap);
  p = pool.take(100000, &cap);
  CHECK(p && cap >= 100000, "no buffer of the larger size");
  CHECK(g_released == 1 && live() == 1 && g_max_live == 1, "released %zu, alive %zu, most alive %zu", g_released, live(), g_max_live);
  pool.give(p, cap);
  char* q = pool.take(50, &cap);  // (and the slot count is right: the one buffer is handed out again, nothing waits)
  CHECK(q == p, "the large buffer was not reused");
  pool.give(q, cap);
  return true;
}

bool smallest_fitting_is_chosen() {
  ++g_cases;
  reset();
  fqhost::OutPool pool(kStub, 3);
  const size_t sizes[3] = {200000, 1000, 50000};  // (a buffer holds an eighth and 4 KiB more than was asked for)
  char* p[3];
  size_t cap[3];
  for (int i = 0; i < 3; ++i) p[i] = pool.take(sizes[i], &cap[i]);
  for (int i = 0; i < 3; ++i) pool.give(p[i], cap[i]);
  size_t c = 0;
  char* q = pool.take(30000, &c);
  CHECK(q == p[2] && c == cap[2], "30000 bytes asked for: got the buffer of %zu, not the one of %zu", c, cap[2]);
  char* r = pool.take(30000, &c);
  CHECK(r == p[0], "the next 30000 bytes: not the largest buffer");
  pool.give(q, cap[2]);
  pool.give(r, cap[0]);
  CHECK(g_max_live == 3 && g_released == 0, "most alive %zu, released %zu", g_max_live, g_released);
  return true;
}

// no pinned memory: pageable memory instead, which goes back through free() and never to the pinned allocator
bool falls_back_to_pageable() {
  ++g_cases;
  reset();
  {
    fqhost::OutPool pool(kStub, 2);
    g_fail = true;
    size_t cap = 0, cap2 = 0;
    char* p = pool.take(4000, &cap);
    CHECK(p && cap >= 4000 && live() == 0, "no pageable buffer");
    p[0] = p[3999] = 1;
    g_fail = false;
    char* q = pool.take(100, &cap2);  // a pinned one beside it
    CHECK(q && live() == 1, "no pinned buffer beside the pageable one");
    pool.give(p, cap);
    pool.give(q, cap2);
    // both too small and the limit reached: the pinned one makes room first, the pageable one for the next take
    p = pool.take(1000000, &cap);
    CHECK(p && cap >= 1000000, "no room made");
    q = pool.take(1000000, &cap2);
    CHECK(q && cap2 >= 1000000, "no room made twice");
    pool.give(p, cap);
    pool.give(q, cap2);
  }
  CHECK(!g_foreign, "a pageable buffer went to the pinned allocator's release");
  CHECK(live() == 0, "%zu pinned buffers left", live());
  return true;
}

// no memory of either kind: nothing comes back, and the slot is not used up
bool total_failure_takes_no_slot() {
  ++g_cases;
  reset();
  fqhost::OutPool pool(kStub, 1);
  size_t cap = 7;
  char* p = pool.take((size_t)1 << 60, &cap);
  CHECK(p == nullptr && cap == 0, "2^60 bytes were to be had");
  p = pool.take(100, &cap);  // (would wait for ever had the failure counted as a buffer)
  CHECK(p && cap >= 100 && live() == 1, "no buffer after the failure");
  pool.give(p, cap);
  return true;
}

}  // namespace

int main() {
  for (size_t limit : {1, 2, 5})
    for (int threads : {1, 4})
      if (!never_more_than_limit(limit, threads)) return 1;
  if (!take_waits(false) || !take_waits(true)) return 1;
  if (!small_one_is_replaced() || !smallest_fitting_is_chosen() || !falls_back_to_pageable() || !total_failure_takes_no_slot()) return 1;
  printf("ok %d\n", g_cases);
  return 0;
}
