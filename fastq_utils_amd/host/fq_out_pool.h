// fq_out_pool.h - the pinned buffers in which a batch's output text comes back from the GPU: a fixed number of them
// goes round between the threads that fetch the text and the thread that writes it.  Into fresh pageable memory the
// copy ran at 7.5 GB/s per context (page faults, a bounce buffer) and the copies of the next blocks TO the GPU waited
// behind it: 28 s for 200 M pairs where pinned buffers take 6.7.  take() makes the buffers as they are first asked for,
// and blocks once `limit` of them are out until give() brings one back - or stop() ends the run.
// The header names no symbol of the library (the allocator comes as two function pointers, FQ_PINNED_ALLOC(ctx) for a
// program that links libfqgpu.so), so the host-only check links without it.
#pragma once
#include <condition_variable>
#include <cstdlib>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "../../include/fqg.h"

namespace fqhost {

struct PinnedAlloc {
  fqg_ctx* ctx = nullptr;
  void* (*alloc)(fqg_ctx*, size_t) = nullptr;
  void (*release)(fqg_ctx*, void*) = nullptr;
};
#define FQ_PINNED_ALLOC(ctx) (fqhost::PinnedAlloc{(ctx), fqg_host_alloc, fqg_host_free})

class OutPool {
 public:
  OutPool(const PinnedAlloc& mem, size_t limit) : mem_(mem), limit_(limit) {}
  OutPool(const OutPool&) = delete;
  ~OutPool() {
    for (auto& f : free_) drop(f.first, pageable_.erase(f.first) != 0);
  }

  // a buffer of at least `bytes` (*cap: what it holds); nullptr after stop(), or when no memory at all is to be had
  char* take(size_t bytes, size_t* cap) {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      size_t best = free_.size();  // a free one that is large enough: the smallest such
      for (size_t i = 0; i < free_.size(); ++i)
        if (free_[i].second >= bytes && (best == free_.size() || free_[i].second < free_[best].second)) best = i;
      if (best != free_.size()) {
        char* p = free_[best].first;
        *cap = free_[best].second;
        free_.erase(free_.begin() + (long)best);
        return p;
      }
      if (n_made_ < limit_) {
        ++n_made_;
        lk.unlock();
        const size_t want = bytes + bytes / 8 + 4096;
        char* p = static_cast<char*>(mem_.alloc(mem_.ctx, want));
        const bool plain = !p;  // (no pinned memory to be had: pageable memory does it, slower)
        if (plain) p = static_cast<char*>(malloc(want));
        *cap = p ? want : 0;
        if (plain) {
          lk.lock();
          if (!p) --n_made_;
          else pageable_.insert(p);
        }
        return p;
      }
      if (!free_.empty()) {  // every buffer made, none of the free ones large enough: one of them makes room
        char* small = free_.back().first;
        free_.pop_back();
        --n_made_;
        const bool plain = pageable_.erase(small) != 0;
        lk.unlock();
        drop(small, plain);
        lk.lock();
        continue;
      }
      if (quit_) return nullptr;
      cv_.wait(lk);
    }
  }
  void give(char* p, size_t cap) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(mu_);
    free_.emplace_back(p, cap);
    cv_.notify_all();
  }
  void stop() {  // whoever waits in take() gets nullptr
    std::lock_guard<std::mutex> lk(mu_);
    quit_ = true;
    cv_.notify_all();
  }

 private:
  void drop(char* p, bool plain) {
    if (plain) free(p);
    else mem_.release(mem_.ctx, p);
  }
  PinnedAlloc mem_;
  size_t limit_, n_made_ = 0;
  std::vector<std::pair<char*, size_t>> free_;
  std::set<char*> pageable_;  // buffers that are not pinned (the pinned allocation failed)
  std::mutex mu_;
  std::condition_variable cv_;
  bool quit_ = false;
};

}  // namespace fqhost
