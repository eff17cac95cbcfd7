// fq_ordered.h - N worker threads take items from one source in its order, work on them side by side, and ONE consumer
// gets the results back in that order.  The hand-over under the loops that spread a file over several contexts
// (FQGPU_DEVICES): the record-aligned pieces of fastq_info (fq_multi.h) and the record blocks of fastq_pre_barcodes
// (fq_blocks.h).  Nothing here knows what an item is; only the standard library is used.
//
//   fetch(seq, item, last)  under the fetch lock, one worker at a time: item number `seq` of the source; false when
//                           there is none (the source is used up, or was aborted).  `last` = true: no item follows.
//                           Nobody fetches again after either.
//   work(worker, item)      outside any lock.  A failure is data inside the item; it is not looked at here.
//   abort()                 from stop(): lets go whoever waits inside fetch or work for something that will not come
//   worker_exit(worker, w)  (optional) in the worker thread as it ends: what it waited for, FQGPU_TIMING
//
// The consumer thread calls next() until it is false, done() where a window bounds the items under way, and stop()
// (or the destructor) BEFORE it prints and leaves on anything that ends the run early: results behind the item it
// stopped at are dropped.
#pragma once
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

namespace fqhost {

template <class Item>
class OrderedRun {
 public:
  struct Waits {  // seconds of one worker
    double fetch = 0, hand_over = 0;
    uint64_t items = 0;
  };
  using Fetch = std::function<bool(uint64_t seq, Item& item, bool& last)>;
  using Work = std::function<void(size_t worker, Item& item)>;
  using WorkerExit = std::function<void(size_t worker, const Waits& w)>;

  // window > 0: no fetch begins `window` or more items ahead of the number the consumer is done() with
  OrderedRun(size_t n_workers, uint64_t window, Fetch fetch, Work work, std::function<void()> abort, WorkerExit worker_exit = nullptr)
      : window_(window), fetch_(std::move(fetch)), work_(std::move(work)), abort_(std::move(abort)), worker_exit_(std::move(worker_exit)) {
    for (size_t i = 0; i < n_workers; ++i) threads_.emplace_back([this, i] { run(i); });
  }
  ~OrderedRun() { stop(); }
  OrderedRun(const OrderedRun&) = delete;
  OrderedRun& operator=(const OrderedRun&) = delete;

  // the next item in fetch order; false behind the last one (and after stop())
  bool next(Item& out) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return stop_ || done_.count(taken_) || taken_ >= n_items_; });
    auto it = done_.find(taken_);
    if (stop_ || it == done_.end()) return false;
    out = std::move(it->second);
    done_.erase(it);
    ++taken_;
    return true;
  }
  // the consumer has finished with one more item (the window moves on)
  void done() {
    std::lock_guard<std::mutex> lk(mu_);
    ++finished_;
    cv_.notify_all();
  }
  // no more fetches, everybody woken, the workers joined.  Idempotent.
  void stop() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    if (threads_.empty()) return;
    if (abort_) abort_();
    for (auto& t : threads_) t.join();
    threads_.clear();
  }

 private:
  static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

  void run(size_t worker) {
    Waits w;
    for (;;) {
      Item item;
      uint64_t seq = 0;
      const double t0 = now();
      {
        std::lock_guard<std::mutex> fetching(fetch_mu_);
        if (window_) {  // (inside the fetch lock: the order of fetches is the order of arrival here)
          std::unique_lock<std::mutex> lk(mu_);
          cv_.wait(lk, [&] { return stop_ || next_seq_ < finished_ + window_; });
        }
        if (closed_ || stop_) break;
        bool last = false;
        const bool got = fetch_(next_seq_, item, last);
        if (got) seq = next_seq_++;
        if (!got || last) {  // the number of items is known: the consumer ends behind them
          closed_ = true;
          std::lock_guard<std::mutex> lk(mu_);
          n_items_ = next_seq_;
          cv_.notify_all();
        }
        if (!got) break;
      }
      const double t1 = now();
      work_(worker, item);
      const double t2 = now();
      {
        std::lock_guard<std::mutex> lk(mu_);
        done_.emplace(seq, std::move(item));
        cv_.notify_all();
      }
      w.fetch += t1 - t0, w.hand_over += now() - t2, ++w.items;
    }
    if (worker_exit_) worker_exit_(worker, w);
  }

  const uint64_t window_;
  const Fetch fetch_;
  const Work work_;
  const std::function<void()> abort_;
  const WorkerExit worker_exit_;
  std::mutex fetch_mu_, mu_;
  std::condition_variable cv_;  // (mu_) a result, the number of items, the window, stop
  std::atomic<bool> stop_{false};
  bool closed_ = false;         // (fetch_mu_) nobody fetches again
  uint64_t next_seq_ = 0;       // (fetch_mu_) items fetched so far
  uint64_t finished_ = 0, taken_ = 0, n_items_ = ~0ull;  // (mu_)
  std::map<uint64_t, Item> done_;                        // (mu_)
  std::vector<std::thread> threads_;                     // (the consumer's)
};

}  // namespace fqhost
