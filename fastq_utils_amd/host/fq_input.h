// fq_input.h - host side of the drop-in programs: reading (optionally gzipped) FASTQ files into
// pinned staging buffers, piece by piece, with the incomplete tail of one piece carried into the
// next.  Decompression stays on the host (zlib), as in the reference (src/fastq.c:631-661); how an input is opened
// and read is fq_source.h.
//
// Reading runs AHEAD of the GPU: a producer thread fills a ring of pinned slots while the caller has
// the previous piece copied to the device and validated (what the reference does serially with four
// gzgets per record, src/fastq.c:245-261).
//
// Layout of a slot: [ headroom | raw bytes ].  The producer writes raw file bytes behind the headroom
// without knowing where the previous piece's last complete record ended; the consumer learns that from
// the validation of the previous piece and copies the few carried bytes in FRONT of the raw bytes.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fqg.h"
#include "fq_reframe.h"
#include "fq_source.h"

namespace fqhost {

// The programs run one job and exit: un-pinning hundreds of megabytes of staging slots first (0.1 - 0.2 s) buys nothing -
// the operating system takes the memory back.  Set once by a program's main(); library-style users leave it alone.
// A slot that outlives its owner this way is NOT lost: it goes to a process-wide pool and the next reader (the second
// pass over a file, the second file of a pair, the one-device loop after a multi-device attempt) takes it over instead
// of pinning a new one - a program holds as many pinned slots as its busiest reader needs, however many readers it
// builds (the slots are portable pinned memory: any device's context may copy from them).
inline bool& keep_slots_until_exit() {
  static bool v = false;
  return v;
}

// input bytes handed to the GPU so far (every piece an Input gives out, carried tails not counted twice): what the
// machine-readable metrics of a program are made of (FQGPU_JSON_METRICS)
inline std::atomic<unsigned long long>& bytes_handed_out() {
  static std::atomic<unsigned long long> v{0};
  return v;
}

class SlotPool {
 public:
  static SlotPool& get() {
    static SlotPool* p = new SlotPool;  // (never destroyed: reader threads may still hold slots when the program leaves)
    return *p;
  }
  // pinned memory of at least `bytes`; nullptr when the allocation fails
  char* take(fqg_ctx* ctx, size_t bytes) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      size_t best = free_.size();
      for (size_t i = 0; i < free_.size(); ++i)
        if (free_[i].second >= bytes && free_[i].second <= bytes + bytes / 2 + (1u << 20) &&
            (best == free_.size() || free_[i].second < free_[best].second))
          best = i;
      if (best != free_.size()) {
        char* p = free_[best].first;
        free_.erase(free_.begin() + (long)best);
        return p;
      }
    }
    char* p = static_cast<char*>(fqg_host_alloc(ctx, bytes));
    if (p) {
      std::lock_guard<std::mutex> lk(mu_);
      size_[p] = bytes;
    }
    return p;
  }
  // the owner is done with it: back to the pool while the program keeps its slots, freed otherwise
  void give(fqg_ctx* ctx, char* p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(mu_);
    auto it = size_.find(p);
    if (keep_slots_until_exit() && it != size_.end()) {
      free_.emplace_back(p, it->second);
      return;
    }
    if (it != size_.end()) size_.erase(it);
    fqg_host_free(ctx, p);
  }
  size_t pinned_bytes() {  // (tests) everything this pool has handed out or holds
    std::lock_guard<std::mutex> lk(mu_);
    size_t t = 0;
    for (auto& kv : size_) t += kv.second;
    return t;
  }

 private:
  std::mutex mu_;
  std::vector<std::pair<char*, size_t>> free_;
  std::map<char*, size_t> size_;
};
// The piece size for a regular file of `file_bytes` bytes on disk: a slot for a small file need not have the size of a
// piece - pinning memory takes as long as filling it (128 MiB: 22 ms of every start, 512 MiB: 90 ms, per input file).
// A compressed file is given what 24 times its size inflates to, at least 1 MiB; one that inflates to more comes in
// several pieces, like any large file.  FQGPU_CHUNK_MB set: that size, exactly (the tests cut files where they want).
inline size_t piece_for_file(size_t piece, uint64_t file_bytes, bool compressed) {
  if (getenv("FQGPU_CHUNK_MB")) return piece;
  const uint64_t may = compressed ? file_bytes * 24 : file_bytes;
  const uint64_t mib = 1u << 20;
  const uint64_t want = std::max<uint64_t>(mib, (may + mib) & ~(mib - 1));
  return (size_t)std::min<uint64_t>(piece, want);
}
inline char* slot_alloc(fqg_ctx* ctx, size_t bytes) { return SlotPool::get().take(ctx, bytes); }
inline void slot_release(fqg_ctx* ctx, char* p) { SlotPool::get().give(ctx, p); }

// Readers that run ahead of the GPU, and exit().  A program that links the per-record library (libfastq_gpu.so under the
// reference's own main()) leaves through exit() whenever it likes - on its first finding, say, while a producer thread is
// pinning or filling the next slot, i.e. is INSIDE a HIP call.  exit() runs the HIP runtime's own teardown from one of
// its hooks; a thread of ours inside the runtime at that moment is a crash after everything has been said (a wrong exit
// status).  So the hooks stop the readers first: every Input with a live producer is registered here, and the handler
// - registered with atexit() when the first of them starts, i.e. AFTER the runtime was initialised by fqg_open, and
// therefore run BEFORE the runtime's handlers (exit() runs them last-registered first) - tells them to stop and joins
// them.  The drop-in programs themselves leave through _exit() (leave(), fq_source.h) and never get here.
class ExitQuiesce {
 public:
  typedef void (*StopFn)(void*);
  static ExitQuiesce& get() {
    static ExitQuiesce* p = new ExitQuiesce;  // (never destroyed: it is used from an exit handler)
    return *p;
  }
  void add(void* who, StopFn stop) {
    std::lock_guard<std::mutex> lk(mu_);
    live_.emplace_back(who, stop);
    if (!hooked_) {
      hooked_ = true;
      // (on_exit, glibc: the handler learns the status exit() was called with - it needs it when it gives up waiting)
      on_exit([](int status, void*) { ExitQuiesce::get().stop_all(status); }, nullptr);
    }
  }
  void remove(void* who) {
    std::lock_guard<std::mutex> lk(mu_);
    for (size_t i = 0; i < live_.size(); ++i)
      if (live_[i].first == who) {
        live_.erase(live_.begin() + (long)i);
        return;
      }
  }
  // Stops and joins every live reader - for at most kPatience: a reader blocked in read() / gzread() on a pipe that
  // has stalled (stdin, a slow upstream) only sees its stop flag when the read returns, and a program that leaves on its
  // first finding must not hang in exit() behind it.  When the patience runs out the process ends at once with the
  // status it was leaving with (_exit: no further handlers - the runtime's teardown is exactly what must not run beside
  // a thread that is still inside a HIP call).
  void stop_all(int status) {
    std::vector<std::pair<void*, StopFn>> all;
    {
      std::lock_guard<std::mutex> lk(mu_);
      all.swap(live_);
    }
    if (all.empty()) return;
    struct Wait {
      std::mutex mu;
      std::condition_variable cv;
      bool done = false;
    };
    auto w = std::make_shared<Wait>();
    std::thread t([all, w] {
      for (auto& e : all) e.second(e.first);
      {
        std::lock_guard<std::mutex> lk(w->mu);
        w->done = true;
      }
      w->cv.notify_all();
    });
    {
      std::unique_lock<std::mutex> lk(w->mu);
      if (!w->cv.wait_for(lk, std::chrono::seconds(kPatienceSeconds), [&] { return w->done; })) {
        fflush(nullptr);
        _exit(status);
      }
    }
    t.join();
  }
  static constexpr int kPatienceSeconds = 3;

 private:
  std::mutex mu_;
  std::vector<std::pair<void*, StopFn>> live_;
  bool hooked_ = false;
};

// Pinned slots handed from ONE producer to any number of consumers, for the readers whose items have no order among
// them (fq_multi.h, fq_blocks.h).  The producer takes a free slot (acquire), fills it and publishes an Item that says
// where in the slot it lies (Item::slot, Item::size); a consumer takes the next item (next) and gives its slot back
// (release).
//
// Pinning a slot takes six times as long as filling it (128 MiB: 23 ms against 3.6 ms from tmpfs): the slots are pinned
// by a thread of their own, one after the other, while the producer fills - and fills again - the ones it has.  (The
// producer pinned them itself, on its way: 0.18 s of a 0.5 s job in front of every byte read after them.)  All the
// slots the owner asked for are pinned while the producer still runs - consumers may each hold one while another
// waits for the next item with a lock of the caller's held - and a slot that cannot be pinned is the queue's failure:
// nobody is left waiting for a slot that will not come.
template <class Item>
class PinnedQueue {
 public:
  PinnedQueue(fqg_ctx* ctx, int n_slots) : ctx_(ctx), slots_((size_t)n_slots) {}
  ~PinnedQueue() {
    stop();
    for (auto& s : slots_) slot_release(ctx_, s.buf);
  }
  PinnedQueue(const PinnedQueue&) = delete;
  PinnedQueue& operator=(const PinnedQueue&) = delete;

  // the producer thread runs `produce`, the pinner gives every slot `slot_bytes`
  void start(size_t slot_bytes, std::function<void()> produce) {
    producer_ = std::thread(std::move(produce));
    pinner_ = std::thread([this, slot_bytes] { pin(slot_bytes); });
  }
  // both threads told to stop and joined (the owner's destructor, before it lets go of what the producer reads)
  void stop() {
    abort();
    if (producer_.joinable()) producer_.join();
    if (pinner_.joinable()) pinner_.join();
  }
  double pin_seconds() const { return t_pin_; }  // (FQGPU_TIMING; after stop())

  // ---- the producer's side ----
  // a free slot, now the producer's; -1 when the queue has stopped or failed
  int acquire() {
    std::unique_lock<std::mutex> lk(mu_);
    int s = -1;
    cv_.wait(lk, [&] {
      if (quit_ || failed_) return true;
      for (size_t i = 0; i < slots_.size(); ++i)
        if (slots_[i].buf && !slots_[i].busy) {
          s = (int)i;
          return true;
        }
      return false;
    });
    if (s >= 0) slots_[(size_t)s].busy = true;
    return s;
  }
  char* data(int slot) const { return slots_[(size_t)slot].buf; }
  // room for `want` bytes in a slot the producer holds, the first `keep` of them kept; false: the queue has failed
  bool grow(int slot, size_t keep, size_t want) {
    Slot& s = slots_[(size_t)slot];
    if (want <= s.cap) return true;
    const size_t cap = std::max(want, s.cap + s.cap / 2);
    char* nb = slot_alloc(ctx_, cap + 1);
    if (!nb) {
      fail("unable to allocate pinned memory");
      return false;
    }
    if (keep) memcpy(nb, s.buf, keep);
    slot_release(ctx_, s.buf);
    s.buf = nb;
    s.cap = cap;
    return true;
  }
  void give_back(int slot) {
    std::lock_guard<std::mutex> lk(mu_);
    slots_[(size_t)slot].busy = false;
    cv_.notify_all();
  }
  void publish(const Item& it) {
    std::lock_guard<std::mutex> lk(mu_);
    ready_.push_back(it);
    cv_.notify_all();
  }
  void finish() {  // the last item has been published
    std::lock_guard<std::mutex> lk(mu_);
    done_ = true;
    cv_.notify_all();
  }
  void fail(const std::string& msg) {
    std::lock_guard<std::mutex> lk(mu_);
    fail_locked(msg);
  }
  bool stopped() {
    std::lock_guard<std::mutex> lk(mu_);
    return quit_;
  }

  // ---- the consumers' side (thread-safe) ----
  // next item in the producer's order; false when there are no more
  bool next(Item* out) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return !ready_.empty() || done_ || failed_ || quit_; });
    if (quit_) return false;
    if (failed_) {
      FQ_PRINT_ERROR("%s.\n", fail_msg_.c_str());
      leave(kExitSys);
    }
    if (ready_.empty()) return false;
    *out = ready_.front();
    ready_.pop_front();
    bytes_handed_out() += out->size;
    return true;
  }
  void release(const Item& it) { give_back(it.slot); }
  // Stop handing out items: wakes the producer (which may be waiting for a free slot that nobody will release any
  // more) and every consumer waiting in next(), which then returns false.  For the error paths of the consumers: they
  // stop with items still held, and joining them without this would wait forever.
  void abort() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
    }
    cv_.notify_all();
  }

 private:
  struct Slot {
    char* buf = nullptr;
    size_t cap = 0;
    bool busy = false;
  };
  void fail_locked(const std::string& msg) {
    if (!failed_) fail_msg_ = msg;
    failed_ = true;
    cv_.notify_all();
  }
  void pin(size_t bytes) {
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < slots_.size(); ++i) {
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (quit_ || failed_ || done_) break;
      }
      char* buf = slot_alloc(ctx_, bytes + 1);
      std::lock_guard<std::mutex> lk(mu_);
      if (!buf) {
        if (!quit_ && !done_) fail_locked("unable to allocate pinned memory");  // (nobody needs the slot any more otherwise)
        break;
      }
      slots_[i].buf = buf;
      slots_[i].cap = bytes;
      cv_.notify_all();
    }
    t_pin_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }

  fqg_ctx* ctx_;
  std::vector<Slot> slots_;
  std::deque<Item> ready_;
  std::thread producer_, pinner_;
  std::mutex mu_;
  std::condition_variable cv_;
  bool quit_ = false, failed_ = false, done_ = false;
  std::string fail_msg_;
  double t_pin_ = 0;
};

class Input {
 public:
  Input(fqg_ctx* ctx, const char* path, size_t piece_bytes) : ctx_(ctx), src_(path, bgzf_blocks()), cap_(piece_bytes) {
    if (src_.inflated() && src_.file_bytes()) cap_ = piece_for_file(cap_, src_.file_bytes(), true);
    if (src_.kind() == FastqSource::kPlain && src_.plain_bytes() < cap_) cap_ = std::max<size_t>(src_.plain_bytes(), 1);  // small file: one small slot
    if (src_.kind() == FastqSource::kBgzf) cap_ = std::max<size_t>(cap_, 1u << 17);  // (whole blocks of up to 64 KiB are inflated into a slot)
    // The reference's gzgets limits (fq_reframe.h).  Inflated input and stdin pass through one thread anyway: it cuts
    // as it goes (a memchr per line beside the inflate).  A plain file is read by many threads and handed over as it
    // is; the GPU reports a line beyond the limits (FQG_E_LINE_TOO_LONG) and the program starts over with
    // FQGPU_REFRAME set (fq_respawn.h), which brings it here.
    reframe_ = (src_.inflated() && reframe_supported()) || reframing();
  }
  // the producer is told to stop and joined (the destructor; exit(): ExitQuiesce)
  void stop_reading() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
    }
    cv_.notify_all();
    if (producer_.joinable() && producer_.get_id() != std::this_thread::get_id()) producer_.join();
  }
  ~Input() {
    ExitQuiesce::get().remove(this);
    stop_reading();
    for (Slot& s : slots_) slot_release(ctx_, s.buf);
    slot_release(ctx_, whole_);
    slot_release(ctx_, big_);
  }
  Input(const Input&) = delete;
  Input& operator=(const Input&) = delete;

  // Next piece: the carried tail of the previous one followed by fresh bytes.  Returns false once
  // the final piece has been handed out.  An empty file yields one empty, final piece.
  bool next(bool whole_file = false) {
    if (finished_) return false;
    if (whole_file) return next_whole();
    if (!producer_.joinable()) {
      ExitQuiesce::get().add(this, [](void* in) { static_cast<Input*>(in)->stop_reading(); });
      producer_ = std::thread([this] { produce(); });
    }
    const int prev = cur_;
    // carried bytes of the piece the caller is done with
    const char* carry_src = nullptr;
    size_t carry = 0;
    if (prev >= 0 && have_carry_) {
      carry_src = data_ + carry_at_;
      carry = len_ - carry_at_;
    }
    have_carry_ = false;
    const int want = (prev + 1) % kSlots;
    Slot& s = slots_[want];
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return s.ready || failed_; });
      if (failed_) {
        FQ_PRINT_ERROR("%s.\n", fail_msg_.c_str());
        leave(kExitSys);
      }
    }
    if (carry > s.head) {  // a tail longer than the headroom (a record of megabases): rebuild this one piece
      char* nb = alloc(carry + s.len + 1);
      memcpy(nb, carry_src, carry);
      memcpy(nb + carry, s.buf + s.head, s.len);
      slot_release(ctx_, big_);
      big_ = nb;
      data_ = nb;
    } else {
      if (carry) memcpy(s.buf + s.head - carry, carry_src, carry);
      data_ = s.buf + s.head - carry;
    }
    len_ = carry + s.len;
    bytes_handed_out() += s.len;
    eof_ = s.last;
    if (prev >= 0) {  // the previous slot may be refilled
      std::lock_guard<std::mutex> lk(mu_);
      slots_[prev].ready = false;
      cv_.notify_all();
    }
    cur_ = want;
    if (eof_) finished_ = true;
    return true;
  }
  // keep bytes [consumed, size) for the next piece (only meaningful for non-final pieces); the bytes of
  // the current piece stay readable until the next call of next()
  void carry_from(size_t consumed) {
    carry_at_ = consumed;
    have_carry_ = true;
    if (whole_mode_) whole_carry_ = len_ - consumed;
  }
  void stop() { finished_ = true; }
  const char* data() const { return data_; }
  size_t size() const { return len_; }
  bool final() const { return eof_; }
  // what fqg_validate must be told about this input's pieces
  uint32_t vflags() const { return reframe_ ? FQG_VALIDATE_REFRAMED : 0u; }
  // bytes of a plain (uncompressed, seekable) input, 0 when unknown: a size hint for whoever sizes tables from it
  uint64_t plain_bytes() const { return src_.plain_bytes(); }
  const std::string& path() const { return src_.path(); }

 private:
  static constexpr int kSlots = 3;
  static constexpr size_t kHead = 8u << 20;  // > the longest record the reference's line buffers admit
  struct Slot {
    char* buf = nullptr;
    size_t head = 0, len = 0;
    bool ready = false, last = false, allocated = false;
  };

  // bytes a slot holds behind its headroom: the piece, and in re-framing mode the two bytes per cut on top of a piece
  // of at least kReframeMin bytes (the bytes held back from one round to the next stay below the longest limit)
  static constexpr size_t kReframeMin = 4u << 20;
  size_t slot_room() const {
    if (!reframe_) return cap_;
    const size_t c = std::max(cap_, kReframeMin);
    return c + c / 256 + 64;
  }
  char* alloc(size_t n) {
    char* p = slot_alloc(ctx_, n);
    if (!p) {
      FQ_PRINT_ERROR("unable to allocate %zu bytes of pinned memory", n);
      leave(kExitSys);
    }
    return p;
  }

  static FastqSource::Options bgzf_blocks() {
    FastqSource::Options o;
    o.bgzf = true;
    return o;
  }
  void fail(const std::string& msg) {
    std::lock_guard<std::mutex> lk(mu_);
    fail_msg_ = msg;
    failed_ = true;
    cv_.notify_all();
  }

  // The reference's reads return whole lines as long as no line reaches the smallest of its buffers: then there is nothing
  // to cut, whichever call reads which line, and all the line reader's state needs is the number of lines (fq_reframe.h).
  // That is every ordinary file, and looking for the longest line is work for many threads - the walk line by line on the
  // one thread that feeds the GPU was a sixth of the time a gzip'd file of 100 M reads took.  true: raw[0, *taken) stands
  // as it is (everything but an unfinished last line; everything when at_end) and the reader's state is up to date.
  bool short_lines_only(const char* raw, size_t n, bool at_end, size_t* taken) {
    const size_t limit = Reframer::room(0);  // 999: a line of that many bytes with its newline still comes back whole
    if (n < (1u << 20)) return false;        // (small pieces: the one thread is as fast as asking the others)
    if (!scan_pool_) scan_pool_.reset(new ReaderPool(std::min(host_threads(), 32u)));
    const unsigned T = (unsigned)std::min<size_t>(scan_pool_->size(), n >> 20);
    struct Part {
      size_t first = 0, last = 0, count = 0, longest = 0;  // first / last newline (when count), longest stretch between two of them
    };
    std::vector<Part> parts(T);
    scan_pool_->run(T, [&](unsigned t) {
      const size_t a = n * t / T, b = n * (t + 1) / T;
      Part& p = parts[t];
      size_t at = a;
      while (at < b) {
        const char* nl = static_cast<const char*>(memchr(raw + at, '\n', b - at));
        if (!nl) break;
        const size_t q = (size_t)(nl - raw);
        if (!p.count) p.first = q;
        else p.longest = std::max(p.longest, q - p.last);
        p.last = q;
        ++p.count;
        at = q + 1;
      }
    });
    // the stretches that cross from one thread's part into the next, the first line and the unfinished last one
    size_t prev_nl = (size_t)-1, lines = 0, longest = 0;  // (position of the newline in front of the current line; -1: raw's first byte starts it)
    for (const Part& p : parts) {
      if (!p.count) continue;
      longest = std::max(longest, std::max(p.longest, p.first - prev_nl));  // (unsigned: first - (-1) = first + 1 = the line with its newline)
      prev_nl = p.last;
      lines += p.count;
    }
    const size_t tail = n - (prev_nl + 1);  // bytes behind the last newline
    if (longest > limit || tail >= limit) return false;
    rf_.phase = (unsigned)((rf_.phase + lines) & 3u);
    *taken = at_end ? n : prev_nl + 1;
    return true;
  }

  void produce() {
    // pinning a slot takes as long as filling it: the slots behind the first are allocated by a helper while the first
    // is being read (the file may well end inside the first)
    const size_t head = std::min(kHead, std::max<size_t>(cap_, 4096));  // (tiny files: tiny slots)
    std::thread helper;
    const bool more = src_.plain_bytes() > cap_;  // (gz input, stdin: unknown - the slots are pinned as they are needed)
    if (more)
      helper = std::thread([this, head] {
        for (int i = 1; i < kSlots; ++i) {
          char* b = slot_alloc(ctx_, head + slot_room() + 1);
          std::lock_guard<std::mutex> lk(mu_);
          slots_[i].buf = b;
          slots_[i].allocated = true;
          cv_.notify_all();
          if (!b || quit_) return;
        }
      });
    struct Join {
      std::thread& t;
      ~Join() {
        if (t.joinable()) t.join();
      }
    } join{helper};
    for (int i = 0;; i = (i + 1) % kSlots) {
      Slot& s = slots_[i];
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return (!s.ready && (i == 0 || !more || s.allocated)) || quit_; });
        if (quit_) return;
      }
      if (!s.buf) {
        if (i > 0 && more) return fail("unable to allocate pinned memory");
        s.buf = alloc(head + slot_room() + 1);
      }
      s.head = head;
      bool at_end = false;
      size_t len;
      if (!reframe_) len = src_.read(s.buf + s.head, cap_, &at_end);
      else {
        // raw bytes = what the last round held back + a fresh read; the cut form of what can be judged goes out
        char* raw = s.buf + s.head;
        const size_t held = rf_tail_.size(), want = std::max(cap_, kReframeMin) - held;
        if (held) memcpy(raw, rf_tail_.data(), held);
        const size_t n = held + src_.read(raw + held, want, &at_end);
        bool clean = true;
        size_t taken;
        if (!short_lines_only(raw, n, at_end, &taken)) taken = rf_.run(raw, n, at_end, rf_out_, &clean);
        rf_tail_.assign(raw + taken, n - taken);
        len = taken;
        if (!clean) {
          // (cannot be: two bytes per limit - 1 >= 999 bytes were allowed for)
          if (rf_out_.size() > slot_room()) return fail("internal: a re-framed piece outgrew its slot");
          memcpy(raw, rf_out_.data(), rf_out_.size());
          len = rf_out_.size();
        }
      }
      if (src_.failed()) return fail(src_.error());
      {
        std::lock_guard<std::mutex> lk(mu_);
        s.len = len;
        s.last = at_end;
        s.ready = true;
        cv_.notify_all();
        if (at_end) return;
      }
    }
  }

  // the whole (rest of the) file as one image, read on the calling thread
  bool next_whole() {
    whole_mode_ = true;
    size_t cap = std::max<size_t>(cap_, 4096), len = whole_carry_;
    // a plain file's size is known: one allocation of exactly what is left (growing by doubling would hold the old and
    // the new pinned buffer at once and copy a 32 GB file seven times); gz input and stdin grow as they go
    if (src_.kind() == FastqSource::kPlain) cap = std::max<size_t>((size_t)src_.plain_left() + len + 1, 4096);
    char* buf = alloc(cap + 1);
    if (len) memcpy(buf, data_ + carry_at_, len);
    whole_carry_ = 0;
    bool at_end = false;
    while (!at_end) {
      if (len == cap || (src_.kind() == FastqSource::kBgzf && cap - len < 65536)) {  // (whole blocks only)
        char* nb = alloc(cap * 2 + 1);
        memcpy(nb, buf, len);
        slot_release(ctx_, buf);
        buf = nb;
        cap *= 2;
      }
      len += src_.read(buf + len, cap - len, &at_end);
      if (src_.failed()) {
        FQ_PRINT_ERROR("%s.\n", src_.error().c_str());
        leave(kExitSys);
      }
    }
    if (reframe_) {
      bool clean = true;
      rf_.run(buf, len, true, rf_out_, &clean);  // (the whole file at once: this object hands out nothing else)
      if (!clean) {
        char* nb = alloc(rf_out_.size() + 1);
        memcpy(nb, rf_out_.data(), rf_out_.size());
        slot_release(ctx_, buf);
        buf = nb;
        len = rf_out_.size();
      }
    }
    slot_release(ctx_, whole_);
    whole_ = buf;
    data_ = buf;
    len_ = len;
    bytes_handed_out() += len;
    eof_ = true;
    finished_ = true;
    return true;
  }

  fqg_ctx* ctx_;
  FastqSource src_;
  size_t cap_;
  Slot slots_[kSlots];
  std::unique_ptr<ReaderPool> scan_pool_;
  std::thread producer_;
  std::mutex mu_;
  std::condition_variable cv_;
  bool quit_ = false, failed_ = false;
  std::string fail_msg_;
  // the piece the caller holds
  int cur_ = -1;
  const char* data_ = nullptr;
  char *big_ = nullptr, *whole_ = nullptr;
  size_t len_ = 0, carry_at_ = 0, whole_carry_ = 0;
  bool have_carry_ = false, whole_mode_ = false;
  bool eof_ = false, finished_ = false;
  // the reference's gzgets limits (fq_reframe.h); the state belongs to whichever thread reads (producer or next_whole)
  bool reframe_ = false;
  Reframer rf_;
  std::string rf_tail_, rf_out_;
};

}  // namespace fqhost
