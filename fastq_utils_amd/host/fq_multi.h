// fq_multi.h - the -r pass of fastq_info (validate_single_fastq_file, reference src/fastq_info.c:155-176) over
// several GPUs of one node: FQGPU_DEVICES=0,1,...  ("validation shards naturally").
//
// One host thread + one fqg_ctx + one statistics accumulator per device.  The file is cut into pieces that START AND
// END AT RECORD BOUNDARIES without looking at a GPU: a record starts at every fourth line, so counting newlines on
// the host (the reader threads do it while the bytes are in their cache) gives every piece its first line number,
// and the bytes of the record that straddles a cut are moved to the piece it began in.  Pieces then have no order
// among them: whichever device is free takes the next one.  What the serial loop would report - the first finding
// in file order, the progress ticker, the statistics of a clean file - is put together on the host: findings by
// piece order, statistics by fqg_acc_export / fqg_acc_merge.  No collective is needed on this path.
// (How the pieces go to the devices' threads and their results come back in piece order: fq_ordered.h.)
#pragma once
#include <functional>

#include "fq_input.h"

namespace fqhost {

struct Piece {
  char* data = nullptr;        // record-aligned image (points into a slot)
  size_t size = 0;
  uint64_t first_record = 0;   // records of the file before it
  uint64_t stream_offset = 0;  // bytes of the (inflated) file before it
  bool final = false;
  int slot = -1;
  uint64_t seq = 0;            // position in file order
};

class AlignedPieces {
 public:
  // limit: the file is taken to end after this many (inflated) bytes
  AlignedPieces(fqg_ctx* ctx, const char* path, size_t piece_bytes, int n_slots, uint64_t limit = ~0ull)
      : src_(path, up_to(limit)), cap_(piece_bytes), q_(ctx, n_slots) {
    // (small files: small slots - pinning is start-up time)
    if (src_.kind() == FastqSource::kPlain) cap_ = piece_for_file(cap_, src_.plain_bytes(), false);
    else if (src_.file_bytes()) cap_ = piece_for_file(cap_, src_.file_bytes(), true);
    q_.start(cap_ + kTail, [this] { produce(); });
  }
  ~AlignedPieces() {
    q_.stop();
    if (getenv("FQGPU_TIMING"))
      fprintf(fqhost::diag(), "fqgpu timing: piece cutter: %llu slots filled; waiting for a free (pinned) slot %.3f s, pinning (beside it) %.3f s, reading + counting lines %.3f s, cutting %.3f s\n",
              (unsigned long long)t_slots_, t_wait_, q_.pin_seconds(), t_read_, t_cut_);
  }
  // next piece in file order; false when the file is exhausted.  Thread-safe.
  bool next(Piece* out) { return q_.next(out); }
  void release(const Piece& p) { q_.release(p); }
  // stop handing out pieces (the error paths of the consumers: they stop with pieces still held)
  void abort() { q_.abort(); }

 private:
  static constexpr size_t kTail = 8u << 20;  // room behind a slot's bytes for the rest of a straddling record
  static FastqSource::Options up_to(uint64_t limit) {
    FastqSource::Options o;
    o.limit = limit;
    return o;
  }

  void produce() {
    // `held`: the piece whose end is not known yet (the record that straddles the next cut still has to be added)
    Piece held;
    bool have_held = false;
    size_t held_tail = 0;       // bytes of later slots already added behind it
    uint64_t lines_before = 0;  // newlines in the file before the raw bytes being read
    bool mid_line = false;      // the previous raw byte was not a newline
    bool at_end = false;
    uint64_t seq = 0;
    uint64_t raw_before = 0;    // bytes of the file before the raw bytes being read
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    while (!at_end) {
      const double t0 = now();
      const int si = q_.acquire();
      if (si < 0) return;
      const double t1 = now();
      char* const buf = q_.data(si);
      FastqSource::Lines runs;
      const size_t len = src_.read(buf, cap_, &at_end, &runs);
      if (src_.failed()) return q_.fail(src_.error());
      uint64_t nl = 0;
      for (const FastqSource::LineRun& r : runs) nl += r.lines;
      const double t3 = now();
      t_wait_ += t1 - t0, t_read_ += t3 - t1, ++t_slots_;
      struct Cut {
        double& acc;
        double from;
        std::function<double()> clock;
        ~Cut() { acc += clock() - from; }
      } cut_timer{t_cut_, t3, now};
      // where the first record of these bytes starts: at the first line whose number is a multiple of four
      uint64_t skip_lines = (4 - lines_before % 4) % 4;
      if (mid_line && skip_lines == 0) skip_lines = 4;
      if (!have_held) skip_lines = 0;  // the file starts with a record
      size_t skip = 0;
      bool found = true;
      for (uint64_t k = 0; k < skip_lines; ++k) {
        const char* p = (const char*)memchr(buf + skip, '\n', len - skip);
        if (!p) {
          found = false;
          break;
        }
        skip = (size_t)(p - buf) + 1;
      }
      if (!found) skip = len;  // no record starts in these bytes: all of them belong to the held piece
      if (have_held) {
        if (held_tail + skip > kTail)
          return q_.fail("more than 8 MiB of one record straddle two pieces (FQGPU_DEVICES): use one device");
        memcpy(held.data + held.size, buf, skip);
        held.size += skip;
        held_tail += skip;
      }
      if (found && (skip < len || at_end)) {
        if (have_held) q_.publish(held);
        held = Piece();
        held.data = buf + skip;
        held.size = len - skip;
        held.first_record = (lines_before + skip_lines) / 4;
        held.stream_offset = raw_before + skip;
        held.slot = si;
        held.seq = seq++;
        held_tail = 0;
        have_held = true;
      } else {
        q_.give_back(si);  // nothing of this slot starts a piece (its bytes were appended to the held piece)
      }
      lines_before += nl;
      raw_before += len;
      if (len) mid_line = buf[len - 1] != '\n';
    }
    if (have_held) {
      held.final = true;
      q_.publish(held);
    } else {
      // an empty file: one empty, final piece
      const int si = q_.acquire();
      if (si < 0) return;
      Piece p;
      p.data = q_.data(si);
      p.final = true;
      p.slot = si;
      q_.publish(p);
    }
    q_.finish();
  }

  FastqSource src_;
  size_t cap_;
  double t_wait_ = 0, t_read_ = 0, t_cut_ = 0;  // FQGPU_TIMING (written by the producer, read after its join)
  uint64_t t_slots_ = 0;
  PinnedQueue<Piece> q_;  // (last: its threads are gone before anything they use)
};

inline std::vector<int> devices_from_env() {
  std::vector<int> d;
  const char* e = getenv("FQGPU_DEVICES");
  if (!e) return d;
  for (const char* p = e; *p;) {
    char* end = nullptr;
    const long v = strtol(p, &end, 10);
    if (end == p) break;
    d.push_back((int)v);
    p = *end == ',' ? end + 1 : end;
  }
  return d;
}

// the contexts of a run over `devs`: `first` (open already, on devs[0]) and one more for every further entry
inline std::vector<fqg_ctx*> open_more_contexts(fqg_ctx* first, const std::vector<int>& devs) {
  std::vector<fqg_ctx*> ctx(devs.size(), first);
  for (size_t i = 1; i < devs.size(); ++i) {
    const int rc = fqg_open(devs[i], &ctx[i]);
    if (rc != 0) {
      FQ_PRINT_ERROR("FQGPU_DEVICES: device %d is not a usable MI355X GPU (fqg_open: %d)", devs[i], rc);
      leave(kExitSys);
    }
  }
  return ctx;
}

}  // namespace fqhost
