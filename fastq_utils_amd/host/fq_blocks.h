// fq_blocks.h - one (gz) FASTQ input cut into BLOCKS OF EXACTLY B RECORDS (the last block: what is left), without
// looking at a GPU.  For programs that walk several inputs in lock step (fastq_pre_barcodes, reference
// src/fastq_pre_barcodes.c:594-727: iteration k uses record k of every input): when every input is cut at the same
// record numbers, block j of all inputs is a unit of work with no order among the units, and whichever device is free
// takes the next one ("shards naturally" by record block).
// (How the units go to the devices' threads and their results come back in unit order: fq_ordered.h.)
//
// A record is four lines, so the cut behind record R is the byte behind the 4R-th newline.  The reader threads count
// the newlines of what they read while the bytes are in their cache (as host/fq_multi.h does); the cut is then
// searched only inside the one part whose count crosses 4R.  Bytes read beyond a cut are carried into the next block.
#pragma once
#include "fq_input.h"

namespace fqhost {

struct Block {
  char* data = nullptr;  // pinned
  size_t size = 0;
  uint64_t first_record = 0;  // == seq * B
  uint64_t lines = 0;         // newlines among the bytes (4 * B in every block but the last)
  bool final = false;
  int slot = -1;
  uint64_t seq = 0;
};

class RecordBlocks {
 public:
  static constexpr size_t kPeek = 1u << 20;

  RecordBlocks(fqg_ctx* ctx, const char* path, int n_slots) : src_(path, FastqSource::Options()), q_(ctx, n_slots) {
    // the first bytes, read here: the caller probes the first record in them and sizes the blocks from their lines
    carry_.resize(kPeek);
    FastqSource::Lines runs;
    const size_t got = src_.read(carry_.data(), kPeek, &at_end_, &runs);
    if (src_.failed()) {
      FQ_PRINT_ERROR("%s.\n", src_.error().c_str());
      leave(kExitSys);
    }
    carry_.resize(got);
    for (const FastqSource::LineRun& r : runs) carry_lines_ += r.lines;
  }
  ~RecordBlocks() {
    q_.stop();
    if (getenv("FQGPU_TIMING"))
      fprintf(diag(), "fqgpu timing: block cutter of %s: %llu blocks; waiting for a free (pinned) slot %.3f s, reading + counting lines %.3f s, cutting + carrying %.3f s\n",
              path().c_str(), (unsigned long long)t_blocks_, t_wait_, t_read_, t_cut_);
  }
  RecordBlocks(const RecordBlocks&) = delete;
  RecordBlocks& operator=(const RecordBlocks&) = delete;

  const char* peek() const { return carry_.data(); }
  size_t peek_size() const { return carry_.size(); }
  uint64_t peek_lines() const { return carry_lines_; }
  const std::string& path() const { return src_.path(); }

  // blocks of `records` records from now on (call once, before the first next())
  void start(uint64_t records) {
    per_block_ = std::max<uint64_t>(records, 1);
    // (bytes per line so far; a file without a newline in its first bytes is one long line)
    bytes_per_line_ = carry_lines_ ? (double)carry_.size() / (double)carry_lines_ : (double)std::max<size_t>(carry_.size(), 64);
    // every slot is pinned at the size a block is expected to have; one that turns out larger grows its slot where it is
    q_.start(block_bytes_estimate(), [this] { produce(); });
  }
  // next block in file order; false when the input is used up.  Thread-safe.
  bool next(Block* out) { return q_.next(out); }
  void release(const Block& b) { q_.release(b); }
  // stop handing out blocks (error paths: consumers stop with blocks held)
  void abort() { q_.abort(); }

 private:
  // what 4 * per_block_ lines are expected to take.  (No block is longer than its file: a small plain file gets small
  // slots; a gzip file may inflate to 24 times its size and more.)
  size_t block_bytes_estimate() const {
    const size_t room = (size_t)((double)(4 * per_block_) * bytes_per_line_ * 1.06) + (1u << 20);
    return src_.kind() == FastqSource::kPlain ? (size_t)std::min<uint64_t>(room, src_.plain_bytes() + (64u << 10)) : room;
  }

  void produce() {
    const uint64_t need = 4 * per_block_;
    uint64_t seq = 0;
    for (;;) {
      if (at_end_ && carry_.empty() && seq > 0) break;
      const double t0 = t_clock();
      const int si = q_.acquire();
      if (si < 0) return;
      const double t1 = t_clock();
      t_wait_ += t1 - t0;
      double t_reading = 0;
      FastqSource::Lines segs;  // runs of the block's bytes whose newline counts are known
      size_t len = carry_.size();
      uint64_t lines = carry_lines_;
      if (!q_.grow(si, 0, std::max<size_t>(block_bytes_estimate(), len))) return;
      if (len) {
        memcpy(q_.data(si), carry_.data(), len);
        segs.push_back(FastqSource::LineRun{0, len, lines});
      }
      carry_.clear();
      carry_lines_ = 0;
      while (lines < need && !at_end_) {
        // what the missing lines should take, a little more than that: the surplus is carried, a shortfall reads again
        size_t est = (size_t)((double)(need - lines) * bytes_per_line_ * 1.03) + (64u << 10);
        if (src_.kind() == FastqSource::kPlain) est = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(est, src_.plain_left()));  // (what the file still has)
        if (!q_.grow(si, len, len + est)) return;
        const double tr = t_clock();
        const size_t had = segs.size();
        const size_t got = src_.read(q_.data(si) + len, est, &at_end_, &segs);
        t_reading += t_clock() - tr;
        if (src_.failed()) return q_.fail(src_.error());
        uint64_t nl = 0;
        for (size_t i = had; i < segs.size(); ++i) {  // (the source counts from where it wrote)
          segs[i].begin += len, segs[i].end += len;
          nl += segs[i].lines;
        }
        len += got;
        lines += nl;
        total_bytes_ += got;
        total_lines_ += nl;
        if (total_lines_ > 1000) bytes_per_line_ = (double)total_bytes_ / (double)total_lines_;
        if (q_.stopped()) return;
      }
      char* const buf = q_.data(si);
      size_t cut = len;
      if (lines >= need) {
        // the byte behind the need-th newline
        uint64_t acc = 0;
        for (const FastqSource::LineRun& g : segs) {
          if (acc + g.lines < need) {
            acc += g.lines;
            continue;
          }
          const char* p = buf + g.begin;
          const char* e = buf + g.end;
          for (uint64_t k = acc; k < need; ++k) p = (const char*)memchr(p, '\n', (size_t)(e - p)) + 1;
          cut = (size_t)(p - buf);
          break;
        }
        if (cut < len) {
          carry_.assign(buf + cut, buf + len);
          carry_lines_ = lines - need;
        }
        lines = need;
      }
      Block b;
      b.data = buf;
      b.size = cut;
      b.first_record = seq * per_block_;
      b.lines = lines;
      b.final = at_end_ && carry_.empty();
      b.slot = si;
      b.seq = seq++;
      q_.publish(b);
      t_read_ += t_reading;
      t_cut_ += t_clock() - t1 - t_reading;
      ++t_blocks_;
      if (b.final) break;
    }
    q_.finish();
  }

  FastqSource src_;
  std::vector<char> carry_;  // read, not handed out yet
  uint64_t carry_lines_ = 0;
  bool at_end_ = false;
  uint64_t per_block_ = 1;
  double bytes_per_line_ = 64;
  uint64_t total_bytes_ = 0, total_lines_ = 0;
  static double t_clock() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  double t_wait_ = 0, t_read_ = 0, t_cut_ = 0;  // FQGPU_TIMING (the producer's; read after its join)
  uint64_t t_blocks_ = 0;
  PinnedQueue<Block> q_;  // (last: its threads are gone before anything they use)
};

}  // namespace fqhost
