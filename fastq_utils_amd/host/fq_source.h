// fq_source.h - a FASTQ input one can read inflated bytes from: "-" (stdin), a plain file, a bgzip'd file, any other
// gzip file.  Opened once, as the reference opens it (fastq_open, src/fastq.c:631-661), and read by whoever stages it
// for the GPU: the ring of fq_input.h, the cutters of fq_multi.h and fq_blocks.h.  Needs nothing of the library.
//
// A plain (not gzipped) regular file is read with pread() by several threads at once - 50 Mreads/s of 150 bp reads are
// 17.5 GB/s, more than one core copies.  A gzip file is inflated on every core the process may use: a bgzip'd one block
// by block (read_bgzf, where the owner asks for it), any other one by chunks whose first blocks are searched for
// (fq_pgzip.h); stdin and small files by one zlib thread.
//
// One thread reads at a time.  An error is recorded here (failed() / error()) and the read returns: the owner looks
// after every call and tells its consumers in its own way.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "fq_parallel.h"
#include "fq_pgzip.h"
#include "fq_respawn.h"

namespace fqhost {

// src/fastq.h:68-80
#define FQ_PRINT_ERROR(...)       \
  do {                            \
    fprintf(stderr, "\nERROR: "); \
    fprintf(stderr, __VA_ARGS__); \
    fprintf(stderr, "\n");        \
  } while (0)
#define FQ_PRINT_INFO(...)        \
  do {                            \
    fprintf(stderr, "INFO:");     \
    fprintf(stderr, __VA_ARGS__); \
    fprintf(stderr, "\n");        \
  } while (0)
constexpr int kExitParams = 1, kExitSys = 2, kExitFormat = 3;

// How the programs leave: with everything they said flushed, and WITHOUT exit()'s hooks.  The HIP runtime tears itself
// down in one of them, and it must not meet a thread of ours that is still inside a HIP call (a reader pinning its next
// slot while the main thread has found the file's first error): that is a crash after the error message, i.e. a wrong
// exit status.  Nothing is lost: outputs are closed by those who write them before they leave.
[[noreturn]] inline void leave(int code) {
  fflush(stdout);
  fflush(stderr);
  if (getenv("FQGPU_PLAIN_EXIT")) exit(code);  // (tools/exit_stress.py: does the process survive exit()'s hooks?)
  _exit(code);
}

inline unsigned host_read_threads() {
  if (const char* e = getenv("FQGPU_HOST_THREADS")) return (unsigned)std::max(1L, strtol(e, nullptr, 10));
  const unsigned hw = std::thread::hardware_concurrency();
  // (a dozen copy a tmpfs file faster than PCIe takes it; more of them only compete with the DMA for host memory:
  // 8 / 16 / 32 / 64 threads -> 1.06 / 1.16 / 1.24 / 1.46 s for the 100 M-read file of the bench)
  return std::max(1u, std::min(12u, hw ? hw : 1u));
}

// (ReaderPool - a few threads that stay around - lives in fq_parallel.h)

// gzip files below this size stay with one zlib thread (FQGPU_PGZIP_MIN: tests send tiny files through the chunked reader)
inline uint64_t pgzip_min_bytes() {
  if (const char* e = getenv("FQGPU_PGZIP_MIN")) return (uint64_t)std::max(0L, atol(e));
  return 1u << 20;
}

// The many-core reader for the gzip file open on fd (fq_pgzip.h), or nothing when one zlib thread is to read it: small
// files, a single usable core, FQGPU_NO_PARALLEL_INFLATE.  (What that reader does not want to decide it leaves to one
// zlib stream of its own, so every file gzopen reads is read.)
inline std::unique_ptr<ParallelGunzip> open_pgzip(int fd, uint64_t size, const char* path) {
  if (size < pgzip_min_bytes() || host_threads() <= 1 || getenv("FQGPU_NO_PARALLEL_INFLATE")) return nullptr;
  const unsigned T = std::min(host_threads(), 64u);
  // (tools/pgzip_scan.sh on the 16-core share of an EPYC 9575F: 2.6 / 3.0 / 3.5 GB/s inflated with chunks of 1 / 2 / 4 MiB)
  size_t chunk = std::max<size_t>(512u << 10, std::min<size_t>(4u << 20, (128u << 20) / T));
  chunk = std::min<size_t>(chunk, std::max<size_t>((size_t)size / T, 128u << 10));
  if (const char* e = getenv("FQGPU_PGZIP_CHUNK")) chunk = (size_t)std::max(4096L, atol(e));
  return std::unique_ptr<ParallelGunzip>(new ParallelGunzip(fd, size, path, T, chunk));
}
inline void pgzip_report(const ParallelGunzip* pg, const std::string& path) {
  if (!pg || !(getenv("FQGPU_PGZIP_DEBUG") || getenv("FQGPU_TIMING"))) return;
  const ParallelGunzip::Stats& st = pg->stats();
  fprintf(fqhost::diag(), "fqgpu timing: %s inflated by chunks: %llu rounds, %llu chunks joined, %llu without a block start, %llu wrong guesses, "
          "%llu members%s%s; reading %.3f s, finding + inflating %.3f s, joining %.3f s, markers -> bytes + CRC-32 %.3f s\n",
          path.c_str(), (unsigned long long)st.batches, (unsigned long long)st.chunks_joined, (unsigned long long)st.chunks_not_found,
          (unsigned long long)st.chunks_discarded, (unsigned long long)st.members, st.fell_back ? "; one zlib stream from: " : "",
          st.fell_back ? st.why.c_str() : "", st.s_load, st.s_decode, st.s_join + st.s_windows, st.s_narrow);
}

class FastqSource {
 public:
  enum Kind { kStdin, kPlain, kBgzf, kPgzip, kZlib };
  struct Options {
    bool bgzf = false;       // a bgzip'd file has its blocks inflated side by side (read_bgzf); otherwise it is a gzip file like any other
    uint64_t limit = ~0ull;  // the input is taken to end after this many (inflated) bytes (whole blocks cannot end there: no read_bgzf then)
  };
  // a run of the bytes of one read() whose newline count is known; the runs of a read tile [0, its return value)
  struct LineRun {
    size_t begin, end;
    uint64_t lines;
  };
  typedef std::vector<LineRun> Lines;

  FastqSource(const char* path, const Options& opt) : path_(path), limit_(opt.limit) {
    // fastq_open, src/fastq.c:631-661
    if (path_ == "-") gz_ = gzdopen(fileno(stdin), "rb");
    else {
      // a regular file that does not start with the gzip magic is what zlib would pass through unchanged
      const int fd = open(path, O_RDONLY);
      struct stat sb;
      if (fd >= 0 && fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode)) {
        unsigned char magic[18];
        memset(magic, 0, sizeof(magic));
        const ssize_t got = pread(fd, magic, sizeof(magic), 0);
        file_bytes_ = (uint64_t)sb.st_size;
        if (!(got >= 2 && magic[0] == 0x1f && magic[1] == 0x8b)) {
          kind_ = kPlain;
          plain_size_ = std::min<uint64_t>(file_bytes_, limit_);
        } else if (opt.bgzf && opt.limit == ~0ull && got == 18 && bgzf_block_size(magic, 18) > 0 && !getenv("FQGPU_NO_PARALLEL_INFLATE")) {
          // bgzip'd FASTQ: a sequence of small gzip members that say how long they are (SAM/BAM specification 4.1) -
          // inflated on all cores (read_bgzf below) instead of by one zlib thread
          kind_ = kBgzf;
        } else if ((pgz_ = open_pgzip(fd, file_bytes_, path))) {
          kind_ = kPgzip;  // any other gzip file of some size: chunks of it are inflated side by side
        }
        if (kind_ != kZlib) fd_ = fd;
      }
      if (fd_ < 0) {
        if (fd >= 0) close(fd);
        gz_ = gzopen(path, "r");
      }
    }
    if (!gz_ && fd_ < 0) {
      FQ_PRINT_ERROR("Unable to open %s", path);
      leave(kExitParams);
    }
    if (gz_) gzbuffer(gz_, 1 << 20);
    if (path_ == "-") kind_ = kStdin;
  }
  // (the owner has joined whoever was reading)
  ~FastqSource() {
    if (gz_) gzclose(gz_);
    pgzip_report(pgz_.get(), path_);
    pgz_.reset();
    if (fd_ >= 0) close(fd_);
    free(bz_raw_);
  }
  FastqSource(const FastqSource&) = delete;
  FastqSource& operator=(const FastqSource&) = delete;

  Kind kind() const { return kind_; }
  bool inflated() const { return kind_ != kPlain; }  // (stdin too: it passes through zlib)
  // bytes of a regular file on disk, 0 for stdin and whatever else is no regular file
  uint64_t file_bytes() const { return file_bytes_; }
  // bytes of a plain (uncompressed, seekable) input up to the limit, 0 when unknown; what of them has not been read
  uint64_t plain_bytes() const { return kind_ == kPlain ? plain_size_ : 0; }
  uint64_t plain_left() const { return kind_ == kPlain ? plain_size_ - plain_off_ : 0; }
  const std::string& path() const { return path_; }
  bool failed() const { return failed_; }
  const std::string& error() const { return error_; }

  static uint64_t count_lines(const char* a, const char* b) {
    uint64_t c = 0;
    for (const char* p = a; (p = (const char*)memchr(p, '\n', (size_t)(b - p))) != nullptr; ++p) ++c;
    return c;
  }

  // Up to `want` bytes to dst; *at_end is set by the call that delivers the input's last byte (a bgzip'd input delivers
  // whole blocks: fewer than 64 KiB short of `want` is "full", and `want` must hold a block).  With `lines`, the
  // newlines are counted as well - by the threads that read, while the bytes are in their cache - and the runs they
  // counted are appended, positions relative to dst.
  size_t read(char* dst, size_t want, bool* at_end, Lines* lines = nullptr) {
    if (kind_ == kPlain) return read_plain(dst, want, at_end, lines);
    want = (size_t)std::min<uint64_t>(want, limit_ - total_);
    size_t len = 0;
    if (kind_ == kBgzf) len = read_bgzf(dst, want, at_end);
    else if (pgz_) {
      len = pgz_->read(dst, want, at_end);
      if (pgz_->failed()) fail(pgz_->error().c_str());  // (zlib's text, as gzerror gives it)
    } else {
      while (len < want) {
        const int got = gzread(gz_, dst + len, (unsigned)std::min<size_t>(want - len, 1u << 30));
        if (got < 0) {
          int en = 0;
          fail(gzerror(gz_, &en));
          break;
        }
        if (got == 0) {
          *at_end = true;
          break;
        }
        len += (size_t)got;
      }
    }
    if (failed_) return len;
    total_ += len;
    if (total_ >= limit_) *at_end = true;
    if (!*at_end && gz_) {
      const int c = gzgetc(gz_);  // a file that ends exactly where the buffer does
      if (c < 0) *at_end = true;
      else gzungetc(c, gz_);
    }
    if (lines && len) lines->push_back(LineRun{0, len, count_lines(dst, dst + len)});
    return len;
  }

 private:
  void fail(const char* what) {
    error_ = what;
    failed_ = true;
  }
  // `n` bytes of the file from `off` to dst, by up to host_read_threads() threads of `pool`, each a page-aligned part;
  // with `runs`, in steps of 256 KiB whose lines are counted while the bytes are still in the reading core's cache
  // (counting a part after reading all of it is a second pass over memory).  false: a read failed.
  bool pread_parts(std::unique_ptr<ReaderPool>& pool, unsigned threads, char* dst, size_t n, uint64_t off, Lines* runs) {
    const unsigned T = (unsigned)std::min<uint64_t>(threads, std::max<uint64_t>(1, n >> 22));
    const size_t step = runs ? (size_t)256u << 10 : ~(size_t)0;
    std::vector<uint64_t> cnt(T, 0);
    std::atomic<bool> bad{false};
    auto bound = [&](unsigned t) { return t == T ? n : (n * t / T) & ~(size_t)4095; };
    auto part = [&](unsigned t) {
      size_t done = bound(t);
      const size_t b = bound(t + 1);
      while (done < b) {
        const ssize_t got = pread(fd_, dst + done, std::min(b - done, step), (off_t)(off + done));
        if (got <= 0) {
          bad = true;
          return;
        }
        if (runs) cnt[t] += count_lines(dst + done, dst + done + (size_t)got);
        done += (size_t)got;
      }
    };
    if (T <= 1) part(0);
    else {
      if (!pool) pool.reset(new ReaderPool(threads));
      pool->run(T, part);
    }
    if (bad) return false;
    for (unsigned t = 0; runs && t < T; ++t)
      if (bound(t + 1) > bound(t)) runs->push_back(LineRun{bound(t), bound(t + 1), cnt[t]});
    return true;
  }
  size_t read_plain(char* dst, size_t want, bool* at_end, Lines* lines) {
    const size_t len = (size_t)std::min<uint64_t>(want, plain_size_ - plain_off_);
    if (!pread_parts(pool_, host_read_threads(), dst, len, plain_off_, lines)) {
      fail("read error");
      return 0;
    }
    plain_off_ += len;
    if (plain_off_ >= plain_size_) *at_end = true;
    return len;
  }

  // ---- BGZF input (bgzip'd FASTQ; SAM/BAM specification 4.1) ------------------------------------------------------
  // total size of the block that starts at p when p is a BGZF block header (gzip member, FEXTRA with the 'B' 'C'
  // subfield), 0 otherwise
  static size_t bgzf_block_size(const unsigned char* p, size_t avail) {
    if (avail < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
    const size_t xlen = p[10] | ((size_t)p[11] << 8);
    size_t q = 12;
    while (q + 4 <= 12 + xlen && q + 4 <= avail) {
      const size_t slen = p[q + 2] | ((size_t)p[q + 3] << 8);
      if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && q + 6 <= avail) {
        const size_t bsize = (p[q + 4] | ((size_t)p[q + 5] << 8)) + 1;
        return bsize >= 12 + xlen + 8 ? bsize : 0;
      }
      q += 4 + slen;
    }
    return 0;
  }
  // up to `want` inflated bytes: compressed bytes are read in pieces of 32 MiB, the blocks in them are listed
  // (their sizes are in their headers and trailers) and every block is inflated to its own place, many at a time.
  // Whole blocks only: fewer than 64 KiB short of `want` is "full".
  size_t read_bgzf(char* dst, size_t want, bool* at_end) {
    struct Block {
      size_t at, size, xlen, out_at, isize;
    };
    size_t len = 0;
    for (;;) {
      // refill the compressed window [bz_at_, bz_buf_.size()): what is left of it to the front, then up to 128 MiB of
      // the file behind it, read by the pool (one thread reads a tmpfs file at a few GB/s - less than the pool inflates)
      if (bz_buf_.size() - bz_at_ < (1u << 17) && bgzf_off_ < file_bytes_) {
        if (!inflate_pool_) {
          inflate_pool_.reset(new ReaderPool(host_threads()));  // (fq_parallel.h: the cores this process may use)
        }
        const size_t old = bz_buf_.size() - bz_at_, add = (size_t)std::min<uint64_t>(128u << 20, file_bytes_ - bgzf_off_);
        if (bz_raw_cap_ < old + add) {  // (plain memory, never zero-filled: a vector's resize would write it first)
          unsigned char* nb = static_cast<unsigned char*>(malloc(old + (128u << 20)));
          if (!nb) {
            fail("out of memory");
            return len;
          }
          if (old) memcpy(nb, bz_buf_.data() + bz_at_, old);
          free(bz_raw_);
          bz_raw_ = nb;
          bz_raw_cap_ = old + (128u << 20);
        } else if (old) memmove(bz_raw_, bz_buf_.data() + bz_at_, old);
        if (!pread_parts(inflate_pool_, inflate_pool_->size(), reinterpret_cast<char*>(bz_raw_) + old, add, bgzf_off_, nullptr)) {
          fail("read error");
          return len;
        }
        bz_buf_ = Span{bz_raw_, old + add};
        bz_at_ = 0;
        bgzf_off_ += add;
      }
      if (bz_at_ == bz_buf_.size()) {
        *at_end = true;
        return len;
      }
      std::vector<Block> blocks;
      size_t p = bz_at_, total = 0;
      while (p < bz_buf_.size()) {
        const size_t bsize = bgzf_block_size(bz_buf_.data() + p, bz_buf_.size() - p);
        if (!bsize) {
          if (bz_buf_.size() - p < 18 && bgzf_off_ < file_bytes_) break;  // a header cut by the window: next round
          fail("not a BGZF block where one was expected (a bgzip'd file followed by other data?)");
          return len;
        }
        if (p + bsize > bz_buf_.size()) {
          if (bgzf_off_ < file_bytes_) break;
          fail("truncated BGZF block");
          return len;
        }
        const unsigned char* t = bz_buf_.data() + p + bsize - 4;
        const size_t isize = (size_t)t[0] | ((size_t)t[1] << 8) | ((size_t)t[2] << 16) | ((size_t)t[3] << 24);
        if (isize > 65536) {
          fail("BGZF block larger than 64 KiB");
          return len;
        }
        if (len + total + isize > want) break;
        const size_t xlen = bz_buf_[p + 10] | ((size_t)bz_buf_[p + 11] << 8);
        blocks.push_back({p, bsize, xlen, len + total, isize});
        total += isize;
        p += bsize;
      }
      if (blocks.empty()) {
        if (p < bz_buf_.size() && bgzf_off_ >= file_bytes_ && len + 65536 > want) return len;  // no room for the next block
        if (p < bz_buf_.size() && len + 65536 > want) return len;
        if (p >= bz_buf_.size() && bgzf_off_ >= file_bytes_) {
          *at_end = true;
          return len;
        }
        if (bz_buf_.size() - bz_at_ >= (1u << 17)) return len;  // (cannot be: a window of 128 KiB holds a block)
        continue;
      }
      // (inflating is all this input costs - zlib gives a few hundred MB/s per core, the GPU takes tens of GB/s: every
      // core the host has, FQGPU_HOST_THREADS caps it)
      const unsigned T = (unsigned)std::min<size_t>(inflate_pool_->size(), std::max<size_t>(1, blocks.size() / 4));
      std::atomic<bool> bad{false};
      const unsigned char* src = bz_buf_.data();
      inflate_pool_->run(T, [&](unsigned t) {
        z_stream zs;  // one inflate state per thread and batch, reset per block (setting one up allocates its window)
        memset(&zs, 0, sizeof(zs));
        if (inflateInit2(&zs, -15) != Z_OK) {
          bad = true;
          return;
        }
        for (size_t i = blocks.size() * t / T; i < blocks.size() * (t + 1) / T && !bad; ++i) {
          const Block& b = blocks[i];
          if (b.isize == 0) continue;  // (the end-of-file marker, or an empty block)
          if (inflateReset(&zs) != Z_OK) {
            bad = true;
            break;
          }
          zs.next_in = const_cast<Bytef*>(src + b.at + 12 + b.xlen);
          zs.avail_in = (uInt)(b.size - 12 - b.xlen - 8);
          zs.next_out = reinterpret_cast<Bytef*>(dst + b.out_at);
          zs.avail_out = (uInt)b.isize;
          const int rc = inflate(&zs, Z_FINISH);
          const bool good = rc == Z_STREAM_END && zs.total_out == b.isize;
          const unsigned char* c = src + b.at + b.size - 8;
          const uint32_t want_crc = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
          if (!good || (uint32_t)crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef*>(dst + b.out_at), (uInt)b.isize) != want_crc)
            bad = true;
        }
        inflateEnd(&zs);
      });
      if (bad) {
        fail("corrupt BGZF block (inflate or CRC-32 failed)");
        return len;
      }
      len += total;
      bz_at_ = p;
      if (bz_at_ == bz_buf_.size() && bgzf_off_ >= file_bytes_) {
        *at_end = true;
        return len;
      }
      if (len + 65536 > want) return len;
    }
  }

  std::string path_;
  Kind kind_ = kZlib;
  gzFile gz_ = nullptr;  // stdin, small gzip files, whatever is no regular file: one zlib thread
  int fd_ = -1;          // a regular file read with pread(): plain, bgzip'd (read_bgzf) or inflated by chunks (fq_pgzip.h)
  uint64_t file_bytes_ = 0;
  uint64_t plain_size_ = 0, plain_off_ = 0;
  uint64_t limit_, total_ = 0;  // (inflated input: bytes handed out so far)
  std::unique_ptr<ParallelGunzip> pgz_;
  uint64_t bgzf_off_ = 0;
  struct Span {  // the compressed window (bytes of bz_raw_)
    const unsigned char* p = nullptr;
    size_t n = 0;
    const unsigned char* data() const { return p; }
    size_t size() const { return n; }
    unsigned char operator[](size_t i) const { return p[i]; }
  } bz_buf_;
  unsigned char* bz_raw_ = nullptr;
  size_t bz_raw_cap_ = 0, bz_at_ = 0;
  std::unique_ptr<ReaderPool> pool_, inflate_pool_;
  bool failed_ = false;
  std::string error_;
};

}  // namespace fqhost
