// bam_input.h - what the drop-in programs that read a BAM file share (bam_add_tags, bam2fastq, bam_umi_count): how
// they leave, how they report, and the input side - the whole file read, its BGZF members inflated back to back
// (SAM/BAM specification, section 4.1), the alignment records found by their block_size fields.
#pragma once
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <string>

#include "../../include/fqg.h"
#include "fq_parallel.h"

namespace fqbam {

// How the program leaves: with everything it wrote flushed, and WITHOUT exit()'s hooks - the HIP runtime tears itself
// down in one of them, and now and then that ended a run that had printed all it had to print with a segmentation
// fault (status 139 instead of 0: seen once in 300 runs of the GPU suite).
[[noreturn]] inline void leave(int code) {
  fflush(nullptr);
  if (getenv("FQGPU_PLAIN_EXIT")) exit(code);  // (tools/exit_stress.py: does the process survive exit()'s hooks?)
  _exit(code);
}

#define PRINT_ERROR(...)          \
  do {                            \
    fprintf(stderr, "\nERROR: "); \
    fprintf(stderr, __VA_ARGS__); \
    fprintf(stderr, "\n");        \
  } while (0)

inline bool read_all(FILE* f, std::vector<uint8_t>& raw) {
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + k);
  return !ferror(f);
}

// the offsets of the alignment records of an inflated stream (one entry at least); false: not a BAM stream
inline bool index_records(const uint8_t* stream, size_t nbytes, std::vector<uint64_t>& offsets, uint64_t* n_rec, uint64_t* used) {
  if (fqg_bam_index_records(stream, nbytes, nullptr, 0, n_rec, used) != 0) return false;
  offsets.assign(*n_rec ? *n_rec : 1, 0);
  fqg_bam_index_records(stream, nbytes, offsets.data(), *n_rec, n_rec, used);  // (a record cut short ends the walk)
  return true;
}

// The input of a program in two steps (bam_umi_count says "Processing" and creates its files between them); each
// prints its message and leaves with status 2 when it fails.
//
// FQGPU_INFLATE_GPU=1 (and a context): the BGZF blocks are inflated on the device (fqg_bgzf_inflate, docs/host_gzip.md
// section 4).  The stream comes back once for the host's walk over the records and stays on the device, where the bulk
// calls read it (`device`: FQG_MEM_DEVICE, nothing is uploaded a second time).  A file the library's header walk refuses,
// or a block that does not inflate, is the message and the status of the host path: the two walks have the same rules,
// and the device's verdict on a block is zlib's.  A wrong CRC-32 is not looked at, as the host path (raw inflate) does
// not look at it.  FQGPU_INFLATE_DEBUG=1 says on stderr which inflate ran.
//
// FQGPU_INDEX_GPU=1, together with FQGPU_INFLATE_GPU=1 on that one context: the stream does not come back at all.  A prefix
// of it is fetched, and a longer one, until the header walk (fqg_bam_header_end) has its verdict; the records are indexed
// where they lie (fqg_bam_index_device, docs/host_gzip.md section 5).  `stream` then holds the HEADER alone, `offsets`
// stays empty until fetch_offsets, and the bulk calls read stream and offsets on the device (FQG_MEM_DEVICE_INDEXED).
// Same verdicts, same messages: the two header walks and the two record walks have the same rules.
// FQGPU_INDEX_DEBUG=1 says on stderr which index ran.
struct BamInput {
  std::vector<uint8_t> stream;    // the inflated file - with the index on the device: its header
  std::vector<uint64_t> offsets;  // of its alignment records
  uint64_t n_rec = 0, used = 0;   // how many; the end of the last complete one
  uint64_t total = 0;             // bytes of the inflated file
  uint64_t header_end = 0;        // where the first record starts, or would
  const uint8_t* device = nullptr;  // the inflated file on the device; null: it is in `stream` alone
  const uint64_t* device_offsets = nullptr;  // the offsets on the device; null: they are in `offsets` alone
  fqg_ctx* index_ctx = nullptr;   // the context that indexes on the device; null: the host does

  void inflate(FILE* in, const char* name, fqg_ctx* ctx = nullptr) {
    std::vector<uint8_t> raw;
    bool ok = read_all(in, raw);
    const char* e = getenv("FQGPU_INFLATE_GPU");
    const bool on_device = ctx && e && !strcmp(e, "1");
    unsigned long long n_blocks = 0;
    if (ok && on_device) {
      fqg_inflate_result r;
      int rc = fqg_bgzf_inflate(ctx, raw.data(), raw.size(), &r);
      if (rc == 0 && r.bad_block == UINT64_MAX) {
        const char* ix = getenv("FQGPU_INDEX_GPU");
        if (ix && !strcmp(ix, "1")) index_ctx = ctx;
        total = r.out_bytes;
        if (!index_ctx) {
          stream.resize(r.out_bytes);
          rc = fqg_inflate_output(ctx, 0, stream.data(), r.out_bytes);
        }
        device = static_cast<const uint8_t*>(fqg_inflate_device(ctx));
        n_blocks = r.n_blocks;
      } else if (rc == 0 || rc == FQG_ERR_ARG) ok = false;
      if (ok && rc != 0) {
        PRINT_ERROR("GPU library failure in fqg_bgzf_inflate (%d): %s", rc, fqg_last_error(ctx));
        leave(2);
      }
    } else if (ok) {
      size_t n = 0;
      ok = fqhost::bgzf_inflate_parallel(raw, stream, &n);
      n_blocks = n;
    }
    if (getenv("FQGPU_INFLATE_DEBUG")) {
      if (ok) fprintf(stderr, "[inflate] %s: %llu blocks\n", on_device ? "device" : "host", n_blocks);
      else fprintf(stderr, "[inflate] %s: refused\n", on_device ? "device" : "host");
    }
    if (!ok) {
      PRINT_ERROR("%s is not a readable BGZF / BAM file", name);
      leave(2);
    }
  }
  void index(const char* name) {
    bool ok = true;
    if (index_ctx) {
      uint64_t have = 0, need = 64u << 10;
      int rc = FQG_NEED_MORE;
      while (ok && rc == FQG_NEED_MORE) {  // (at least twice as much each time: a header is walked a few times at most)
        const uint64_t want = std::min<uint64_t>(total, std::max<uint64_t>(need, 2 * have));
        stream.resize(want);
        lib(fqg_inflate_output(index_ctx, have, stream.data() + have, want - have), "fqg_inflate_output");
        have = want;
        rc = fqg_bam_header_end(stream.data(), have, total, &header_end, &need);
        ok = rc == 0 || rc == FQG_NEED_MORE;
      }
      if (ok) {
        stream.resize(std::max(have, header_end));
        if (header_end > have) lib(fqg_inflate_output(index_ctx, have, stream.data() + have, header_end - have), "fqg_inflate_output");
        stream.resize(header_end);
        fqg_bam_index_result r;
        lib(fqg_bam_index_device(index_ctx, device, total, header_end, &r), "fqg_bam_index_device");
        n_rec = r.n_records;
        used = r.used;
        device_offsets = fqg_bam_index_offsets(index_ctx);
      }
    } else {
      total = stream.size();
      ok = index_records(stream.data(), stream.size(), offsets, &n_rec, &used);
      header_end = n_rec ? offsets[0] : used;
    }
    if (getenv("FQGPU_INDEX_DEBUG")) {
      if (ok) fprintf(stderr, "[index] %s: %llu records\n", index_ctx ? "device" : "host", (unsigned long long)n_rec);
      else fprintf(stderr, "[index] %s: refused\n", index_ctx ? "device" : "host");
    }
    if (!ok) {
      PRINT_ERROR("%s is not a BAM file", name);
      leave(2);
    }
  }
  // what the bulk calls take: the stream, where it and the offsets lie, the offsets from alignment `first` on
  const void* data() const { return device ? (const void*)device : (const void*)stream.data(); }
  int mem() const { return device_offsets ? FQG_MEM_DEVICE_INDEXED : device ? FQG_MEM_DEVICE : FQG_MEM_HOST; }
  const uint64_t* offs(uint64_t first = 0) const { return (device_offsets ? device_offsets : offsets.data()) + first; }
  // the offsets on the host as well (8 bytes per alignment), for a program that cuts the stream into pieces
  void fetch_offsets() {
    if (!device_offsets) return;
    offsets.assign(n_rec ? n_rec : 1, 0);
    lib(fqg_bam_index_output(index_ctx, 0, offsets.data(), n_rec), "fqg_bam_index_output");
  }
  // the C string at `pos` of the inflated file
  std::string c_string(uint64_t pos) {
    if (!device_offsets) return std::string((const char*)stream.data() + pos);
    std::vector<char> buf(std::min<uint64_t>(total - pos, 64u << 10) + 1, '\0');
    lib(fqg_inflate_output(index_ctx, pos, buf.data(), buf.size() - 1), "fqg_inflate_output");
    return std::string(buf.data());
  }

 private:
  void lib(int rc, const char* what) {
    if (rc == 0) return;
    PRINT_ERROR("GPU library failure in %s (%d): %s", what, rc, fqg_last_error(index_ctx));
    leave(2);
  }
};

}  // namespace fqbam
