// bam_input.h - what the drop-in programs that read a BAM file share (bam_add_tags, bam2fastq, bam_umi_count): how
// they leave, how they report, and the input side - the whole file read, its BGZF members inflated back to back
// (SAM/BAM specification, section 4.1), the alignment records found by their block_size fields.
#pragma once
#include <string.h>
#include <unistd.h>

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
struct BamInput {
  std::vector<uint8_t> stream;    // the inflated file
  std::vector<uint64_t> offsets;  // of its alignment records
  uint64_t n_rec = 0, used = 0;   // how many; the end of the last complete one
  const uint8_t* device = nullptr;  // the inflated file on the device; null: it is in `stream` alone

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
        stream.resize(r.out_bytes);
        rc = fqg_inflate_output(ctx, 0, stream.data(), r.out_bytes);
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
    if (!index_records(stream.data(), stream.size(), offsets, &n_rec, &used)) {
      PRINT_ERROR("%s is not a BAM file", name);
      leave(2);
    }
  }
};

}  // namespace fqbam
