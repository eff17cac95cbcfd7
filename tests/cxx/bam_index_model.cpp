// bam_index_model.cpp - the record index of fqg_bam_index_device on the CPU: fastq_utils_amd/csrc/fqg_bam_index_core.h run
// the way fqg_bam_index_kernels.hip runs it - windows, one segment at a time resolved backwards in chunks, thirty-six
// positions per round (all of a round resolved BEFORE any of them is stored, as the lanes of a wavefront do), the ring,
// the follower, the stretches - with every buffer allocated to its exact size, so that a sanitizer sees any index the
// kernels would get wrong.
//
//   bam_index_model <pack> <out> <seg> <window> <ring>
// pack: per stream u64 nbytes, u64 first_record, the bytes.  out: per stream u64 n, u64 used, n offsets.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../../fastq_utils_amd/csrc/fqg_bam_index_core.h"

using namespace fqg::bx;

namespace {

constexpr uint64_t kChunk = 4096;  // kBxChunk

struct Index {
  uint64_t n = 0, used = 0;
  std::vector<uint64_t> offsets;
};

void tables(const uint8_t* stream, uint64_t nbytes, uint64_t w_lo, uint64_t w_hi, uint64_t seg, uint32_t ring, uint32_t* entries,
            uint16_t* counts) {
  for (uint64_t seg_lo = w_lo; seg_lo < w_hi; seg_lo += seg) {  // (a workgroup each)
    const uint64_t seg_hi = std::min(seg_lo + seg, w_hi);
    std::unique_ptr<uint32_t[]> ring_entry(new uint32_t[ring]);
    std::unique_ptr<uint16_t[]> ring_count(new uint16_t[ring]);
    for (uint64_t c_hi = seg_hi; c_hi > seg_lo;) {
      const uint64_t c_lo = c_hi - seg_lo > kChunk ? c_hi - kChunk : seg_lo;
      const uint64_t c_end = std::min(c_hi + 3, nbytes);
      std::unique_ptr<uint8_t[]> stage(new uint8_t[c_end - c_lo]);  // exactly the bytes of the stream a chunk may look at
      memcpy(stage.get(), stream + c_lo, c_end - c_lo);
      for (uint64_t top = c_hi; top > c_lo;) {
        const uint64_t g_lo = top - c_lo > kBxMinStep ? top - kBxMinStep : c_lo;
        uint32_t e[kBxMinStep];
        uint16_t n[kBxMinStep];
        for (uint64_t lane = 0; lane < top - g_lo; ++lane) {
          const uint64_t q = top - 1 - lane;
          bx_resolve(q, seg_lo, seg_hi, nbytes, stage.get() + (q - c_lo), ring_entry.get(), ring_count.get(), ring, &e[lane], &n[lane]);
        }
        for (uint64_t lane = top - g_lo; lane-- > 0;) {  // (the stores in the other order: no lane may depend on it)
          const uint64_t q = top - 1 - lane;
          ring_entry[(uint32_t)q & (ring - 1)] = e[lane];
          ring_count[(uint32_t)q & (ring - 1)] = n[lane];
          entries[q - w_lo] = e[lane];
          counts[q - w_lo] = n[lane];
        }
        top = g_lo;
      }
      c_hi = c_lo;
    }
  }
}

Index index_stream(const uint8_t* stream, uint64_t nbytes, uint64_t first, uint64_t seg, uint64_t window, uint32_t ring) {
  Index out;
  const uint64_t span = nbytes - first, cap = span / kBxMinStep + 1;
  std::unique_ptr<uint64_t[]> offsets(new uint64_t[cap]);
  BxState s;
  memset(&s, 0, sizeof(s));
  s.p = first;
  for (uint64_t w_lo = first; w_lo < nbytes; w_lo += window) {
    const uint64_t w_hi = std::min(nbytes, w_lo + window), win = w_hi - w_lo;
    std::unique_ptr<uint32_t[]> entries(new uint32_t[win]);
    std::unique_ptr<uint16_t[]> counts(new uint16_t[win]);
    const uint64_t stretch_cap = bx_max_stretches(win, seg, ring);
    std::unique_ptr<BxStretch[]> stretch(new BxStretch[stretch_cap]);
    tables(stream, nbytes, w_lo, w_hi, seg, ring, entries.get(), counts.get());
    bx_follow(&s, stream, nbytes, w_lo, w_hi, seg, entries.get(), counts.get(), stretch.get(), stretch_cap);
    if (s.overflow) {
      fprintf(stderr, "the stretches of a window did not fit\n");
      exit(4);
    }
    for (uint32_t t = 0; t < s.n_stretch; ++t) bx_write_stretch(stretch[t], stream, nbytes, offsets.get(), cap);
  }
  out.n = s.k;
  out.used = s.p;
  if (out.n > cap) {
    fprintf(stderr, "more records than the stream has room for\n");
    exit(4);
  }
  out.offsets.assign(offsets.get(), offsets.get() + out.n);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: bam_index_model <pack> <out> <seg> <window> <ring>\n");
    return 2;
  }
  const uint64_t seg = strtoull(argv[3], nullptr, 10), window = strtoull(argv[4], nullptr, 10);
  const uint32_t ring = (uint32_t)strtoul(argv[5], nullptr, 10);
  if (seg < 64 || seg > kBxMaxSeg || window < seg || window % seg || ring < kBxMinRing || ring > kBxMaxRing || (ring & (ring - 1))) {
    fprintf(stderr, "geometry the library does not use\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  uint64_t head[2], n_streams = 0;
  while (fread(head, 8, 2, in) == 2) {
    // the stream in a buffer of exactly its size
    std::unique_ptr<uint8_t[]> stream(new uint8_t[head[0]]);
    if (head[0] && fread(stream.get(), 1, head[0], in) != head[0]) return 2;
    if (head[1] > head[0]) return 2;
    const Index ix = index_stream(stream.get(), head[0], head[1], seg, window, ring);
    const uint64_t res[2] = {ix.n, ix.used};
    fwrite(res, 8, 2, out);
    if (ix.n) fwrite(ix.offsets.data(), 8, ix.n, out);
    ++n_streams;
  }
  fclose(out);
  printf("streams %llu\n", (unsigned long long)n_streams);
  return 0;
}
