// span_fit_check.cpp - span_units / span_fits (fastq_utils_amd/csrc/fqg_fastq_tile.h, the text the kernels compile): the
// one rule by which k_bc_plan_tile, k_rf_tile_flags and k_split_tile_flags FLAG a tile and by which the emit kernels count
// the 16-byte units they LAND in LDS.
//
// One file, against the rule restated here in bytes (divisions, no shifts): a span of n bytes whose first byte lies s
// bytes behind a 16-byte boundary covers the bytes [0, roundup16(s + n)) of the input area, the lane writers read up to
// 32 bytes behind a line, and a span longer than the area is refused whatever its units:
//   every skew 0..15, in_cap over every multiple of 16 from 48 to 4096,
//   n in {0, 1, 15, 16, 17} and from in_cap - 64 to in_cap + 16
// and wherever the rule says "fits", 16 * units <= in_cap - 32: the landing loops store units [0, units), nothing at or
// past in_cap.
// Two and three files numbered through (the running total of bc_span_plan and bc_emit_tile_fits): the AND over the files
// of what span_fits answers refuses exactly when the restated sum does - some file longer than the area, or the units of
// the files that are not, together, past in_cap - 32.
// Prints the counts; exit status 1 on the first difference.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../fastq_utils_amd/csrc/fqg_fastq_tile.h"

static uint64_t roundup16(uint64_t x) { return (x + 15) / 16 * 16; }

// the restatement: bytes of the input area the span takes, or -1 where it is longer than the area
static int64_t bytes_taken(uint32_t s, uint64_t n, uint32_t in_cap) {
  if (n > in_cap) return -1;
  return (int64_t)roundup16((uint64_t)s + n);
}

static int fail(const char* what, uint32_t s, uint64_t n, uint32_t in_cap) {
  printf("FAIL %s: skew=%u n=%llu in_cap=%u\n", what, s, (unsigned long long)n, in_cap);
  return 1;
}

int main() {
  uint64_t fits = 0, refused = 0, multi_fits = 0, multi_refused = 0;
  for (uint32_t in_cap = 48; in_cap <= 4096; in_cap += 16) {
    std::vector<uint64_t> ns = {0, 1, 15, 16, 17};
    for (int64_t n = (int64_t)in_cap - 64; n <= (int64_t)in_cap + 16; ++n)
      if (n >= 0) ns.push_back((uint64_t)n);
    for (uint32_t s = 0; s < 16; ++s)
      for (uint64_t n : ns) {
        const int64_t taken = bytes_taken(s, n, in_cap);
        const bool want = taken >= 0 && (uint64_t)taken + 32 <= in_cap;
        uint32_t units = 0;
        const bool got = fqg::span_fits(s, n, in_cap, units);
        if (got != want) return fail("one file", s, n, in_cap);
        if (taken >= 0 && (units != fqg::span_units(s, (uint32_t)n) || 16ull * units != (uint64_t)taken))
          return fail("units", s, n, in_cap);
        if (taken < 0 && units != 0) return fail("units of a refused span", s, n, in_cap);
        if (got && 16ull * units > (uint64_t)in_cap - 32) return fail("a store at or past in_cap", s, n, in_cap);
        ++(got ? fits : refused);
      }
  }
  // several files numbered through
  static const uint32_t kCaps[] = {48, 64, 256, 1024, 4096}, kSkews[] = {0, 1, 15};
  for (uint32_t in_cap : kCaps) {
    std::vector<uint64_t> ns = {0, 1, 15, 16, 17, (uint64_t)in_cap, (uint64_t)in_cap + 1};
    for (int part = 2; part <= 3; ++part)
      for (int64_t n = (int64_t)(in_cap / part) - 24; n <= (int64_t)(in_cap / part) + 2; ++n)
        if (n >= 0) ns.push_back((uint64_t)n);
    for (int files = 2; files <= 3; ++files) {
      const size_t per = ns.size() * 3;  // (n, skew) of one file
      size_t total = 1;
      for (int f = 0; f < files; ++f) total *= per;
      for (size_t c = 0; c < total; ++c) {
        size_t rest = c;
        uint32_t units = 0;
        bool got = true, too_long = false;
        uint64_t sum = 0;
        for (int f = 0; f < files; ++f) {
          const uint64_t n = ns[rest % per / 3];
          const uint32_t s = kSkews[rest % per % 3];
          rest /= per;
          if (!fqg::span_fits(s, n, in_cap, units)) got = false;  // (as bc_span_plan: every file is asked)
          const int64_t taken = bytes_taken(s, n, in_cap);
          if (taken < 0) too_long = true;
          else sum += (uint64_t)taken;
        }
        const bool want = !too_long && sum + 32 <= in_cap;
        if (got != want) return fail(files == 2 ? "two files" : "three files", 0, c, in_cap);
        if (got && 16ull * units > (uint64_t)in_cap - 32) return fail("a store at or past in_cap (files)", 0, c, in_cap);
        ++(got ? multi_fits : multi_refused);
      }
    }
  }
  printf("fits=%llu refused=%llu multi_fits=%llu multi_refused=%llu\n", (unsigned long long)fits, (unsigned long long)refused,
         (unsigned long long)multi_fits, (unsigned long long)multi_refused);
  return 0;
}
