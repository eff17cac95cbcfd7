// mark_pack_check.cpp - pack_marks32 (fastq_utils_amd/csrc/fqg_mark_pack.h, the text the streaming kernel compiles, the dot
// product restated for the host) against a restatement of the form it replaced - two 16-bit halves, each
// (lo >> 7) | (hi << 1) over two dot-product pairs, joined as lo | (hi << 16) - and against a byte loop.
//
//   single  one mark at each of the 32 byte positions
//   pair    every pair of positions (496)
//   all / none
//   random  200 000 random patterns, a third of them sparse and a third dense
// Prints the counts; exit status 1 on the first difference.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../fastq_utils_amd/csrc/fqg_mark_pack.h"

// what the kernel computed before: pack_marks16() twice
static uint32_t old_pack16(uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3) {
  uint32_t lo = fqg::udot4_u8(m0, 0x08040201u, 0u);
  lo = fqg::udot4_u8(m1, 0x80402010u, lo);
  uint32_t hi = fqg::udot4_u8(m2, 0x08040201u, 0u);
  hi = fqg::udot4_u8(m3, 0x80402010u, hi);
  return (lo >> 7) | (hi << 1);
}
static uint32_t old_pack32(const uint32_t (&m)[8]) { return old_pack16(m[0], m[1], m[2], m[3]) | (old_pack16(m[4], m[5], m[6], m[7]) << 16); }

// ... and what both must be, byte by byte
static uint32_t plain_pack32(const uint32_t (&m)[8]) {
  uint32_t out = 0;
  for (int i = 0; i < 32; ++i)
    if ((m[i >> 2] >> (8 * (i & 3))) & 0x80u) out |= 1u << i;
  return out;
}

static unsigned long long g_cases = 0;

// bits: which of the 32 bytes carry a mark (0x80)
static bool check(uint32_t bits) {
  uint32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 32; ++i)
    if ((bits >> i) & 1u) m[i >> 2] |= 0x80u << (8 * (i & 3));
  const uint32_t got = fqg::pack_marks32(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7]);
  const uint32_t old = old_pack32(m), plain = plain_pack32(m);
  ++g_cases;
  if (got != old || got != plain || got != bits) {
    std::printf("marks %08x: pack_marks32 %08x, two pack_marks16 %08x, byte by byte %08x\n", bits, got, old, plain);
    return false;
  }
  return true;
}

int main() {
  if (!check(0u) || !check(~0u)) return 1;
  unsigned long long single = 0, pair = 0, random = 0;
  for (int i = 0; i < 32; ++i) {
    if (!check(1u << i)) return 1;
    ++single;
    for (int j = i + 1; j < 32; ++j) {
      if (!check((1u << i) | (1u << j))) return 1;
      ++pair;
    }
  }
  std::mt19937 rng(20240611u);
  for (int n = 0; n < 200000; ++n) {
    uint32_t x = rng();
    if (n % 3 == 1) x &= rng() & rng();
    if (n % 3 == 2) x |= rng() | rng();
    if (!check(x)) return 1;
    ++random;
  }
  std::printf("single=%llu pair=%llu random=%llu cases=%llu\n", single, pair, random, g_cases);
  return 0;
}
