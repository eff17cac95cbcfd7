// mark_pack_wave_check.cpp - pack_marks32_wave (fastq_utils_amd/csrc/fqg_mark_pack.h: the pack of a whole wavefront through
// two v_mfma_i32_16x16x64_i8, the instruction restated for the host with its lane layout) against pack_marks32, lane by
// lane.
//
//   all / none   every mark of every lane set, and none
//   single       every mark position of every lane (64 x 32), once with the other 63 lanes all-ones and once with them
//                all-zero: a product that reaches a lane from lane j + 16, j + 32 or j + 48, or from another weight row of
//                its group of four, shows here
//   random       100 000 random wavefronts, a third of them sparse and a third dense
// Prints the counts; exit status 1 on the first difference.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../fastq_utils_amd/csrc/fqg_mark_pack.h"

static unsigned long long g_cases = 0;

// bits[l]: which of the 32 bytes of lane l carry a mark (0x80)
static bool check(const uint32_t (&bits)[64]) {
  uint32_t m[64][8], got[64];
  for (int l = 0; l < 64; ++l)
    for (int w = 0; w < 8; ++w) {
      m[l][w] = 0;
      for (int i = 0; i < 4; ++i)
        if ((bits[l] >> (4 * w + i)) & 1u) m[l][w] |= 0x80u << (8 * i);
    }
  fqg::pack_marks32_wave(m, got);
  ++g_cases;
  for (int l = 0; l < 64; ++l) {
    const uint32_t want = fqg::pack_marks32(m[l][0], m[l][1], m[l][2], m[l][3], m[l][4], m[l][5], m[l][6], m[l][7]);
    if (got[l] != want || got[l] != bits[l]) {
      std::printf("lane %d, marks %08x: pack_marks32_wave %08x, pack_marks32 %08x\n", l, bits[l], got[l], want);
      return false;
    }
  }
  return true;
}

int main() {
  uint32_t bits[64];
  for (uint32_t fill : {0u, ~0u}) {
    for (int l = 0; l < 64; ++l) bits[l] = fill;
    if (!check(bits)) return 1;
  }
  unsigned long long single = 0, random = 0;
  for (uint32_t others : {~0u, 0u})
    for (int lane = 0; lane < 64; ++lane)
      for (int i = 0; i < 32; ++i) {
        for (int l = 0; l < 64; ++l) bits[l] = others;
        bits[lane] = 1u << i;
        if (!check(bits)) return 1;
        ++single;
      }
  std::mt19937 rng(20240612u);
  for (int n = 0; n < 100000; ++n) {
    for (int l = 0; l < 64; ++l) {
      uint32_t x = rng();
      if (n % 3 == 1) x &= rng() & rng();
      if (n % 3 == 2) x |= rng() | rng();
      bits[l] = x;
    }
    if (!check(bits)) return 1;
    ++random;
  }
  std::printf("single=%llu random=%llu cases=%llu\n", single, random, g_cases);
  return 0;
}
