// type_spans_check.cpp - the span form of the line-type masks (fastq_utils_amd/csrc/fqg_type_spans.h, the text the
// streaming kernel compiles) against a restatement of the form it replaced: the 2-bit running newline count of every
// byte from two prefix-XORs over the shifted newline mask, and the newline bytes taken out by the caller.
//
//   exact   every 32-bit mask with 0 - 3 set bits x the four types of the first byte: M1 and M3 identical
//   over    the return value is != 0 exactly when the mask has four or more bits: every 4-bit mask, and denser random ones
//   sparse  ... and 0 on every mask of the first group
// Prints the counts (the enumerated masks: 5 489 x 4 = 21 956 cases, C(32, 4) = 35 960 four-bit masks); exit status 1 on the first difference.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../fastq_utils_amd/csrc/fqg_type_spans.h"

static uint32_t prefix_xor32(uint32_t x) {
  x ^= x << 1;
  x ^= x << 2;
  x ^= x << 4;
  x ^= x << 8;
  x ^= x << 16;
  return x;
}

// what the kernel computed before: type_masks32() and the `& ~nl` of its caller
static void old_masks(uint32_t nl, uint32_t t0, uint32_t& M1, uint32_t& M3) {
  const uint32_t e = nl << 1;
  const uint32_t P = prefix_xor32(e);
  const uint32_t Q = prefix_xor32(e & ~P);
  const uint32_t a0 = 0u - (t0 & 1u), a1 = 0u - ((t0 >> 1) & 1u);
  const uint32_t L = P ^ a0;
  const uint32_t Hh = Q ^ a1 ^ (P & a0);
  M1 = (~Hh & L) & ~nl;
  M3 = (Hh & L) & ~nl;
}

// ... and what both must be, byte by byte
static void plain_masks(uint32_t nl, uint32_t t0, uint32_t& M1, uint32_t& M3) {
  M1 = M3 = 0;
  uint32_t t = t0 & 3u;
  for (int i = 0; i < 32; ++i) {
    if ((nl >> i) & 1u) {
      t = (t + 1u) & 3u;
      continue;
    }
    if (t == 1u) M1 |= 1u << i;
    if (t == 3u) M3 |= 1u << i;
  }
}

static unsigned long long g_exact = 0, g_over = 0;

static bool check_sparse(uint32_t x) {
  // (t beyond 3 too: the kernel passes t0 + ex[k] without masking it)
  for (uint32_t t = 0; t < 4; ++t) {
    for (uint32_t add = 0; add <= 252u; add += 252u) {
      uint32_t m1, m3, o1, o3, p1, p3;
      if (fqg::type_spans32(x, t + add, m1, m3) != 0u) {
        std::printf("type_spans32(%08x) says four or more newlines with %d bits\n", x, __builtin_popcount(x));
        return false;
      }
      old_masks(x, t + add, o1, o3);
      plain_masks(x, t + add, p1, p3);
      if (m1 != o1 || m3 != o3 || m1 != p1 || m3 != p3) {
        std::printf("x=%08x t=%u: span %08x %08x, two prefix-XORs %08x %08x, byte by byte %08x %08x\n", x, t + add, m1, m3, o1, o3,
                    p1, p3);
        return false;
      }
    }
    ++g_exact;
  }
  return true;
}

static bool check_dense(uint32_t x) {
  ++g_over;
  for (uint32_t t = 0; t < 4; ++t) {
    uint32_t m1, m3;
    if (fqg::type_spans32(x, t, m1, m3) == 0u) {
      std::printf("type_spans32(%08x) says at most three newlines with %d bits\n", x, __builtin_popcount(x));
      return false;
    }
  }
  return true;
}

int main() {
  if (!check_sparse(0u)) return 1;
  for (int i = 0; i < 32; ++i) {
    const uint32_t bi = 1u << i;
    if (!check_sparse(bi)) return 1;
    for (int j = i + 1; j < 32; ++j) {
      const uint32_t bj = bi | (1u << j);
      if (!check_sparse(bj)) return 1;
      for (int k = j + 1; k < 32; ++k) {
        const uint32_t bk = bj | (1u << k);
        if (!check_sparse(bk)) return 1;
        for (int l = k + 1; l < 32; ++l)
          if (!check_dense(bk | (1u << l))) return 1;
      }
    }
  }
  const unsigned long long exact_enumerated = g_exact, over_enumerated = g_over;
  std::mt19937 rng(20240607u);
  unsigned long long random_dense = 0;
  for (int n = 0; n < 20000; ++n) {
    uint32_t x = rng();
    if (n & 1) x &= rng();  // (a quarter of the bits: four or more in nearly every draw)
    if (n % 4 == 3) x &= rng();
    if (__builtin_popcount(x) >= 4) {
      ++random_dense;
      if (!check_dense(x)) return 1;
    } else if (!check_sparse(x)) {
      return 1;
    }
  }
  std::printf("exact_enumerated=%llu exact=%llu over_enumerated=%llu over=%llu random_dense=%llu\n", exact_enumerated, g_exact,
              over_enumerated, g_over, random_dense);
  return 0;
}
