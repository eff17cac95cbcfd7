// fqg_type_spans.h - line-type masks of 32 bytes from the SPANS between their newlines.
//
// A lane of the streaming pass (fqg_stream_kernels.hip) owns 32 contiguous bytes and their newline mask x, and knows
// the line type t (0 header, 1 sequence, 2 "+", 3 quality; mod 4) of its first byte.  The byte-class checks need M1 =
// the bytes on sequence lines and M3 = the bytes on quality lines, the newline that ends a line NOT included.
//
// With b0 < b1 < b2 the three lowest set bits of x (0 where x has fewer) and m_j = b_j - 1 the bits below b_j (all 32
// where it is absent), the line that the j-th newline ends covers
//     D0 = m0      D1 = m1 & ~(m0 | b0)      D2 = m2 & ~(m1 | b1)      D3 = ~(m2 | b2)
// D0 starts at bit 0, D3 runs to bit 31; an absent newline makes its own span reach bit 31 and the ones behind it empty.
// Line j has type t + j, so M1 = D[(1 - t) & 3] and M3 = D[(3 - t) & 3].  That is exact for AT MOST THREE newlines in the
// 32 bytes (a fourth would start a line of type t again, which four spans cannot hold); the return value tells the
// caller, who must then not use the masks.  Reads of 25 bases or more never get there: four newlines in 32 bytes need
// "\n+\n" + quality + "\n" + header + "\n" inside them.
//
// No HIP header is needed: a CPU program includes this file and runs the very text the kernel compiles
// (tests/test_type_spans.py).  On the device the two-level selection is four v_bitop3_b32 on registers - what the
// compiler makes of (a & x) | (~a & y) by itself is v_bfi_b32, a 4-cycle form on gfx950 (profiles/ANALYSIS_r04.md).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQG_SPANS_HD __host__ __device__ inline
#else
#define FQG_SPANS_HD inline
#endif

namespace fqg {

// a ? x : y, bit by bit
FQG_SPANS_HD uint32_t bit_select32(uint32_t a, uint32_t x, uint32_t y) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, x, y, 0xCA);  // truth table of (A & B) | (~A & C) with A = 0xF0, B = 0xCC, C = 0xAA
#else
  return (a & x) | (~a & y);
#endif
}

// masks of the bytes on sequence (M1) and quality (M3) lines among the 32 whose newline mask is x; t = type of the
// first byte (only its bits 0..1 count).  Returns x without its three lowest bits: != 0 exactly when x has four or more
// bits set, and the masks mean nothing then.
FQG_SPANS_HD uint32_t type_spans32(uint32_t x, uint32_t t, uint32_t& M1, uint32_t& M3) {
  const uint32_t x1 = x & (x - 1u), x2 = x1 & (x1 - 1u), x3 = x2 & (x2 - 1u);
  const uint32_t b0 = x ^ x1, b1 = x1 ^ x2, b2 = x2 ^ x3;  // the three lowest newlines, one bit each
  // m = the bits below a newline (all of them where it is absent); a span is what lies below its own newline and above
  // the one in front.  (As sums the spans are b0 - 1, b1 - 2 b0, b2 - 2 b1, 0 - 2 b2 - but the compiler turns b + b into
  // v_lshlrev_b32, a 4-cycle form on gfx950, and each of these is one three-input boolean instruction.)
  const uint32_t m0 = b0 - 1u, m1 = b1 - 1u, m2 = b2 - 1u;
  const uint32_t d0 = m0;
  const uint32_t d1 = m1 & ~(m0 | b0);
  const uint32_t d2 = m2 & ~(m1 | b1);
  const uint32_t d3 = ~(m2 | b2);
  const uint32_t a0 = 0u - (t & 1u), a1 = 0u - ((t >> 1) & 1u);  // the bits of t in every position
  // (1 - t) & 3 = 1 0 3 2 and (3 - t) & 3 = 3 2 1 0 for t = 0 1 2 3: bit 0 of both is ~t0; bit 1 is t1 and ~t1
  const uint32_t e = bit_select32(a0, d0, d1), f = bit_select32(a0, d2, d3);
  M1 = bit_select32(a1, f, e);
  M3 = bit_select32(a1, e, f);
  return x3;
}

}  // namespace fqg
