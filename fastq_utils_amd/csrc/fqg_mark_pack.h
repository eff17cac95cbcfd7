// fqg_mark_pack.h - eight words of 0x80-per-byte marks -> one 32-bit mask (bit i = byte i of the 32).
//
// The streaming pass (fqg_stream_kernels.hip) turns the byte marks of a lane's 32 bytes into bit masks six times per
// chunk (newline, not-ACGTN and in-range marks of two slices).  v_dot4_u32_u8 with the weights 1 2 4 8 / 16 32 64 128
// gathers the marks of two words (8 bytes) as 8 bits at bit 7..14 of a "pair" P.  Joining two 16-bit halves, each
// (lo >> 7) | (hi << 1), cost six instructions for the four pairs (two shifts right, three shifts left, one mask and a
// three-input OR after the compiler's folding); here the pairs are joined where they stand -
//     A = (P1 << 8) | P0        marks of bytes 0..15 at bit 7..22
//     B = (P3 << 8) | P2        marks of bytes 16..31 at bit 7..22
//     out = (B << 9) | (A >> 7)
// - three v_lshl_or_b32 and one v_lshrrev_b32.  Bit 23 and up of A and B are zero (a pair is below 1 << 15), so the
// left shift by 9 drops nothing but zeros.
//
// No HIP header is needed: a CPU program includes this file and runs the very expressions the kernel compiles
// (tests/test_mark_pack.py), with the dot product restated for the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQG_PACK_HD __host__ __device__ inline
#else
#define FQG_PACK_HD inline
#endif

namespace fqg {

// sum of the four byte products of a and b, plus c
FQG_PACK_HD uint32_t udot4_u8(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else
  for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
  return c;
#endif
}

// The value as it is, but opaque to the compiler: left to itself it distributes the last shift of pack_marks32 over the
// join in front of it - shifts of the single pairs and a three-input OR, six instructions again.  The statement is
// empty (no instruction, no register moved): what the compiler sees on both sides of it stays ordinary code, so the wait
// states a v_dot4 result needs on gfx950 before another vector instruction reads it remain the compiler's business.
FQG_PACK_HD uint32_t as_computed(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(x));
#endif
  return x;
}

// the marks of two words (8 bytes) as 8 bits at bit 7..14
FQG_PACK_HD uint32_t mark_pair(uint32_t m0, uint32_t m1) {
  return udot4_u8(m1, 0x80402010u, udot4_u8(m0, 0x08040201u, 0u));
}

// eight words of 0x80-per-byte marks -> 32-bit mask (bit i = byte i of the 32)
FQG_PACK_HD uint32_t pack_marks32(uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3, uint32_t m4, uint32_t m5, uint32_t m6,
                                  uint32_t m7) {
  const uint32_t a = as_computed((mark_pair(m2, m3) << 8) | mark_pair(m0, m1));
  const uint32_t b = as_computed((mark_pair(m6, m7) << 8) | mark_pair(m4, m5));
  return (b << 9) | (a >> 7);
}

}  // namespace fqg
