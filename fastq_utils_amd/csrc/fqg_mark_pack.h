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
// pack_marks32_wave is the same mask from the matrix pipe: where all 64 lanes of a wavefront pack at once (uniform control
// flow), two v_mfma_i32_16x16x64_i8 stand for the eight v_dot4 and deliver the four pairs; the joins stay.  See below.
//
// No HIP header is needed: a CPU program includes this file and runs the very expressions the kernel compiles
// (tests/test_mark_pack.py, tests/test_mark_pack_wave.py), with the dot product and the MFMA restated for the host.
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

// ---- the pack of a whole wavefront on the matrix pipe ------------------------------------------------------------------
// v_mfma_i32_16x16x64_i8: D (16 x 16, i32) = A (16 x 64, i8) * B (64 x 16, i8) + C.  Every lane supplies 16 bytes of A and
// 16 bytes of B and receives four results:
//   lane l holds row i = l % 16 of A and column j = l % 16 of B, both for the K-block g = l / 16 (A and B share the
//   mapping of a lane's 16 bytes to k, so a lane's bytes meet the bytes of the same index)
//   lane j + 16 (i / 4) receives D[i][j] in register i % 4
// so   D[4 G + r][j] = sum over g, e of A(lane 4 G + r + 16 g)[e] * B(lane j + 16 g)[e]       (e = 0..15).
// With A zero in every lane but those with (l % 16) / 4 == l / 16 (lanes 0..3, 20..23, 40..43, 60..63) only g == G is
// left: lane L = j + 16 G receives in register r the dot product of ITS OWN 16 bytes of B with the 16 bytes of A in lane
// 4 G + r + 16 G = 20 G + r.  This is no matrix product in any useful sense - A is a block-diagonal of two weight rows -
// it is 64 x 2 dot products of 16 bytes in one instruction.
//   r = 0: weights on bytes 0..7     r = 1: weights on bytes 8..15     r = 2, 3: zero (their results are not used)
// The marks go in as they are: 0x80 is -128 as i8, and with the weights -1 -2 -4 .. -64 -128 (0xFF 0xFE 0xFC .. 0xC0 0x80) a
// product is +128 << e: the marks of 8 bytes at bit 7..14, exactly mark_pair().  Two MFMAs per pack (words 0..3, then
// 4..7, as B) give P0 P1 and P2 P3; the joins of pack_marks32 follow unchanged.
constexpr uint32_t kPackW0 = 0xF8FCFEFFu, kPackW1 = 0x80C0E0F0u;  // -1 -2 -4 -8 / -16 -32 -64 -128
struct PackWeights {
  uint32_t w[64][4];  // the 16 bytes of A of every lane
};
constexpr PackWeights make_pack_weights() {
  PackWeights t{};
  for (int l = 0; l < 64; ++l) {
    const bool mine = (l % 16) / 4 == l / 16;
    const int r = l % 4;
    t.w[l][0] = mine && r == 0 ? kPackW0 : 0u;
    t.w[l][1] = mine && r == 0 ? kPackW1 : 0u;
    t.w[l][2] = mine && r == 1 ? kPackW0 : 0u;
    t.w[l][3] = mine && r == 1 ? kPackW1 : 0u;
  }
  return t;
}

#if defined(__HIPCC__)
typedef int pack_v4i __attribute__((ext_vector_type(4)));
// 1 KiB that every wavefront reads once per chunk, 16 bytes per lane (one v_lshlrev_b32 for the offset and one
// global_load_dwordx4 off a scalar base; the table stays in the caches)
__device__ const PackWeights kPackWeights = make_pack_weights();
__device__ __forceinline__ pack_v4i pack_weights(int lane) {
  return *reinterpret_cast<const pack_v4i*>(kPackWeights.w[lane]);
}
// ALL 64 LANES MUST BE ACTIVE, in wave-uniform control flow: a lane that is switched off supplies no marks and no
// weights.  The MFMA stands as the builtin, never as text: the compiler must see it to place the wait states between it
// and the joins that read its results.
__device__ __forceinline__ uint32_t pack_marks32_wave(pack_v4i wts, uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3, uint32_t m4,
                                                      uint32_t m5, uint32_t m6, uint32_t m7) {
  const pack_v4i zero = {0, 0, 0, 0};
  const pack_v4i lo = __builtin_amdgcn_mfma_i32_16x16x64_i8(wts, pack_v4i{(int)m0, (int)m1, (int)m2, (int)m3}, zero, 0, 0, 0);
  const pack_v4i hi = __builtin_amdgcn_mfma_i32_16x16x64_i8(wts, pack_v4i{(int)m4, (int)m5, (int)m6, (int)m7}, zero, 0, 0, 0);
  const uint32_t a = as_computed(((uint32_t)lo.y << 8) | (uint32_t)lo.x);
  const uint32_t b = as_computed(((uint32_t)hi.y << 8) | (uint32_t)hi.x);
  return (b << 9) | (a >> 7);
}
#endif
// the instruction restated for the host, with the lane layout above: a[l], b[l] are the 16 bytes lane l supplies, d[l] the
// four results it receives; c = 0
inline void mfma_i32_16x16x64_i8_host(const uint32_t (*a)[4], const uint32_t (*b)[4], int32_t (*d)[4]) {
  int8_t ab[64][16], bb[64][16];
  for (int l = 0; l < 64; ++l)
    for (int e = 0; e < 16; ++e) {
      ab[l][e] = (int8_t)(uint8_t)(a[l][e >> 2] >> (8 * (e & 3)));
      bb[l][e] = (int8_t)(uint8_t)(b[l][e >> 2] >> (8 * (e & 3)));
    }
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 16; ++j) {
      int32_t sum = 0;
      for (int g = 0; g < 4; ++g) {
        const uint32_t* al = a[i + 16 * g];
        if (!(al[0] | al[1] | al[2] | al[3])) continue;  // (sixteen zeros add nothing: most lanes of the pack's A)
        for (int e = 0; e < 16; ++e) sum += (int32_t)ab[i + 16 * g][e] * (int32_t)bb[j + 16 * g][e];
      }
      d[j + 16 * (i / 4)][i % 4] = sum;
    }
}
// the pack of a wavefront: m[l] are the eight mark words of lane l, out[l] its mask
inline void pack_marks32_wave(const uint32_t (*m)[8], uint32_t* out) {
  constexpr PackWeights wts = make_pack_weights();
  uint32_t b_lo[64][4], b_hi[64][4];
  int32_t lo[64][4], hi[64][4];
  for (int l = 0; l < 64; ++l)
    for (int w = 0; w < 4; ++w) {
      b_lo[l][w] = m[l][w];
      b_hi[l][w] = m[l][4 + w];
    }
  mfma_i32_16x16x64_i8_host(wts.w, b_lo, lo);
  mfma_i32_16x16x64_i8_host(wts.w, b_hi, hi);
  for (int l = 0; l < 64; ++l) {
    const uint32_t a = ((uint32_t)lo[l][1] << 8) | (uint32_t)lo[l][0];
    const uint32_t b = ((uint32_t)hi[l][1] << 8) | (uint32_t)hi[l][0];
    out[l] = (b << 9) | (a >> 7);
  }
}

}  // namespace fqg
