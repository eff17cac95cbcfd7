// fqg_bam_tile.h - the tile frame of the kernels that walk an inflated BAM stream (k_bt_tile, k_b2f_tile): one
// wavefront per tile of T consecutive alignments, one lane per alignment.  The tile's bytes are ONE span of the stream;
// a span that fits is copied to LDS with 16-byte loads, what the tile writes is built in LDS images of its output spans
// and goes out with 16-byte stores (emit_flush).  Whether a tile fits, and the records, are the kernel's business.
#pragma once
#include "fqg_tile.h"

namespace fqg {

// what the argument structs of both kernels start with
struct BamTiles {
  const uint8_t* buf;        // the stream, at a 16-byte boundary
  uint64_t nbytes;
  const unsigned long long* offs;  // of every alignment, ascending, each + 36 inside the stream (the C-ABI checks)
  uint32_t n, T;             // alignments; per tile
  uint32_t in_cap, out_cap;  // LDS bytes of the two areas (dynamic shared memory: in_cap + out_cap + 64)
};

// A lane's view of its tile.  valid: the lane has an alignment of its own (the others look at the tile's last one).
// in_off: where alignment i starts; in0, last_off: the tile's first and last; in_skew = in0 & 15 (the stream starts at a
// 16-byte boundary).  in_end: the end of the tile's span - of its last record as its block_size tells it when that
// lies inside the stream (`inside`), of the stream otherwise.
struct BamTileView {
  uint32_t i0, Tn, i, in_skew;
  uint64_t in_off, in0, last_off, in_end;
  bool valid, inside;
};

// 4 bytes at any alignment, little-endian
__device__ __forceinline__ uint32_t bam_ld32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// false: this workgroup has no tile
__device__ __forceinline__ bool bam_tile_view(const BamTiles& A, int lane, BamTileView& v) {
  v.i0 = blockIdx.x * A.T;
  if (v.i0 >= A.n) return false;
  v.Tn = A.n - v.i0 < A.T ? A.n - v.i0 : A.T;
  v.valid = (uint32_t)lane < v.Tn;
  v.i = v.i0 + (v.valid ? (uint32_t)lane : v.Tn - 1);
  v.in_off = A.offs[v.i];
  v.in0 = rfl64(v.in_off);
  v.in_skew = (uint32_t)(v.in0 & 15u);
  // the span runs to the end of the tile's last record, which only the record itself tells
  v.last_off = rl64(v.in_off, (int)v.Tn - 1);
  const uint32_t last_block = v.last_off + 4 <= A.nbytes ? bam_ld32(A.buf + v.last_off) : 0u;
  const uint64_t end = v.last_off + 4ull + last_block;
  v.inside = end <= A.nbytes;
  v.in_end = v.inside ? end : A.nbytes;
  return true;
}

// The span [in0, in_end) to LDS: s_in[k] = stream byte base + k, base (returned) = in0 - in_skew.  The caller has found
// in_skew + (in_end - in0) + 16 <= in_cap.  Ends with the wavefront's fence and barrier: every lane may read all of it.
__device__ __forceinline__ uint64_t bam_tile_stage(const BamTiles& A, const BamTileView& v, int lane, uint8_t* s_in) {
  const uint32_t span = v.in_skew + (uint32_t)(v.in_end - v.in0);
  const uint64_t base = v.in0 - v.in_skew;
  const uint32_t units = (span + 15u) >> 4;
  // whole 16-byte units that lie inside the stream: 8 loads in flight per lane; the last unit(s) of the stream byte by byte
  const uint64_t safe_units = A.nbytes > base ? (A.nbytes - base) >> 4 : 0;
  for (uint32_t u0 = 0; u0 < units; u0 += 8 * kWave) {
    bc_u32x4 q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint32_t u = u0 + j * kWave + (uint32_t)lane;
      u = u < units ? u : units - 1;
      if ((uint64_t)u < safe_units) q[j] = __builtin_nontemporal_load(reinterpret_cast<const bc_u32x4*>(A.buf + base + 16ull * u));
      else {
        uint32_t t[4] = {0, 0, 0, 0};  // (unrolled: the words stay in registers)
#pragma unroll
        for (int b = 0; b < 16; ++b)
          if (base + 16ull * u + (uint64_t)b < A.nbytes) t[b >> 2] |= (uint32_t)A.buf[base + 16ull * u + (uint64_t)b] << (8 * (b & 3));
        q[j] = bc_u32x4{t[0], t[1], t[2], t[3]};
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t u = u0 + j * kWave + (uint32_t)lane;
      if (u < units) *reinterpret_cast<bc_u32x4*>(s_in + 16u * u) = q[j];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return base;
}

// Where the tile's image of one output lies: the lane's record goes to out + out_off and has `size` bytes, so the
// tile writes [first, first + len); skew = what the image's first byte is behind a 16-byte boundary in memory (its
// place in the LDS image: emit_flush).
struct BamImage {
  uint64_t first, len;
  uint32_t skew;
};
__device__ __forceinline__ BamImage bam_tile_image(const uint8_t* out, uint64_t out_off, uint32_t size, uint32_t Tn) {
  const uint64_t first = rfl64(out_off);
  return {first, rl64(out_off + size, (int)Tn - 1) - first, (uint32_t)((uintptr_t)(out + first) & 15u)};
}

}  // namespace fqg
