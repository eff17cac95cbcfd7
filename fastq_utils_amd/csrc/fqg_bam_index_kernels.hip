// fqg_bam_index_kernels.hip - the offsets of the alignment records of an inflated BAM stream that lies on the device
// (fqg_bam_index_device, include/fqg.h).  Every decision is fqg_bam_index_core.h's; read that first.
//
// The walk over the records is a chain of dependent 4-byte reads.  It is cut into three launches per window of the stream:
//   k_bamidx_tables   one workgroup (ONE wavefront) per segment.  The segment is resolved from its end backwards, a chunk
//                     of kBxChunk bytes at a time: the chunk (and the three bytes behind it, a block_size field may
//                     straddle its end) is staged with 16-byte loads to the LDS address that has the source's alignment,
//                     as k_deflate_members / k_inflate_blocks stage, then lanes 0..35 take thirty-six positions per round
//                     (bx_resolve: positions q .. q+35 depend on positions >= q+36 alone).  The entries and counts of the
//                     last `ring` positions stay in LDS, which is all a step shorter than bx_reach(ring) looks at - so the
//                     segment can be much larger than LDS, and the serial part below has few segments to enter; every
//                     entry and count also goes to the window's tables in global memory.
//   k_bamidx_follow   the only serial part: lane 0 of one wavefront follows the chain of the real records through the
//                     window (bx_follow), one table look-up per segment it enters (two dependent loads more for a hop),
//                     and lists the stretches.  Its state - position, record count - is carried in device memory from
//                     window to window; the host does not look at it before the last window.
//   k_bamidx_offsets  one thread per stretch walks its records in the stream and writes offsets[base + i].
// No atomics, no flags, nothing waits for another workgroup inside a launch: the launches are ordered by the stream.
//
// One wavefront per workgroup in k_bamidx_tables: a round is thirty-six independent positions, and the rounds of a segment
// are serial; more wavefronts would only wait at the barrier of every round.  LDS per workgroup: kBxStageLds + 6 * ring
// bytes (52 KiB at the default ring of 8192: three workgroups per CU); no scratch memory.
#pragma once
#include "fqg_bam_index_core.h"
#include "fqg_device.h"

namespace fqg {

constexpr uint32_t kBxBlock = kWave;
constexpr uint32_t kBxChunk = 4096;
constexpr uint32_t kBxStageLds = kBxChunk + 48;  // up to 15 bytes in front, 3 behind, and the word that holds the last of them
static_assert(kBxStageLds % 16 == 0 && kBxStageLds >= 15 + kBxChunk + 3 + 15, "the staged words of a chunk");

struct BxArgs {
  const uint8_t* stream;  // byte 0 of the stream; 16-byte words that hold a byte of it are loaded whole
  uint64_t nbytes;
  uint64_t w_lo, w_hi;    // the window; the tables are indexed by position - w_lo
  uint64_t seg;
  uint32_t ring, reserved;
  uint32_t* entries;
  uint16_t* counts;
  bx::BxStretch* stretch;
  uint64_t stretch_cap;
  bx::BxState* state;
  unsigned long long* offsets;
  uint64_t offsets_cap;
};

__host__ __device__ inline uint32_t bx_lds_bytes(uint32_t ring) { return kBxStageLds + ring * 6u; }

__global__ __launch_bounds__(kBxBlock) void k_bamidx_tables(BxArgs A) {
  extern __shared__ uint4 bx_lds[];
  uint8_t* const stage8 = reinterpret_cast<uint8_t*>(bx_lds);
  uint32_t* const ring_entry = reinterpret_cast<uint32_t*>(stage8 + kBxStageLds);
  uint16_t* const ring_count = reinterpret_cast<uint16_t*>(ring_entry + A.ring);
  const uint32_t lane = threadIdx.x, mask = A.ring - 1u;
  const uint64_t seg_lo = A.w_lo + (uint64_t)blockIdx.x * A.seg;
  if (seg_lo >= A.w_hi) return;
  const uint64_t seg_hi = seg_lo + A.seg < A.w_hi ? seg_lo + A.seg : A.w_hi;
  for (uint64_t c_hi = seg_hi; c_hi > seg_lo;) {
    const uint64_t c_lo = c_hi - seg_lo > kBxChunk ? c_hi - kBxChunk : seg_lo;
    const uint64_t c_end = c_hi + 3 < A.nbytes ? c_hi + 3 : A.nbytes;  // (c_hi <= nbytes: only bytes of the stream)
    const uintptr_t a = (uintptr_t)A.stream + (uintptr_t)c_lo, a0 = a & ~(uintptr_t)15;
    const uintptr_t a1 = ((uintptr_t)A.stream + (uintptr_t)c_end + 15) & ~(uintptr_t)15;
    const uint32_t words = (uint32_t)((a1 - a0) >> 4);  // <= kBxStageLds / 16
    const uint4* src = reinterpret_cast<const uint4*>(a0);
    __syncthreads();  // (the chunk before is read no more)
    for (uint32_t k = lane; k < words && k < kBxStageLds / 16; k += kBxBlock) bx_lds[k] = src[k];
    __syncthreads();
    const uint8_t* const bytes = stage8 + (uint32_t)(a - a0);  // byte c_lo
    for (uint64_t top = c_hi; top > c_lo;) {
      const uint64_t g_lo = top - c_lo > bx::kBxMinStep ? top - bx::kBxMinStep : c_lo;
      const bool mine = lane < (uint32_t)(top - g_lo);
      const uint64_t q = top - 1 - lane;
      uint32_t e = 0;
      uint16_t n = 0;
      if (mine) bx::bx_resolve(q, seg_lo, seg_hi, A.nbytes, bytes + (uint32_t)(q - c_lo), ring_entry, ring_count, A.ring, &e, &n);
      if (mine) {
        ring_entry[(uint32_t)q & mask] = e;
        ring_count[(uint32_t)q & mask] = n;
        A.entries[q - A.w_lo] = e;
        A.counts[q - A.w_lo] = n;
      }
      __syncthreads();  // (the next round reads what this one wrote)
      top = g_lo;
    }
    c_hi = c_lo;
  }
}

__global__ __launch_bounds__(kBxBlock) void k_bamidx_follow(BxArgs A) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  bx::BxState s = *A.state;
  bx::bx_follow(&s, A.stream, A.nbytes, A.w_lo, A.w_hi, A.seg, A.entries, A.counts, A.stretch, A.stretch_cap);
  *A.state = s;
}

__global__ __launch_bounds__(kBxBlock) void k_bamidx_offsets(BxArgs A) {
  const uint64_t t = (uint64_t)blockIdx.x * kBxBlock + threadIdx.x;
  if (t >= A.state->n_stretch || t >= A.stretch_cap) return;
  bx::bx_write_stretch(A.stretch[t], A.stream, A.nbytes, reinterpret_cast<uint64_t*>(A.offsets), A.offsets_cap);
}

}  // namespace fqg
