// fqg_bam_index_core.h - the record walk over an inflated BAM stream, as fqg_bam_index_records does it, cut into the
// pieces the device needs to do it in parallel.  The kernels (fqg_bam_index_kernels.hip) and their CPU model
// (tests/cxx/bam_index_model.cpp) both get every decision from this text; no standard library.
//
// The rule (fqg_umi_abi.inc, the loop of fqg_bam_index_records).  At position p of a stream of nbytes:
//   stop if p + 4 > nbytes;  block = the int32 at p;  stop if block < 32 or p + 4 + block > nbytes;
//   otherwise p is a record and the walk goes on at p + 4 + block.
// A step is at least 36 bytes long, so where the walk that STARTS at q goes depends on positions >= q + 36 alone:
// treated as a possible start, every position of the stream can be resolved, thirty-six at a time, from the end of a
// SEGMENT of the stream backwards.  What is kept per position is a table entry and a count:
//   entry  kind (2 bits) | value (30 bits): where the walk from q gets to without leaving what the workgroup can see
//     kBxExit  it leaves the segment: value = landing position - segment end
//     kBxStop  it stops inside the segment, the rule says so at value = position - segment start
//     kBxHop   it reaches the record at value = position - segment start, whose step is bx_reach(ring) bytes or longer:
//              the tables of the positions behind it are no longer at hand (they live in a ring of `ring` positions),
//              or the landing does not fit an entry (block goes up to 2^31 - 1).  Whoever follows the chain reads
//              that record's block_size from the stream itself and looks the landing up: exact, one step slower.
//   count  the records the walk passes on the way (the record of a hop is NOT counted: it is the follower's step).
// The chain of the real records is then followed from the first record with one look-up per segment it enters
// (bx_follow), which gives every entered stretch its start, the number of its first record and its length; the stretches
// are walked independently to write the offsets.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQG_BX_HD __host__ __device__ inline
#else
#define FQG_BX_HD inline
#endif

namespace fqg {
namespace bx {

constexpr uint32_t kBxMinStep = 36;  // block_size field + the 32 fixed bytes of an alignment
constexpr uint32_t kBxExit = 0, kBxStop = 1, kBxHop = 2;
constexpr uint32_t kBxValueBits = 30, kBxValueMask = (1u << kBxValueBits) - 1u;
constexpr uint64_t kBxMaxSeg = 1ull << 20;  // a count is 16 bits: (1 << 20) / 36 records at most
constexpr uint32_t kBxMinRing = 128, kBxMaxRing = 1u << 14;  // (100 KiB of LDS: above it nothing is gained)

// steps of this many bytes or more are hops: what a step shorter than this lands on is still in the ring, and was not
// overwritten by the (at most 36) positions resolved together with the one that looks
FQG_BX_HD uint32_t bx_reach(uint32_t ring) { return ring - 64u; }

FQG_BX_HD uint32_t bx_entry(uint32_t kind, uint32_t value) { return (kind << kBxValueBits) | (value & kBxValueMask); }
FQG_BX_HD uint32_t bx_kind(uint32_t entry) { return entry >> kBxValueBits; }
FQG_BX_HD uint32_t bx_value(uint32_t entry) { return entry & kBxValueMask; }

FQG_BX_HD int32_t bx_rd32(const uint8_t* b) {
  return (int32_t)((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24));
}

// The rule.  `field`: the four bytes at p; they are looked at only when p + 4 <= nbytes.  True: p is a record, *next is
// where the walk goes on (36 <= *next - p, *next <= nbytes).
FQG_BX_HD bool bx_step(uint64_t p, uint64_t nbytes, const uint8_t* field, uint64_t* next) {
  if (p + 4 > nbytes) return false;
  const int32_t block = bx_rd32(field);
  if (block < 32 || p + 4 + (uint64_t)block > nbytes) return false;
  *next = p + 4 + (uint64_t)block;
  return true;
}

// One position of the backward recurrence.  q lies in the segment [seg_lo, seg_hi), seg_hi - seg_lo <= kBxMaxSeg;
// `field` as above.  ring_entry / ring_count hold, at index (position & (ring - 1)), what was resolved for the positions
// (q, q + ring) of this segment (ring: a power of two); only positions in [q + 36, q + bx_reach(ring)) are read.
FQG_BX_HD void bx_resolve(uint64_t q, uint64_t seg_lo, uint64_t seg_hi, uint64_t nbytes, const uint8_t* field, const uint32_t* ring_entry,
                          const uint16_t* ring_count, uint32_t ring, uint32_t* entry, uint16_t* count) {
  uint64_t next;
  if (!bx_step(q, nbytes, field, &next)) {
    *entry = bx_entry(kBxStop, (uint32_t)(q - seg_lo));
    *count = 0;
  } else if (next - q >= bx_reach(ring)) {
    *entry = bx_entry(kBxHop, (uint32_t)(q - seg_lo));
    *count = 0;
  } else if (next >= seg_hi) {
    *entry = bx_entry(kBxExit, (uint32_t)(next - seg_hi));
    *count = 1;
  } else {
    const uint32_t slot = (uint32_t)next & (ring - 1u);
    *entry = ring_entry[slot];
    *count = (uint16_t)(ring_count[slot] + 1u);
  }
}

// What the follower carries from segment to segment and from window to window.
struct BxState {
  uint64_t p;       // where the chain stands: the next record, or where it stopped
  uint64_t k;       // records in front of p
  uint32_t done;    // the rule said stop at p
  uint32_t n_stretch;  // stretches of the window that was followed last
  uint32_t overflow;   // a window had more stretches than bx_max_stretches says it can have: the index is not to be used
  uint32_t reserved;
};
// A stretch of the chain: n records, the first at `start` and the k-th of the stream, each the step behind the one before.
struct BxStretch {
  uint64_t start, base;
  uint32_t n, reserved;
};

// The chain through one window [w_lo, w_hi) of segments of seg bytes (the first at w_lo; the last may be shorter), whose
// tables lie at index position - w_lo.  Every stretch goes to out[0 .. s->n_stretch); cap is never reached (a window has at most
// bx_max_stretches of them; if it were, s->overflow says so).  `stream`: byte 0 of the stream, read only for the record of a hop.
FQG_BX_HD uint64_t bx_max_stretches(uint64_t window, uint64_t seg, uint32_t ring) {
  return (window + seg - 1) / seg + window / bx_reach(ring) + 2;
}
FQG_BX_HD void bx_follow(BxState* s, const uint8_t* stream, uint64_t nbytes, uint64_t w_lo, uint64_t w_hi, uint64_t seg,
                         const uint32_t* entries, const uint16_t* counts, BxStretch* out, uint64_t cap) {
  uint64_t p = s->p, k = s->k, n_out = 0;
  bool done = s->done != 0;
  while (!done && p >= w_lo && p < w_hi && n_out < cap) {
    const uint64_t seg_lo = w_lo + (p - w_lo) / seg * seg, seg_hi = seg_lo + seg < w_hi ? seg_lo + seg : w_hi;
    const uint32_t e = entries[p - w_lo], n = counts[p - w_lo], kind = bx_kind(e);
    BxStretch st;
    st.start = p;
    st.base = k;
    st.n = n;
    st.reserved = 0;
    if (kind == kBxExit) {
      p = seg_hi + bx_value(e);
    } else if (kind == kBxStop) {
      p = seg_lo + bx_value(e);
      done = true;
    } else {
      const uint64_t r = seg_lo + bx_value(e);
      uint64_t next;
      if (bx_step(r, nbytes, stream + r, &next)) {  // (it is a record: bx_resolve said so)
        st.n = n + 1u;
        p = next;
      } else {
        p = r;
        done = true;
      }
    }
    k += st.n;
    if (st.n) out[n_out++] = st;
  }
  if (!done && p >= w_lo && p < w_hi) s->overflow = 1u;  // (the loop ended on cap, not on the window's end)
  s->p = p;
  s->k = k;
  s->done = done ? 1u : 0u;
  s->n_stretch = (uint32_t)n_out;
}

// A stretch written out: offsets[base + i] for its n records; nothing at or behind offsets[cap].
FQG_BX_HD void bx_write_stretch(const BxStretch& st, const uint8_t* stream, uint64_t nbytes, uint64_t* offsets, uint64_t cap) {
  uint64_t p = st.start;
  for (uint32_t i = 0; i < st.n && st.base + i < cap; ++i) {
    uint64_t next;
    if (!bx_step(p, nbytes, stream + p, &next)) return;  // (cannot be: the tables counted these records)
    offsets[st.base + i] = p;
    p = next;
  }
}

}  // namespace bx
}  // namespace fqg
