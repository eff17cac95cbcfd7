// fqg_stream_kernels.hip - single-pass ("streaming") framing + byte-class checks for gfx950.
//
// The two-pass path of fqg_kernels.hip reads the image twice: a newline census gives every 4 KiB
// chunk its global line rank, then k_frame_fast_t uses the rank for the line index and for the
// line type (index mod 4) that the byte-class checks depend on.  Here the image is read ONCE:
//
//   k_stream_boot   quality range of the first records (line types are known at the image start)
//   k_stream_pass1  one wavefront per 4 KiB chunk, no dependence on any other chunk:
//                     - newline mask, NUL / CR / high-byte detection (SWAR on bytes < 0x80, byte
//                       marks compacted to bit masks with v_dot4_u32_u8 - in the launches that also carry line
//                       workers with v_mfma_i32_16x16x64_i8: fqg_mark_pack.h)
//                     - the line type of the chunk's first byte is SPECULATED from the first
//                       one-character line of the chunk (in FASTQ that is the "+" line, type 2)
//                     - with that type: bases outside ACGTN on sequence lines -> suspect byte
//                       positions are queued; quality bytes are only tested against the boot
//                       range, and a chunk with bytes outside it computes its exact min / max
//                     - every '\n' is staged as a 16-bit entry (offset in chunk, class of the byte
//                       after it, "the byte after that is '\n'") through a per-wave LDS table, so
//                       that the global stores are contiguous
//   k_scan_a/b      prefix over the per-chunk newline counts (fqg_kernels.hip)
//   k_stream_chunks one lane per chunk, now with the true rank: verification of the speculation (a
//                   wrong or missing one sends the chunk to the redo list, where k_frame_fast_t
//                   repeats the checks with the true type), quality range merge
//   k_stream_lines  one lane per record: staged entries -> line_end[], header-start checks ('@', not
//                   empty; "+\n") by line type, lengths, statistics (k_stream_lines_fast: the
//                   steps of ordinary records, without a search)
//   k_stream_queue  queued suspect positions -> record bits (binary search in line_end[])
//
// Nothing here decides an error code: as in the two-pass path, records the checks cannot vouch for
// are marked in the suspect bitmap and k_validate_exact alone decides.  Over-marking is harmless;
// what must be exact are the line index, the quality range (hull of the boot range, of verified
// per-chunk ranges and of redone chunks) and the image flags that force the two-pass / exact path.
#include "fqg_device.h"
#include "fqg_type_spans.h"
#include "fqg_mark_pack.h"
#include "fqg_part_steps.h"
#include "fqg_line_window.h"

namespace fqg {

constexpr uint32_t kH = 0x80808080u;

// four words of 0x80-per-byte marks -> 16-bit mask (bit i = byte i of the 16)
__device__ __forceinline__ uint32_t pack_marks16(uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3) {
  uint32_t lo = __builtin_amdgcn_udot4(m0, 0x08040201u, 0u, false);
  lo = __builtin_amdgcn_udot4(m1, 0x80402010u, lo, false);
  uint32_t hi = __builtin_amdgcn_udot4(m2, 0x08040201u, 0u, false);
  hi = __builtin_amdgcn_udot4(m3, 0x80402010u, hi, false);
  return (lo >> 7) | (hi << 1);
}

// Newline marks of a word whose bytes are all < 0x80, with the control-character test as ONE three-input boolean
// instruction per word: `bad` collects bit 7 of every byte that is < 0x20 and no '\n'.  (x = byte ^ 0x0A keeps a byte on its side of 0x20; t = 0x80 - x has bit 7
// where x == 0; t + 0x1F = 0x9F - x has bit 7 where x < 0x20.  No byte carries into its neighbour: t is 0x01..0x80.)
// What an instruction costs on gfx950 decides the form (tools/kbench/valubench.hip, profiles/r04*_valubench.txt): a
// two-operand VALU instruction on registers or a literal - and v_bitop3_b32 - issues in 2 cycles per wavefront, a
// three-operand one (v_or3, v_and_or, v_perm, v_dot4, v_xad, v_lshl_or ..) or one that reads an SGPR in 4.
__device__ __forceinline__ uint32_t nl_marks7(uint32_t w, uint32_t& bad) {
  const uint32_t x = w ^ 0x0A0A0A0Au;
  const uint32_t t = kH - x;
  const uint32_t c = t + 0x1F1F1F1Fu;
  bad = __builtin_amdgcn_bitop3_b32(bad, c, t, 0xF4);  // bad | (c & ~t): truth table of A | (B & ~C) with A = 0xF0, B = 0xCC, C = 0xAA
  return t & kH;
}
__device__ __forceinline__ uint32_t or3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xFE); }

// a wave-uniform value in a VECTOR register: v_sub / v_add on two vector registers issue in 2 cycles, with an SGPR
// operand in 4 (the compiler would keep such a value in an SGPR)
__device__ __forceinline__ uint32_t in_vgpr(uint32_t x) {
  uint32_t v;
  asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
  return v;
}

// 0x80 in every byte (< 0x80) that is not one of A C G T N
__device__ __forceinline__ uint32_t not_acgtn7(uint32_t w) {
  // byte table indexed by (c & 7): 7F 'A' 7F 'C' 'T' 7F 'N' 'G'; 0x7F never matches (its low bits are 7)
  const uint32_t want = __builtin_amdgcn_perm(0x474E7F54u, 0x437F417Fu, w & 0x07070707u);
  return ((w ^ want) + 0x7F7F7F7Fu) & kH;
}

// 0x80 in every byte (< 0x80) inside [lo, hi]; lob = lo * 0x01010101, hihb = (hi | 0x80) * 0x01010101
__device__ __forceinline__ uint32_t in_range7(uint32_t w, uint32_t lob, uint32_t hihb, uint32_t kh = kH) {
  return ((w | kH) - lob) & (hihb - w) & kh;
}
// The same with the lower bound as an ADDEND: lo_add = (0x80 - lo) * 0x01010101 (lo <= 127).  A byte b < 0x80 plus
// 0x80 - lo stays below 0x100 - no byte carries into its neighbour - and has bit 7 exactly when b >= lo: one
// instruction where `(w | 0x80..) - lo..` takes two.
__device__ __forceinline__ uint32_t in_range7a(uint32_t w, uint32_t lo_add, uint32_t hihb, uint32_t kh) {
  return (w + lo_add) & (hihb - w) & kh;
}

// ------------------------------------------------------------------------------------------
// quality range of the complete records inside the first `span` bytes (span: multiple of 256,
// span <= image size).  One workgroup.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kBootMax = 64u << 10;  // span <= kBootMax (host: kStreamBootBytes)
constexpr int kBootBlock = 1024;          // 16 wavefronts, 4 KiB of the window each: the walks below are serial per
                                          // wavefront, and the whole call waits for this one workgroup (0.040 -> 0.02 ms)
__global__ __launch_bounds__(kBootBlock) void k_stream_boot(const uint8_t* __restrict__ img, uint32_t span,
                                                            CallState* __restrict__ cs) {
  constexpr int kBootWaves = kBootBlock / kWave;
  __shared__ uint32_t s_cnt[kBootWaves];
  __shared__ __attribute__((aligned(16))) uint8_t s_img[kBootMax];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  const uint32_t part = span / kBootWaves;  // (span is a multiple of 256: part is a multiple of 16)
  // the prefix goes to LDS first (all loads in flight at once): the two byte-wise walks below would
  // otherwise pay a memory round trip per 64 bytes each
  for (uint32_t o = threadIdx.x * 16u; o < span; o += kBootBlock * 16u)
    *reinterpret_cast<uint4*>(s_img + o) = *reinterpret_cast<const uint4*>(img + o);
  __syncthreads();
  const uint8_t* p = s_img + (uint64_t)wv * part;
  uint32_t cnt = 0;
  for (uint32_t o = lane; o < part; o += kWave) cnt += (p[o] == '\n');
  cnt = wave_sum(cnt);
  if (lane == 0) s_cnt[wv] = cnt;
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (int w = 0; w < kBootWaves; ++w) {
    if (w < wv) before += s_cnt[w];
    total += s_cnt[w];
  }
  const uint32_t limit = total & ~3u;
  if (threadIdx.x == 0) cs->boot_lines = total;
  uint32_t line = before, qmin = 255, qmax = 0;
  for (uint32_t o = 0; o < part; o += kWave) {
    const uint32_t c = o + lane < part ? (uint32_t)p[o + lane] : 0u;
    const uint64_t bal = __ballot(o + lane < part && c == '\n');
    const uint32_t mine = line + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
    if ((mine & 3u) == 3u && mine < limit && c != '\n' && o + lane < part) {
      qmin = c < qmin ? c : qmin;
      qmax = c > qmax ? c : qmax;
    }
    line += (uint32_t)__builtin_popcountll(bal);
  }
  wave_minmax(qmin, qmax);
  if (lane == 0 && qmin <= qmax) {
    atomicMin(&cs->boot_qmin, qmin);
    atomicMax(&cs->boot_qmax, qmax);
    atomicMin(&cs->qmin_byte, qmin);
    atomicMax(&cs->qmax_byte, qmax);
  }
}

// ------------------------------------------------------------------------------------------
// pass 1
// ------------------------------------------------------------------------------------------
struct StreamOut {
  uint32_t* counts;            // newlines per chunk
  uint32_t* cinfo;             // chunk info word
  uint16_t* stage;             // kStageCap entries per chunk
  unsigned long long* queue;   // suspect byte positions
  unsigned long long queue_cap;
};

__device__ __forceinline__ void queue_suspect(const StreamOut& o, CallState* cs, uint64_t pos) {
  if (__hip_atomic_load(&cs->queue_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > o.queue_cap) return;
  const unsigned long long at = atomicAdd(&cs->queue_count, 1ull);
  if (at < o.queue_cap) o.queue[at] = pos;
}

// Work decomposition of pass 1: ONE WAVEFRONT per 4 KiB chunk, walked as kHalves = 2 slices of
// 2 KiB; inside a slice every lane owns 32 CONTIGUOUS bytes (two 16-byte loads at a 32-byte lane
// stride - measured as fast as the fully interleaved pattern), so that all per-lane masks are
// 32 bits wide and the cross-lane work (scan, look-ahead) is paid once per 32 bytes.
constexpr int kHalves = 2;
constexpr int kLaneBytes = 32;
constexpr int kHalfBytes = kWave * kLaneBytes;  // 2 KiB

struct Piece32 {
  uint4 a, b;  // bytes 0..15, 16..31
};

// Staging of the newlines of one chunk.  Every lane writes (offset | "second next byte is a newline")
// of its newlines to the wave's LDS table at their rank; lane i then takes entry i, adds the class
// of the byte after that newline and stores the 16-bit entry (contiguous 2-byte stores).  The byte
// after a newline comes from an LDS copy of the chunk, in image order (a gather from global memory
// would miss the L2 often enough to cost 10 % more HBM reads; the copy's 16-byte stores at a 32-byte
// lane stride meet two-way bank conflicts, which the store's own issue time covers - a conflict-free
// layout of round 3 paid for itself with six address instructions per look-up).
// The name-capturing instantiation reads header lines from the copy 8 bytes at a time at any alignment: kCopyFront
// bytes of slack in front of it and kCopyBack behind - a header's 64-byte window starts 3 bytes before its '@' and may
// reach past the chunk.
constexpr uint32_t kCopyFront = 16, kCopyBack = 64;
constexpr uint32_t kCopyRow = kCopyFront + kChunkBytes + kCopyBack;

__device__ __forceinline__ uint32_t stage_entry(uint32_t ent, uint32_t c1) {
  return ent | ((c1 == '@' ? kClsAt : (c1 == '+' ? kClsPlus : 0u)) << 12);
}

template <uint32_t ABL>
__device__ __forceinline__ void stage_chunk(const uint8_t* __restrict__ img, uint64_t n, uint64_t cb, uint32_t chunk,
                                            const uint32_t (&nl)[kHalves], const uint32_t (&nl2)[kHalves],
                                            const uint32_t (&ex)[kHalves], uint32_t tot, bool fits,
                                            uint16_t* __restrict__ slots, const uint8_t* __restrict__ copy,
                                            uint32_t tail, uint16_t* __restrict__ stage, bool interior) {
  const int lane = lane_id();
#pragma unroll
  for (int k = 0; k < kHalves; ++k) {
    uint32_t m = nl[k], r = ex[k];
    const uint32_t at = (uint32_t)k * kHalfBytes + (uint32_t)lane * kLaneBytes;
    if (fits) {
      // every rank of the chunk has a slot (`fits` is uniform: total <= kStageCap): no test per newline.  The entry is the
      // bit of nl2 on top of (at | j) - v_bfe_u32, v_or_b32 and one v_lshl_or_b32; `at` holds the slice and has its low five
      // bits clear.  (as_computed: or the compiler shifts the bit by itself and joins the three with a v_or3_b32.)
      while (m) {
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        m &= m - 1;
        slots[r] = (uint16_t)((__builtin_amdgcn_ubfe(nl2[k], j, 1u) << 14) | as_computed(at | j));
        ++r;
      }
      continue;
    }
    // (a chunk with more newlines than slots: the image is abandoned to the two-pass path, kFlagStageOverflow)
    while (m) {
      const uint32_t j = (uint32_t)__builtin_ctz(m);
      m &= m - 1;
      if (r < (uint32_t)kStageCap) slots[r] = (uint16_t)((at + j) | (((nl2[k] >> j) & 1u) << 14));
      ++r;
    }
  }
  __builtin_amdgcn_wave_barrier();
  uint16_t* dst = stage + (uint64_t)chunk * kStageCap;
  for (uint32_t i = lane; i < tot; i += kWave) {
    const uint32_t ent = slots[i];
    const uint32_t o = (ent & 0xFFFu) + 1;  // the byte after the '\n'
    uint32_t c1 = 0;
    if (!(ABL & 4u)) {
      if (interior) c1 = o < (uint32_t)kChunkBytes ? (uint32_t)copy[o] : (tail & 0xFFu);
      else c1 = cb + o < n ? (uint32_t)img[cb + o] : 0u;
    }
    dst[i] = (uint16_t)stage_entry(ent, c1);
  }
}

// ABL: ablation mask for tools/kbench (product code instantiates 0): 1 = no byte-class checks,
// 2 = no staging, 4 = no fetch of the byte after a newline, 8 = no base check, 16 = no quality test
// WAVE_PACK: the six mark packs on the matrix pipe (pack_marks32_wave) instead of v_dot4 (pack_marks32)
// NAMES: also capture the header lines that begin in the chunk (NameCapture, fqg_device.h)
// NAMES: 0 = no capture, 1 = 64-byte records, 2 = 16-byte digests (fqg_device.h)
// LDS of a pass-1 workgroup: the staging slots and the copies of its four chunks (static in k_stream_pass1, a piece of the
// dynamic LDS in the kernel that also runs the line workers, k_stream_pass1_lines)
template <int NAMES>
struct Pass1Lds {
  uint16_t slots[kBlock / kWave][kStageCap];
  __attribute__((aligned(16))) uint8_t copy[kBlock / kWave][NAMES ? kCopyRow : (uint32_t)kChunkBytes];
};

// ------------------------------------------------------------------------------------------
// The steps of pass 1, in the order of the header comment: each takes what it reads and returns what it makes, and
// stream_pass1_body below is their sequence.
// ------------------------------------------------------------------------------------------
// which chunk the wavefront has, and which lane of it this is
struct ChunkLane {
  uint32_t chunk;
  uint64_t cb, wb;  // the chunk's first byte in the image; the first of the lane's 32 bytes of slice 0
  bool interior;    // the chunk and the 4 bytes behind it lie inside the image (all but the last one or two chunks)
  int lane;
  uint8_t* copy;    // the wave's LDS copy of the chunk, in image order
};

// WAVE_PACK: the six mark packs of a chunk run on the matrix pipe (pack_marks32_wave, fqg_mark_pack.h): twelve MFMAs
// where 48 v_dot4 stand.  Every one of them stands where the whole wavefront goes or does not go - a wavefront that is
// in pass 1 has all 64 lanes (it leaves by chunk), `interior` depends on the chunk alone, and whether a chunk takes the
// class tests of a typed chunk comes from ballots - so all 64 lanes supply their marks.  The weights depend on the lane
// alone: one 16-byte load per chunk.
template <bool WAVE_PACK>
struct MarkPack {
  pack_v4i wts = {0, 0, 0, 0};
  __device__ __forceinline__ explicit MarkPack(int lane) {
    if (WAVE_PACK) wts = pack_weights(lane);
  }
  __device__ __forceinline__ uint32_t operator()(uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3, uint32_t m4, uint32_t m5,
                                                 uint32_t m6, uint32_t m7) const {
    if constexpr (WAVE_PACK) return pack_marks32_wave(wts, m0, m1, m2, m3, m4, m5, m6, m7);
    else return pack_marks32(m0, m1, m2, m3, m4, m5, m6, m7);
  }
};

// ---- load and marks, interior form: a chunk that lies inside the image with the 4 bytes behind it ----
// 16-byte loads, SWAR marks, the LDS copy.  Out: nl = newline bits of the lane's 32 bytes per slice, v = the bytes,
// tail = the 4 bytes after the chunk (look-ahead of the last lane), prev (NAMES) = the byte in front of the chunk,
// flags = the image flags the chunk raises.  (The edge form - the last one or two chunks - stands in stream_pass1_body.)
template <uint32_t ABL, int NAMES, class PACK>
__device__ __forceinline__ void load_marks_interior(const uint8_t* __restrict__ img, const ChunkLane& c, const PACK& pack,
                                                    uint32_t (&nl)[kHalves], Piece32 (&v)[kHalves], uint32_t& tail, uint32_t& prev,
                                                    uint32_t& flags) {
  tail = *reinterpret_cast<const uint32_t*>(img + c.cb + kChunkBytes);
  if (NAMES && c.chunk) prev = *reinterpret_cast<const uint32_t*>(img + c.cb - 4) >> 24;
#pragma unroll
  for (int k = 0; k < kHalves; ++k) {
    v[k].a = *reinterpret_cast<const uint4*>(img + c.wb + (uint64_t)k * kHalfBytes);
    v[k].b = *reinterpret_cast<const uint4*>(img + c.wb + (uint64_t)k * kHalfBytes + 16);
  }
  if (!(ABL & 6u)) {
#pragma unroll
    for (int k = 0; k < kHalves; ++k) {
      *reinterpret_cast<uint4*>(&c.copy[k * kHalfBytes + c.lane * kLaneBytes]) = v[k].a;
      *reinterpret_cast<uint4*>(&c.copy[k * kHalfBytes + c.lane * kLaneBytes + 16]) = v[k].b;
    }
  }
  uint32_t hiacc = 0, badacc = 0;
#pragma unroll
  for (int k = 0; k < kHalves; ++k) {
    hiacc = or3(or3(or3(or3(hiacc, v[k].a.x, v[k].a.y), v[k].a.z, v[k].a.w), v[k].b.x, v[k].b.y), v[k].b.z, v[k].b.w);
    nl[k] = pack(nl_marks7(v[k].a.x, badacc), nl_marks7(v[k].a.y, badacc), nl_marks7(v[k].a.z, badacc), nl_marks7(v[k].a.w, badacc),
                   nl_marks7(v[k].b.x, badacc), nl_marks7(v[k].b.y, badacc), nl_marks7(v[k].b.z, badacc), nl_marks7(v[k].b.w, badacc));
  }
  const bool high = __ballot((hiacc & kH) != 0) != 0;
  const bool ctrl = __ballot((badacc & kH) != 0) != 0;
  if (high) flags |= kFlagHigh;  // (the masks above are meaningless then; the host drops this pass)
  if (ctrl && !high) {
    // rare: a control byte other than '\n'.  Only NUL and CR change what a line is (C strings,
    // src/fastq.c:250,317); anything else (a tab in a header ...) is just a byte.
    uint32_t nul = 0, cr = 0;
#pragma unroll
    for (int k = 0; k < kHalves; ++k) {
      const uint32_t w[8] = {v[k].a.x, v[k].a.y, v[k].a.z, v[k].a.w, v[k].b.x, v[k].b.y, v[k].b.z, v[k].b.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        nul |= eq_bytes(w[j], 0u);
        cr |= eq_bytes(w[j], 0x0D0D0D0Du);
      }
    }
    if (__ballot(nul != 0)) flags |= kFlagNul;
    if (__ballot(cr != 0)) flags |= kFlagCr;
  }
}

// ---- ranks of the newlines inside the chunk: one packed scan for both slices ----
struct NlRanks {
  uint32_t ex[kHalves];  // rank in the chunk of the first newline of the lane's 32 bytes, per slice
  uint32_t total;        // newlines of the chunk
  uint32_t staged;       // ... that have a slot in the staging area
};
// (a chunk with more newlines than slots raises kFlagStageOverflow in `flags`)
__device__ __forceinline__ NlRanks rank_newlines(const uint32_t (&nl)[kHalves], uint32_t& flags) {
  static_assert(kHalves == 2 && kHalves * kHalfBytes == kChunkBytes, "one packed scan covers the two slices");
  NlRanks r;
  const uint32_t c01 = __popc(nl[0]) | (__popc(nl[1]) << 16);
  const uint32_t s01 = wave_scan_incl_dpp(c01);
  const uint32_t t01 = __builtin_amdgcn_readlane(s01, 63);
  r.total = (t01 & 0xFFFFu) + (t01 >> 16);
  r.ex[0] = (s01 & 0xFFFFu) - (c01 & 0xFFFFu);
  r.ex[1] = (t01 & 0xFFFFu) + (s01 >> 16) - (c01 >> 16);
  if (r.total > (uint32_t)kStageCap) flags |= kFlagStageOverflow;
  r.staged = r.total < (uint32_t)kStageCap ? r.total : (uint32_t)kStageCap;
  return r;
}

// ---- look-ahead: newline bits of the bytes 1 and 2 further on (funnel shifts over {next lane, this lane}) ----
struct LookAhead {
  uint32_t nl2[kHalves];   // the byte two places on is a '\n'
  uint32_t cand[kHalves];  // a '\n' followed by exactly one byte and another '\n'
};
__device__ __forceinline__ LookAhead look_ahead(const uint8_t* __restrict__ img, uint64_t n, const ChunkLane& c,
                                                const uint32_t (&nl)[kHalves], uint32_t tail) {
  uint32_t tail_nl = 0;
  if (c.interior) {
    tail_nl = ((tail & 0xFFu) == '\n' ? 1u : 0u) | (((tail >> 8) & 0xFFu) == '\n' ? 2u : 0u);
  } else {
    for (uint64_t i = 0; i < 2; ++i)
      if (c.cb + kChunkBytes + i < n && img[c.cb + kChunkBytes + i] == '\n') tail_nl |= 1u << i;
  }
  LookAhead la;
#pragma unroll
  for (int k = 0; k < kHalves; ++k) {
    uint32_t nxt = dpp0<0x130, 0xf, 0xf>(nl[k]);  // lane i <- lane i+1
    const uint32_t first_next = (uint32_t)__builtin_amdgcn_readlane(nl[k + 1 < kHalves ? k + 1 : k], 0);
    if (c.lane == 63) nxt = k + 1 < kHalves ? first_next : tail_nl;
    const uint32_t n1 = __builtin_amdgcn_alignbit(nxt, nl[k], 1);
    la.nl2[k] = __builtin_amdgcn_alignbit(nxt, nl[k], 2);
    la.cand[k] = nl[k] & la.nl2[k] & ~n1;
  }
  return la;
}

// ---- speculation: the first line of exactly one byte is taken for a "+" line (type 2) ----
struct Speculation {
  bool found;   // a line type was speculated
  uint32_t t0;  // ... for the chunk's first byte
};
__device__ __forceinline__ Speculation speculate(const uint32_t (&nl)[kHalves], const uint32_t (&ex)[kHalves],
                                                 const uint32_t (&cand)[kHalves]) {
  Speculation sp{false, 0};
#pragma unroll
  for (int k = 0; k < kHalves; ++k) {
    const uint64_t bal = __ballot(cand[k] != 0);
    if (!sp.found && bal) {
      const int l = __builtin_ctzll(bal);
      const uint32_t cl = (uint32_t)__builtin_amdgcn_readlane(cand[k], l);
      const uint32_t nll = (uint32_t)__builtin_amdgcn_readlane(nl[k], l);
      const uint32_t exl = (uint32_t)__builtin_amdgcn_readlane(ex[k], l);
      const uint32_t j = (uint32_t)__builtin_ctz(cl);
      const uint32_t a = exl + __popc(nll & ((1u << j) - 1u));  // rank in the chunk of the '\n' in front of the "+"
      sp.t0 = (1u - a) & 3u;  // the next '\n' (rank a + 1) ends a type-2 line
      sp.found = true;
    }
  }
  return sp;
}

// ---- class tests ----
// The type masks are spans between a lane's first three newlines (fqg_type_spans.h): M1 the bytes of sequence lines, M3
// those of quality lines (the newline bytes are in neither mask).  False for a chunk with a lane of four or more newlines
// in 32 bytes - reads under 25 bases: it makes no class tests and queues nothing, it stays kInfoUnknown, and
// k_stream_chunks sends it to the redo list, where the two-pass kernel repeats the checks exactly.  (The speculation
// stands: the name capture does not use the masks.)
__device__ __forceinline__ bool chunk_type_spans(const uint32_t (&nl)[kHalves], const uint32_t (&ex)[kHalves], uint32_t t0,
                                                 uint32_t (&M1)[kHalves], uint32_t (&M3)[kHalves]) {
  uint32_t over = 0;
#pragma unroll
  for (int k = 0; k < kHalves; ++k) over |= type_spans32(nl[k], t0 + ex[k], M1[k], M3[k]);
  return __ballot(over != 0) == 0;
}

// the range the quality bytes are tested against: the boot range, or the empty range 127 .. 0 - every byte outside - when
// the boot window gave none or one beyond the 7-bit bytes of the SWAR tests
struct QBounds {
  uint32_t lo, hi;
};
__device__ __forceinline__ QBounds test_bounds(QBounds boot) {
  if (boot.lo > boot.hi || boot.lo > 127u) {
    boot.lo = 127u;
    boot.hi = 0u;
  }
  return boot;
}
// the exact range of a chunk's quality bytes, over the wavefront, as bits of the chunk info word (none: no byte selected)
__device__ __forceinline__ uint32_t range_info(const QRange& q) {
  uint32_t qmin, qmax;
  qrange_minmax(q, qmin, qmax);
  wave_minmax(qmin, qmax);
  return qmin <= qmax ? kInfoRange | ((qmin & 0xFFu) << 8) | ((qmax & 0xFFu) << 16) : 0u;
}

// A chunk with a speculated type t0 and its masks: bases outside ACGTN on sequence lines are queued as suspect byte
// positions; quality bytes are tested against the boot range, and a slice with one outside it computes its exact range.
// Returns the chunk info word.
template <uint32_t ABL, class PACK>
__device__ __forceinline__ uint32_t typed_chunk_tests(const ChunkLane& c, const Piece32 (&v)[kHalves], const uint32_t (&M1)[kHalves],
                                                      const uint32_t (&M3)[kHalves], uint32_t t0, QBounds boot, const PACK& pack,
                                                      const StreamOut& o, CallState* __restrict__ cs) {
  const QBounds t = test_bounds(boot);
  const uint32_t hihb_s = ((t.hi & 0x7Fu) | 0x80u) * 0x01010101u;
  // (in vector registers: a subtraction that reads an SGPR issues in 4 cycles instead of 2, and a three-operand
  // instruction cannot hold a literal - the compiler would keep all three in SGPRs)
  const uint32_t lo_add = in_vgpr((0x80u - t.lo) * 0x01010101u), hihb = in_vgpr(hihb_s), khv = in_vgpr(kH);
  QRange q{0x00FF00FFu, 0x00FF00FFu, 0u, 0u};
  bool any_viol = false;
#pragma unroll
  for (int k = 0; k < kHalves; ++k) {
    const uint4 &a = v[k].a, &b = v[k].b;
    const uint32_t inv = pack(not_acgtn7(a.x), not_acgtn7(a.y), not_acgtn7(a.z), not_acgtn7(a.w), not_acgtn7(b.x), not_acgtn7(b.y),
                              not_acgtn7(b.z), not_acgtn7(b.w));
    const uint32_t bad = (ABL & 8u) ? 0u : inv & M1[k];
    if (bad) queue_suspect(o, cs, c.wb + (uint64_t)k * kHalfBytes + (uint32_t)__builtin_ctz(bad));
    const uint32_t okq = pack(in_range7a(a.x, lo_add, hihb, khv), in_range7a(a.y, lo_add, hihb, khv), in_range7a(a.z, lo_add, hihb, khv),
                              in_range7a(a.w, lo_add, hihb, khv), in_range7a(b.x, lo_add, hihb, khv), in_range7a(b.y, lo_add, hihb, khv),
                              in_range7a(b.z, lo_add, hihb, khv), in_range7a(b.w, lo_add, hihb, khv));
    const uint32_t qm = (ABL & 16u) ? 0u : M3[k];
    if (__ballot((qm & ~okq) != 0)) {  // rare: exact range of this slice's quality bytes
      any_viol = true;
      qrange_accum(a, qm & 0xFFFFu, q);
      qrange_accum(b, qm >> 16, q);
    }
  }
  uint32_t info = t0;
  if (any_viol) info |= range_info(q);
  return info;
}

// A chunk without any newline lies inside ONE line (reads of kilobases: most chunks).  There is no type to speculate
// on, but both kinds of check can be made on all of its bytes, and the rank says later which one counts
// (chunk_info_redo / chunk_info_range).  A branch of its own in stream_pass1_body: the typed path is the 150 bp path
// and pays for every instruction.  Returns the chunk info word.
__device__ __forceinline__ uint32_t one_line_tests(const Piece32 (&v)[kHalves], QBounds boot) {
  uint32_t info = kInfoOneLine;
  const QBounds t = test_bounds(boot);
  const uint32_t lob = t.lo * 0x01010101u, hihb = ((t.hi & 0x7Fu) | 0x80u) * 0x01010101u;
  uint32_t not_base = 0, outside = 0;
#pragma unroll
  for (int k = 0; k < kHalves; ++k) {
    const uint32_t w[8] = {v[k].a.x, v[k].a.y, v[k].a.z, v[k].a.w, v[k].b.x, v[k].b.y, v[k].b.z, v[k].b.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      not_base |= not_acgtn7(w[j]);
      outside |= ~in_range7(w[j], lob, hihb) & kH;
    }
  }
  if (__ballot(not_base != 0)) info |= kInfoNotBases;  // (which byte: the repeated check finds it, if the line is a sequence)
  if (__ballot(outside != 0)) {  // rare: the exact range of the chunk's bytes
    QRange q{0x00FF00FFu, 0x00FF00FFu, 0u, 0u};
#pragma unroll
    for (int k = 0; k < kHalves; ++k) {
      qrange_accum(v[k].a, 0xFFFFu, q);
      qrange_accum(v[k].b, 0xFFFFu, q);
    }
    info |= range_info(q);
  }
  return info;
}

// ---- the chunk's results ----
__device__ __forceinline__ void write_chunk_results(const StreamOut& o, CallState* __restrict__ cs, const ChunkLane& c, uint32_t total,
                                                    uint32_t info, uint32_t flags) {
  if (c.lane == 0) {
    o.counts[c.chunk] = total;
    o.cinfo[c.chunk] = info;
    if (flags) atomicOr(&cs->flags, flags);
  }
}

}  // namespace fqg
#include "fqg_name_capture.h"  // capture_digests, capture_records: behind ChunkLane, NlRanks and Speculation
namespace fqg {

// block: which workgroup of the pass this is (chunks 4 block .. 4 block + 3), n_chunks: the pass ends in front of it
template <uint32_t ABL, int NAMES, bool WAVE_PACK>
__device__ __forceinline__ void stream_pass1_body(const uint8_t* __restrict__ img, uint64_t n, uint32_t n_chunks, const StreamOut& o,
                                                  CallState* __restrict__ cs, const NameCapture& nc, uint32_t block,
                                                  Pass1Lds<NAMES>& lds) {
  static_assert(NAMES == 0 || !(ABL & 7u), "the name capture needs the speculation, the staged entries and the copy");
  // (the wave index is uniform: telling the compiler keeps chunk-level values in scalar registers)
  const int lane = lane_id(), wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint8_t* const copy = lds.copy[wv] + (NAMES ? kCopyFront : 0u);
  const uint32_t chunk = block * (kBlock / kWave) + wv;
  if (chunk >= n_chunks) return;
  const uint64_t cb = (uint64_t)chunk * kChunkBytes;
  const ChunkLane c{chunk, cb, cb + (uint64_t)lane * kLaneBytes, cb + kChunkBytes + 4 <= n, lane, copy};
  const MarkPack<WAVE_PACK> pack(lane);
  const QBounds boot{cs->boot_qmin, cs->boot_qmax};

  uint32_t nl[kHalves];  // newline bits of the lane's 32 bytes, per slice
  Piece32 v[kHalves];    // the bytes themselves
  uint32_t tail = 0;     // the 4 bytes after the chunk (look-ahead of the last lane)
  uint32_t prev = '\n';  // NAMES: the byte in front of the chunk (the image starts behind a virtual newline)
  uint32_t flags = 0;    // image flags this chunk raises
  if (c.interior) load_marks_interior<ABL, NAMES>(img, c, pack, nl, v, tail, prev, flags);
  else {
    // Load and marks, edge form - the last one or two chunks: bytes may be missing, look-ahead may cross the end of the
    // image.  (Left here: as a function of its own, however it hands its marks back, these twenty lines cost the 150 bp
    // path of every pass-1 kernel eight more vector registers and a spill - docs/measurement_history.md.)
    uint32_t bad = 0;
#pragma unroll
    for (int k = 0; k < kHalves; ++k) {
      const uint64_t off = c.wb + (uint64_t)k * kHalfBytes;
      nl[k] = 0;
      v[k].a = v[k].b = make_uint4(0, 0, 0, 0);
      for (uint64_t i = off; i < n && i < off + kLaneBytes; ++i) {
        const uint32_t ch = img[i];
        if (ch == '\n') nl[k] |= 1u << (i - off);
        else if (ch == 0u) bad |= kFlagNul;
        else if (ch == '\r') bad |= kFlagCr;
        else if (ch >= 0x80u) bad |= kFlagHigh;
      }
    }
    if (__ballot((bad & kFlagNul) != 0)) flags |= kFlagNul;
    if (__ballot((bad & kFlagCr) != 0)) flags |= kFlagCr;
    if (__ballot((bad & kFlagHigh) != 0)) flags |= kFlagHigh;
  }
  const NlRanks r = rank_newlines(nl, flags);
  const LookAhead la = look_ahead(img, n, c, nl, tail);

  uint32_t info = kInfoUnknown;
  Speculation sp{false, 0};
  if (!(ABL & 1u) && c.interior && !(flags & kFlagHigh)) {
    sp = speculate(nl, r.ex, la.cand);
    uint32_t M1[kHalves], M3[kHalves];
    if (sp.found && chunk_type_spans(nl, r.ex, sp.t0, M1, M3)) info = typed_chunk_tests<ABL>(c, v, M1, M3, sp.t0, boot, pack, o, cs);
    else if (r.total == 0) info = one_line_tests(v, boot);
  }

  if (!(ABL & 2u)) {
    stage_chunk<ABL>(img, n, c.cb, c.chunk, nl, la.nl2, r.ex, r.staged, r.total <= (uint32_t)kStageCap, lds.slots[wv], c.copy, tail,
                     o.stage, c.interior);
  }
  if constexpr (NAMES == 2) capture_digests(img, n, c, nc, lds.slots[wv], prev == '\n', sp, r);
  if constexpr (NAMES == 1) capture_records(img, n, c, nc, lds.slots[wv], prev == '\n', sp, r);
  write_chunk_results(o, cs, c, r.total, info, flags);
}

// WAVE_PACK: for tools/kbench - the launch of its own keeps the v_dot4 packs (alone on the GPU it is 1.7 - 1.9 % slower with the
// MFMAs, docs/measurement_history.md); the launches that also carry line workers (k_stream_pass1_lines) gain by them.
// (waves_per_eu: with a register budget of at most 256 the compiler keeps the MFMA results of the mark packs in vector
// registers; without it they go to accumulation registers and come back through four v_accvgpr_read_b32 per pack)
template <uint32_t ABL, int NAMES = 0, bool WAVE_PACK = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_stream_pass1(const uint8_t* __restrict__ img, uint64_t n,
                                                         uint32_t n_chunks, StreamOut o,
                                                         CallState* __restrict__ cs, NameCapture nc = NameCapture{}) {
  __shared__ Pass1Lds<NAMES> lds;
  stream_pass1_body<ABL, NAMES, WAVE_PACK>(img, n, n_chunks, o, cs, nc, blockIdx.x, lds);
}

// ------------------------------------------------------------------------------------------
// pass 2: the per-chunk duties (k_stream_chunks) and the per-line / per-record duties (k_stream_lines)
// separately.  Its first form (k_stream_pass2, one wavefront per chunk; since removed) walked the image chunk
// by chunk, so a wavefront's line_end[] stores started wherever its first chunk's rank happened to fall, and the
// per-record statistics needed a further pass over the 32 B / record it had just written (k_records_fast).  Here a LANE OWNS A
// RECORD: it fetches the five staged entries that bound its four lines (2-byte loads, neighbouring lanes
// neighbouring addresses), writes the record's four line ends as one aligned 32-byte piece (a wavefront writes
// 2 KiB, aligned), checks the header starts, and derives the lengths, the statistics and the suspect bit from
// registers - the line index is written once and not read again.
// ------------------------------------------------------------------------------------------
struct ChunkRanks {
  const uint32_t* counts;              // newlines per chunk
  const uint32_t* local;               // exclusive prefix inside a span of kScanSpan chunks
  const unsigned long long* span_excl; // exclusive prefix over the spans
  uint32_t n_chunks;
  __device__ __forceinline__ uint64_t rank0(uint32_t c) const { return span_excl[c / kScanSpan] + local[c]; }
};

__global__ __launch_bounds__(kBlock) void k_stream_chunks(ChunkRanks cr, const uint32_t* __restrict__ cinfo, uint64_t limit,
                                                          uint32_t* __restrict__ redo, CallState* __restrict__ cs) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  const int lane = lane_id();
  bool again = false;
  if (c < cr.n_chunks) {
    const uint64_t rank0 = cr.rank0(c);
    const uint32_t cnt = cr.counts[c], info = cinfo[c];
    // only chunks that hold bytes of complete records need their byte checks to stand (a chunk that reaches
    // beyond the last complete record is repeated too: its quality range may include bytes of an incomplete one)
    if (rank0 < limit) {
      if (chunk_info_redo(info, (uint32_t)rank0) || rank0 + cnt >= limit) again = true;
      else if (chunk_info_range(info, (uint32_t)rank0)) {
        // (look first: the hull settles after a few chunks, and every later one would still be an atomic on one address)
        const uint32_t qlo = (info >> 8) & 0xFFu, qhi = (info >> 16) & 0xFFu;
        if (qlo < __atomic_load_n(&cs->qmin_byte, __ATOMIC_RELAXED)) atomicMin(&cs->qmin_byte, qlo);
        if (qhi > __atomic_load_n(&cs->qmax_byte, __ATOMIC_RELAXED)) atomicMax(&cs->qmax_byte, qhi);
      }
    }
  }
  // the redo list: one reservation per WORKGROUP (reads of kilobases send a quarter of their chunks here - a
  // reservation per wavefront was 33 000 atomics with a return value on one address, most of this kernel)
  __shared__ uint32_t s_cnt[kBlock / kWave], s_base;
  const unsigned long long am = __ballot(again);
  const int wv = (int)(threadIdx.x >> 6);
  if (lane == 0) s_cnt[wv] = (uint32_t)__builtin_popcountll(am);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) tot += s_cnt[w];
    s_base = tot ? atomicAdd(&cs->redo_count, tot) : 0u;
  }
  __syncthreads();
  if (again) {
    uint32_t at = s_base + (uint32_t)__builtin_popcountll(am & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) at += s_cnt[w];
    if (at < cr.n_chunks) redo[at] = c;
  }
}

// the chunk that holds the newline of rank R (R < total newlines): the LAST chunk whose first rank is <= R (chunks
// without newlines share their first rank with the chunk behind them).  `g` = where to start looking.
__device__ __forceinline__ uint32_t chunk_of_rank(const ChunkRanks& cr, uint64_t R, uint32_t g) {
  const uint32_t n = cr.n_chunks;
  if (g >= n) g = n - 1;
  uint32_t lo, hi, step = 1;  // invariant: rank0(lo) <= R and (hi == n or rank0(hi) > R)
  if (cr.rank0(g) <= R) {
    lo = g;
    for (;;) {
      const uint32_t t = lo + step;
      if (t >= n) {
        hi = n;
        break;
      }
      if (cr.rank0(t) <= R) {
        lo = t;
        step <<= 1;
      } else {
        hi = t;
        break;
      }
    }
  } else {
    hi = g;
    for (;;) {
      const uint32_t t = hi > step ? hi - step : 0;  // (rank0(0) = 0 <= R)
      if (cr.rank0(t) <= R) {
        lo = t;
        break;
      }
      hi = t;
      step <<= 1;
    }
  }
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (cr.rank0(mid) <= R) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct LinesArgs {
  const uint8_t* img;
  uint64_t n;                 // image bytes
  ChunkRanks cr;
  const uint16_t* stage;
  uint64_t* line_end;
  uint64_t line_cap;
  uint64_t n_newlines;        // ranks 0 .. n_newlines - 1 have a staged entry
  uint64_t n_lines;           // + 1 when the image ends in an unterminated line
  uint64_t limit;             // 4 * complete records
  uint32_t* suspect_bits;     // one bit per record; this kernel owns whole words
  uint64_t suspect_cap;
  unsigned int* flags;
  int space;
  uint32_t weight;
  AccState* acc;              // null: no statistics
  unsigned long long* hist;
  int ablate;                 // measurement only (FQGPU_LINES_ABL): 1 = no line-index stores
  // The line index on demand: a call that only validates never reads most of it back (32 B per record written for
  // nothing: 3.6 GB per 100 M records).  no_index: only the records that hold a line >= keep_from are stored (the last
  // complete record - its end is what the call consumed - and the lines of an incomplete one); index_only: the stores
  // and nothing else - the second run, when something does ask for the index (index_now in fqg_abi.hip).
  uint32_t no_index, index_only;
  uint64_t keep_from;
  uint64_t step_lo = 0, step_hi = 0;  // k_stream_lines_fast: the steps of this launch ([0, every step) by default)
};

constexpr int kLinesHist = 3072;
constexpr int kLinesPer = 2;  // records per lane and step: their staged-entry loads are in flight together (4: 1.29 -> 1.41 ms; 6 wavefronts per SIMD instead of 5: no change)

// the wavefront owns records g*64 .. g*64+63 = two whole words of the bitmap: it stores those that hold a suspect
__device__ __forceinline__ void store_suspect_words(uint32_t* bits, uint64_t g, unsigned long long sm) {
  const uint64_t w = g * 2;
  if ((uint32_t)sm) bits[w] = (uint32_t)sm;
  if ((uint32_t)(sm >> 32)) bits[w + 1] = (uint32_t)(sm >> 32);
}

// The end of a line kernel's workgroup.  Lane 0 of every wavefront brings the wavefront's counted records and their
// shortest and longest read (n_ok, min_rl, max_rl): through s_red they become one addition to the accumulator per
// workgroup.  Then the workgroup's LDS histogram of the lengths below N_HIST goes to A.hist.
template <int N_HIST>
__device__ __forceinline__ void lines_workgroup_end(const LinesArgs& A, unsigned long long (&s_red)[3][kBlock / kWave],
                                                    const uint32_t (&s_hist)[N_HIST], unsigned long long n_ok,
                                                    unsigned long long min_rl, unsigned long long max_rl) {
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / kWave; ++w) {
      n_ok += s_red[0][w];
      min_rl = s_red[1][w] < min_rl ? s_red[1][w] : min_rl;
      max_rl = s_red[2][w] > max_rl ? s_red[2][w] : max_rl;
    }
    if (n_ok) {
      atomicAdd(&A.acc->num_rds, n_ok * A.weight);
      if (min_rl < A.acc->min_rl) atomicMin(&A.acc->min_rl, min_rl);
      if (max_rl > A.acc->max_rl) atomicMax(&A.acc->max_rl, max_rl);
    }
  }
  for (int i = threadIdx.x; i < N_HIST; i += kBlock) {
    const uint32_t cc = s_hist[i];
    if (cc) atomicAdd(&A.hist[i], (unsigned long long)cc * A.weight);
  }
}

template <bool TODO>
__global__ __launch_bounds__(kBlock) void k_stream_lines(LinesArgs A, const uint8_t* __restrict__ todo) {
  __shared__ uint32_t s_hist[kLinesHist];
  __shared__ unsigned long long s_red[3][kBlock / kWave];
  __shared__ uint64_t s_wr0[kBlock / kWave][kWave];   // per wavefront: first rank of the window's chunks
  __shared__ uint32_t s_wcnt[kBlock / kWave][kWave];  // ... and their newline counts
  for (int i = threadIdx.x; i < kLinesHist; i += kBlock) s_hist[i] = 0;
  __syncthreads();
  const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
  uint32_t win0 = 0;
  // a step = kLinesPer * 64 consecutive records (kLinesPer * 256 lines) per wavefront
  const uint64_t n_groups = (A.n_lines + 4 * kWave - 1) / (4 * kWave);
  const uint64_t n_steps = (n_groups + kLinesPer - 1) / kLinesPer;
  // `todo` (what k_stream_lines_fast left over: one byte per step): only the steps it marks, each with a window
  // request of its own - they are few, or this kernel would have been launched alone
  const uint64_t wave0 = (uint64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const double chunks_per_line = A.n_newlines ? (double)A.cr.n_chunks / (double)A.n_newlines : 0.0;
  unsigned long long n_ok = 0, min_rl = ~0ull, max_rl = 0;
  // The window of the next step is REQUESTED here and looked at when that step begins: nothing is computed from the
  // loaded values before (no sum, no select - an instruction that reads a loaded value is where the wavefront waits for
  // it), and the request has no branch (a lane outside the chunk table asks for the last chunk; `nx_in` says so).
  unsigned long long nx_se = 0;
  uint32_t nx_loc = 0, nx_cnt = 0, nx_win = 0;
  bool nx_in = false;
  auto window_request = [&](uint64_t step) {
    const uint64_t g = (step < n_steps ? step : n_steps - 1) * kLinesPer;
    const uint64_t Rw = g ? 4 * g * kWave - 1 : 0;
    const double est = (double)Rw * chunks_per_line;
    uint32_t cw = est > 2.0 ? (uint32_t)(est - 2.0) : 0u;
    if (cw + kWave > A.cr.n_chunks) cw = A.cr.n_chunks > (uint32_t)kWave ? A.cr.n_chunks - kWave : 0u;
    const uint32_t cm = cw + (uint32_t)lane;
    nx_in = cm < A.cr.n_chunks;
    const uint32_t cl = nx_in ? cm : A.cr.n_chunks - 1;
    nx_se = A.cr.span_excl[cl / kScanSpan];
    nx_loc = A.cr.local[cl];
    nx_cnt = A.cr.counts[cl];
    nx_win = cw;
  };
  if (!TODO && wave0 < n_steps) window_request(wave0);
  // TODO: the marks of 64 consecutive steps at a time, a lane each (a wavefront that asked for them one by one waited
  // for 150 loads in a row to find its two or three steps: 66 of the 886 us of the line kernels)
  uint64_t blk = wave0 * (uint64_t)kWave, blk_cur = 0;
  unsigned long long marks = 0;
  for (uint64_t step = wave0;; step += n_waves) {
    if constexpr (TODO) {
      while (!marks && blk < n_steps) {
        const uint64_t s = blk + (uint64_t)lane;
        marks = __ballot(s < n_steps && todo[s] != 0);
        blk_cur = blk;
        blk += n_waves * (uint64_t)kWave;
      }
      if (!marks) break;
      step = blk_cur + (uint64_t)__builtin_ctzll(marks);
      marks &= marks - 1;
      window_request(step);
    } else if (step >= n_steps) break;
    // e[0] = end of the line before mine, e[1..4] = ends of my four lines; ent[] = their staged entries
    uint64_t e[kLinesPer][5];
    uint32_t ent[kLinesPer][5];
    bool have[kLinesPer][5];
    // The chunks this wavefront's ranks live in: a window of 64 chunks starting a little before the estimated
    // chunk of its first rank, loaded by all lanes at once into LDS.  A lane whose rank falls outside it (reads
    // of kilobases: few newlines per chunk) searches the chunk prefix on its own.
    s_wr0[wv][lane] = nx_in ? nx_se + nx_loc : ~0ull;
    s_wcnt[wv][lane] = nx_in ? nx_cnt : 0u;
    win0 = nx_win;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- phase 1a: where the entries are (LDS only, but for lanes outside the window) ----
    // (not a function of its own: with the window handed over by reference, by value or as LDS pointers the kernel came
    // out with six more vector registers - five wavefronts per SIMD become four on the marked steps - or eighty more
    // scalar instructions, docs/measurement_history.md)
    uint64_t at[kLinesPer][5];   // index into stage[] of the entry to fetch
    bool ld[kLinesPer][5];       // ... when there is one
#pragma unroll
    for (int q = 0; q < kLinesPer; ++q) {
      const uint64_t g = step * kLinesPer + q;
      const uint64_t r = g * kWave + (uint64_t)lane;   // my record
      const uint64_t L0 = 4 * r;                       // its first line
      uint64_t R = r ? L0 - 1 : 0;  // first rank to fetch
      const int k0 = r ? 0 : 1;
      e[q][0] = ~0ull;                 // (record 0: the line before starts at -1)
      ent[q][0] = (kClsAt << 12);      // ... and the image's first byte is checked directly below
      have[q][0] = r == 0;
      at[q][0] = 0;
      ld[q][0] = false;
      uint32_t c = 0, i = 0, cnt = 0;
      bool windowed = false;  // c is an index INTO the window (then counts come from LDS)
      if (R < A.n_newlines) {
        if (R >= s_wr0[wv][0] && (R < s_wr0[wv][kWave - 1] + s_wcnt[wv][kWave - 1])) {
          uint32_t lo = 0, hi = kWave;  // last window entry whose first rank is <= R
          while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_wr0[wv][mid] <= R) lo = mid;
            else hi = mid;
          }
          c = lo;
          i = (uint32_t)(R - s_wr0[wv][lo]);
          cnt = s_wcnt[wv][lo];
          windowed = true;
        } else {
          c = chunk_of_rank(A.cr, R, (uint32_t)((double)R * chunks_per_line));
          i = (uint32_t)(R - A.cr.rank0(c));
          cnt = A.cr.counts[c];
        }
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        if (k < k0) continue;
        at[q][k] = 0;
        ld[q][k] = false;
        if (R < A.n_newlines) {
          while (i >= cnt) {  // next chunk that holds a newline
            ++c;
            i = 0;
            if (windowed && c >= (uint32_t)kWave) {  // ran out of the window
              windowed = false;
              c += win0;
            }
            if (windowed) cnt = s_wcnt[wv][c];
            else cnt = __builtin_nontemporal_load(&A.cr.counts[c]);  // (a plain load here: the compiler merges the two into a load through a generic pointer and fails on it)
          }
          const uint32_t cg = windowed ? win0 + c : c;
          at[q][k] = (uint64_t)cg * kStageCap + i;
          ld[q][k] = true;
          ent[q][k] = 0;
          e[q][k] = (uint64_t)cg * kChunkBytes;  // (+ the entry's offset, below)
          have[q][k] = true;
          ++i;
        } else if (R == A.n_newlines && A.n_lines > A.n_newlines) {  // the unterminated last line
          ent[q][k] = 0;
          e[q][k] = A.n;
          have[q][k] = true;
        } else {
          ent[q][k] = 0;
          e[q][k] = 0;
          have[q][k] = false;
        }
        ++R;
      }
    }
    // ---- phase 1b: every request of the step, nothing else: the next step's window, then the kLinesPer * 5 staged
    // entries of the lane (a lane without an entry asks for entry 0) ----
    if constexpr (!TODO) window_request(step + n_waves);
    uint16_t raw[kLinesPer][5];
#pragma unroll
    for (int q = 0; q < kLinesPer; ++q)
#pragma unroll
      for (int k = 0; k < 5; ++k) raw[q][k] = A.stage[at[q][k]];
#pragma unroll
      for (int q = 0; q < kLinesPer; ++q)
#pragma unroll
        for (int k = 0; k < 5; ++k)
          if (ld[q][k]) ent[q][k] = raw[q][k];

    __builtin_amdgcn_wave_barrier();  // (the window is rewritten by the next step)
    // ---- phase 2: the line index, the checks, the statistics ----
#pragma unroll
    for (int q = 0; q < kLinesPer; ++q) {
      const uint64_t g = step * kLinesPer + q;
      const uint64_t r = g * kWave + (uint64_t)lane;
      const uint64_t L0 = 4 * r;
      {
        uint64_t R = r ? L0 - 1 : 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          if (k < (r ? 0 : 1)) continue;
          if (R < A.n_newlines) e[q][k] += (ent[q][k] & 0xFFFu);
          ++R;
        }
      }
      // four ends per lane, 32 contiguous bytes
      if ((A.ablate & 1) || (A.no_index && L0 + 4 <= A.keep_from)) {
      } else if (have[q][4] && L0 + 3 < A.line_cap) {
        typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
        u64x2 lo2, hi2;
        lo2.x = e[q][1]; lo2.y = e[q][2]; hi2.x = e[q][3]; hi2.y = e[q][4];
        __builtin_nontemporal_store(lo2, reinterpret_cast<u64x2*>(A.line_end + L0));
        __builtin_nontemporal_store(hi2, reinterpret_cast<u64x2*>(A.line_end + L0 + 2));
      } else {
#pragma unroll
        for (int k = 1; k < 5; ++k)
          if (have[q][k] && L0 + k - 1 < A.line_cap) A.line_end[L0 + k - 1] = e[q][k];
      }
      // checks (complete records only)
      bool sus = false, complete = have[q][4] && L0 + 3 < A.limit && !A.index_only, counted = false;
      uint64_t rl = 0;
      if (complete) {
        // header line: '@' and not empty; third line: exactly "+\n"  (what the entry BEFORE a line says about it)
        if (r == 0) sus |= A.img[0] != '@' || (A.n > 1 && A.img[1] == '\n');
        else sus |= !(((ent[q][0] >> 12) & 3u) == kClsAt && !((ent[q][0] >> 14) & 1u));
        sus |= !(((ent[q][2] >> 12) & 3u) == kClsPlus && ((ent[q][2] >> 14) & 1u));
        const uint64_t l0 = e[q][1] - e[q][0] - 1, l1 = e[q][2] - e[q][1] - 1, l2 = e[q][3] - e[q][2] - 1, l3 = e[q][4] - e[q][3] - 1;
        const uint32_t has_nl = e[q][4] < A.n ? 1u : 0u;  // only the very last line can lack it
        sus |= l1 < 1 || l1 != l3 || A.space != FQG_SPACE_SEQ;
        sus |= l0 + 1 > FQG_MAX_LABEL_LENGTH - 1 || l2 + 1 > FQG_MAX_LABEL_LENGTH - 1 ||
               l1 + 1 > FQG_MAX_READ_LENGTH - 1 || l3 + has_nl > FQG_MAX_READ_LENGTH - 1;
        counted = A.acc && l1 + 1 <= FQG_MAX_READ_LENGTH - 1;
        if (counted) {
          rl = l1 + 1;  // strlen(seq): the sequence line always ends in '\n' here
          ++n_ok;
          min_rl = rl < min_rl ? rl : min_rl;
          max_rl = rl > max_rl ? rl : max_rl;
        }
      }
      // the length histogram: reads of ONE length are the usual file, and 64 lanes adding 1 to one LDS word are 64
      // serialised atomics (they were most of this kernel's LDS cycles: SQ_LDS_BANK_CONFLICT 3.5x SQ_ACTIVE_INST_LDS in
      // profiles/r03b_pass1_sq_counters.json) - the lanes that share the first counted lane's length add once, together
      {
        const unsigned long long cm = __ballot(counted);
        if (cm) {
          const int first = __builtin_ctzll(cm);
          const uint32_t rl0 = (uint32_t)__builtin_amdgcn_readlane((uint32_t)rl, first);
          const bool with_first = counted && rl == (uint64_t)rl0;
          const unsigned long long same = __ballot(with_first);
          if (lane == first) {
            if (rl < (uint64_t)kLinesHist) atomicAdd(&s_hist[rl], (uint32_t)__builtin_popcountll(same));
            else atomicAdd(&A.hist[rl], (unsigned long long)A.weight * (unsigned long long)__builtin_popcountll(same));
          }
          if (counted && !with_first) {
            if (rl < (uint64_t)kLinesHist) atomicAdd(&s_hist[rl], 1u);
            else atomicAdd(&A.hist[rl], (unsigned long long)A.weight);
          }
        }
      }
      const unsigned long long sm = __ballot(sus);
      if (lane == 0 && sm) {
        if ((g + 1) * kWave <= A.suspect_cap) store_suspect_words(A.suspect_bits, g, sm);
        else atomicOr(A.flags, kFlagSuspectOverflow);
      }
    }
  }
  if (!A.acc) return;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    n_ok += __shfl_down(n_ok, d, 64);
    const unsigned long long a = __shfl_down(min_rl, d, 64), b = __shfl_down(max_rl, d, 64);
    min_rl = a < min_rl ? a : min_rl;
    max_rl = b > max_rl ? b : max_rl;
  }
  if (lane == 0) {
    s_red[0][threadIdx.x >> 6] = n_ok;
    s_red[1][threadIdx.x >> 6] = min_rl;
    s_red[2][threadIdx.x >> 6] = max_rl;
  }
  lines_workgroup_end(A, s_red, s_hist, n_ok, min_rl, max_rl);
}

// ------------------------------------------------------------------------------------------
// The same pass for the steps of an ordinary file - every record of the step complete, the newlines of its 513 ranks in
// at most kFastSlots pieces of 64 staged entries - without a search per lane: the WAVEFRONT fetches the staged entries
// of the chunks its ranks live in, piece by piece with all lanes (coalesced 2-byte loads, all pieces in flight
// together), and drops them into an LDS array BY RANK; a lane then finds the five entries of a record as five
// neighbouring words.  k_stream_lines above works out, per lane and record, which chunk a rank lives in (a binary
// search of the window, then a walk from chunk to chunk: 585 vector and 350 scalar instructions per 128 records,
// most of them 64-bit index arithmetic); here that is one comparison per window chunk.  Steps that do not qualify (the
// first and the last records of an image, reads of kilobases whose ranks spread over more chunks than the window
// holds, chunks with more than 64 newlines) are marked for the general kernel, which runs behind this one on the marks;
// an image whose chunks hold more than 64 newlines on average (reads below 100 bases) goes to the general kernel alone.
//
// What a step costs is vector-ALU issue, the currency pass 1 is short of when the two share a launch, so
// whatever is one fact per wavefront is kept in scalar registers: the step, the window's first chunk (fqg_line_window.h:
// integer arithmetic), the covering chunks, the flags of the call, the decision to store the index, the read length of
// a step whose records share one.  The wavefront's number within the workgroup is declared uniform (readfirstlane) for
// that: from threadIdx.x the compiler takes the whole step loop for divergent.
// ------------------------------------------------------------------------------------------
constexpr int kFastSlots = 16;
constexpr int kFastRanks = 4 * kWave * kLinesPer + 1;  // 513: the ranks of 128 records and the one in front of them
// a piece holds at most 64 of the 513 ranks: a step that qualifies is covered by 9 chunks or more, so the slots below
// this one are never tested against n_cov
constexpr int kFastSlotsMin = (kFastRanks + kWave - 1) / kWave;
constexpr uint32_t kFastRow = (uint32_t)((kFastRanks + 7) & ~3);  // words of s_ent per wavefront: the ranks, then 7 words nobody reads
static_assert(kFastSlotsMin == 9 && kFastSlotsMin <= kFastSlots, "slots of a step");
static_assert(kLineWindowChunks == (uint32_t)kWave, "a window chunk per lane");

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32);
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32);
}

// The histogram of the kernel without a search has a size of its own, below that of the general kernel (kLinesHist): with
// it LinesFastLds, and the union of k_stream_pass1_lines, fit an eighth of a CU's 160 KiB of LDS.  A length at or beyond it
// goes to A.hist by a global atomic, as lengths beyond kLinesHist do in the general kernel.
constexpr int kLinesFastHist = 3008;
struct LinesFastLds {
  uint32_t hist[kLinesFastHist];
  unsigned long long red[3][kBlock / kWave];
  __attribute__((aligned(16))) uint32_t ent[kBlock / kWave][kFastRow];
};
// worker / n_workers: which workgroup of the persistent grid this is; the steps it shares are [A.step_lo, A.step_hi)
// (step_hi = 0: up to the last step of the image)
__device__ __forceinline__ void stream_lines_fast_body(const LinesArgs& A, uint8_t* __restrict__ todo, uint32_t worker,
                                                       uint32_t n_workers, LinesFastLds& lds) {
  auto& s_hist = lds.hist;
  auto& s_red = lds.red;
  auto& s_ent = lds.ent;
  for (int i = threadIdx.x; i < kLinesFastHist; i += kBlock) s_hist[i] = 0;
  __syncthreads();
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* const row = &s_ent[wv][0];
  const uint64_t n_groups = (A.n_lines + 4 * kWave - 1) / (4 * kWave);
  const uint64_t n_steps_all = (n_groups + kLinesPer - 1) / kLinesPer;
  const uint64_t n_steps = uniform64(A.step_hi && A.step_hi < n_steps_all ? A.step_hi : n_steps_all);
  const uint64_t wave0 = uniform64(A.step_lo + (uint64_t)worker * (kBlock / kWave) + (uint64_t)wv);
  const uint64_t n_waves = (uint64_t)n_workers * (kBlock / kWave);
  const uint32_t n_chunks = (uint32_t)__builtin_amdgcn_readfirstlane((int)A.cr.n_chunks);
  LineWindow lw = line_window(n_chunks, A.n_newlines);
  lw.ratio = uniform64(lw.ratio);
  lw.round = uniform64(lw.round);
  lw.frac_bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)lw.frac_bits);
  lw.last = (uint32_t)__builtin_amdgcn_readfirstlane((int)lw.last);
  // the steps [1, whole_steps) have all their ranks staged, their records complete, room in the line index and in the
  // suspect bitmap: one comparison per step (Rhi = 512 step + 512 <= x is step < x / 512; 128 records a step)
  uint64_t whole_steps = A.n_newlines < A.limit ? A.n_newlines : A.limit;
  whole_steps = (whole_steps < A.line_cap ? whole_steps : A.line_cap) / kPartStepRanks;
  whole_steps = uniform64(whole_steps < A.suspect_cap / (kWave * kLinesPer) ? whole_steps : A.suspect_cap / (kWave * kLinesPer));
  // the flags of the call, once, as bits of a scalar word (a boolean the compiler keeps as a lane mask is tested with
  // two vector instructions each time)
  enum : uint32_t { kHasAcc = 1, kIndexOnly = 2, kNoIndex = 4, kStoreIndex = 8, kSusAll = 16 };
  const uint32_t call_flags = (uint32_t)__builtin_amdgcn_readfirstlane(
      (int)((A.acc ? kHasAcc : 0u) | (A.index_only ? kIndexOnly : 0u) | (A.no_index ? kNoIndex : 0u) |
            ((A.ablate & 1) ? 0u : kStoreIndex) | (A.space != FQG_SPACE_SEQ ? kSusAll : 0u)));
  const uint32_t lo12 = in_vgpr(0xFFFu);  // (a three-register v_bitop3 issues in 2 cycles, with a scalar operand in 4)
  // the lane's byte offset into the staged entries of a chunk, and into those of the eighth chunk behind it
  const uint32_t off0 = as_computed(2u * (uint32_t)lane), off8 = as_computed(2u * (uint32_t)lane + 8u * (kStageCap * 2));
  // Statistics and the length histogram.  Records of ONE length are the usual file: the records that share the length of
  // their group's first counted record are counted in a scalar register, a run of groups with the same length at a time
  // (run_len, run_cnt); when the length changes, and once behind the last step, the run goes to the histogram and to the
  // wavefront's count, minimum and maximum (u_*).  The other records of a group - none in the usual file - add
  // themselves to the histogram and to three words of the wavefront's row of s_ent that no entry reaches: nothing of
  // them lives in vector registers across the steps.  (A wavefront's share of the records and a step's lengths fit 32 bits.)
  constexpr uint32_t kOddOk = kFastRanks + 1, kOddMin = kFastRanks + 2, kOddMax = kFastRanks + 3;
  static_assert(kOddMax < kFastRow, "the words behind the dump word");
  if (lane == 0) {
    row[kOddOk] = 0;
    row[kOddMin] = ~0u;
    row[kOddMax] = 0;
  }
  uint32_t u_ok = 0, u_min = ~0u, u_max = 0;
  uint32_t run_len = 0, run_cnt = 0;
  auto run_flush = [&]() {
    if (!run_cnt) return;
    u_ok += run_cnt;
    u_min = run_len < u_min ? run_len : u_min;
    u_max = run_len > u_max ? run_len : u_max;
    if (lane == 0) {
      if (run_len < (uint32_t)kLinesFastHist) atomicAdd(&s_hist[run_len], run_cnt);
      else atomicAdd(&A.hist[run_len], (unsigned long long)A.weight * (unsigned long long)run_cnt);
    }
  };
  // the window of the NEXT step is requested a step ahead and looked at when that step begins (see k_stream_lines): lane
  // j asks for chunk cw + j - a scalar base and the lane's own offset, the last chunk where the table is shorter
  const bool whole = n_chunks >= (uint32_t)kWave;  // every window lies inside the chunk table
  const uint32_t beyond = as_computed((uint32_t)lane < n_chunks ? 0u : ~0u);  // (a vector register, not a lane mask to select by)
  unsigned long long nx_se = 0;
  uint32_t nx_loc = 0, nx_cnt = 0, nx_win = 0;
  auto window_request = [&](uint64_t step) {
    const uint64_t s = step < n_steps ? step : n_steps - 1;
    const uint32_t cw = line_window_start(lw, s ? s * kPartStepRanks - 1 : 0);
    uint32_t j = (uint32_t)lane;
    if (!whole) j = j < n_chunks ? j : n_chunks - 1;  // (cw = 0)
    const uint32_t in_span = ((cw % (uint32_t)kScanSpan) + j) / (uint32_t)kScanSpan;  // 0, or 1 behind a span's end
    nx_se = (A.cr.span_excl + cw / (uint32_t)kScanSpan)[in_span];
    nx_loc = (A.cr.local + cw)[j];
    nx_cnt = (A.cr.counts + cw)[j];
    nx_win = cw;
  };
  if (wave0 < n_steps) window_request(wave0);
  for (uint64_t step = wave0; step < n_steps; step += n_waves) {
    // lane j holds window chunk j: its first rank and its number of newlines
    uint64_t w0 = nx_se + nx_loc;
    uint32_t wc = nx_cnt;
    const uint32_t win0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)nx_win);  // (the same in every lane: scalar arithmetic below)
    w0 |= (uint64_t)beyond | ((uint64_t)beyond << 32);  // (lanes beyond a table of fewer than 64 chunks: ~0 and no newline)
    wc &= ~beyond;
    const uint64_t rb = step * (uint64_t)(kWave * kLinesPer);   // the step's first record
    const uint64_t Rlo = 4 * rb - 1, Rhi = 4 * rb + 4 * kWave * kLinesPer;  // its ranks: [Rlo, Rhi)
    bool fast = step > 0 && step < whole_steps;
    // the chunks the ranks live in: from the last chunk whose first rank is <= Rlo to the last whose first rank is < Rhi
    // (first ranks do not decrease along the window; lanes beyond the image hold ~0)
    const unsigned long long b_lo = __ballot(w0 <= Rlo), b_hi = __ballot(w0 < Rhi);
    // (every value below is the same in all lanes; saying so - readfirstlane - keeps it in scalar registers and the
    // branches scalar: the compiler cannot see it through the comparisons that made it)
    const int jfirst = __builtin_amdgcn_readfirstlane(__builtin_popcountll(b_lo) - 1);
    const int jlast = __builtin_amdgcn_readfirstlane(__builtin_popcountll(b_hi) - 1);
    const uint32_t n_cov = (uint32_t)(jlast - jfirst + 1);
    // where chunk j's first entry goes in s_ent (32-bit, may be "negative": the chunk begins in front of the step's ranks)
    const uint32_t rel0 = (uint32_t)(w0 - Rlo);
    if (fast && b_lo != 0 && n_cov >= (uint32_t)kFastSlotsMin && n_cov <= (uint32_t)kFastSlots) {
      // every covering chunk in ONE piece of 64 entries (reads of 100 bases and more), and the window holds the step's
      // last rank too.  (Chunk jfirst holds rank Rlo - the chunk behind it begins beyond - so with pieces of at most 64
      // its rel0 is -63 .. 0, and that of every covering chunk fits 32 bits.)
      const unsigned long long cover = (~0ull >> (63 - jlast)) & (~0ull << jfirst);
      const unsigned long long many = __ballot(wc > (uint32_t)kWave) & cover;
      const uint32_t last_rel = (uint32_t)__builtin_amdgcn_readlane((int)rel0, jlast);
      const uint32_t last_cnt = (uint32_t)__builtin_amdgcn_readlane((int)wc, jlast);
      fast = many == 0 && last_rel + last_cnt >= (uint32_t)kFastRanks;
    } else fast = false;
    if (!__builtin_amdgcn_readfirstlane((int)fast)) {
      if (lane == 0) todo[step] = 1;  // (its one owner writes it: no atomic - a counter all steps append to was 3.5 ms
                                      // of a 4.2 ms pass on reads of 30 - 150 bases, where no step qualifies)
      window_request(step + n_waves);
      continue;
    }
    // ---- every request of the step: the next step's window, then the staged entries chunk by chunk ----
    window_request(step + n_waves);
    // Slot sl takes the first 64 staged entries of chunk jfirst + sl, lane i entry i: one scalar base and the lane's own
    // offset, no test per lane.  A chunk with fewer newlines gives its last lanes whatever the stage holds behind its
    // entries (inside the chunk's kStageCap slots); those land where the entries of the chunks behind it belong and are
    // overwritten by them - the first ranks of consecutive chunks differ by the newlines of the chunk between them, and
    // the slots are written in order - or beyond the step's ranks, in the dump word.  Slots at and beyond n_cov are
    // skipped by scalar branches; the requests of the others are all issued before the first of them is used.
    constexpr uint32_t kDump = (uint32_t)kFastRanks;  // a word of s_ent nobody reads: where entries outside the step go
    const uint16_t* const base0 = A.stage + (uint64_t)(win0 + (uint32_t)jfirst) * kStageCap;  // (uniform: scalar arithmetic)
    // (the lane's offset as a 32-bit value of its own - off0, off8: a load takes the scalar base, the offset register and
    // a constant of up to 4 KiB, eight slots; left to itself the compiler adds base and lane to a 64-bit address per
    // wavefront and the constant to that, slot by slot, from the ninth slot on)
    const uint8_t* const base_b = reinterpret_cast<const uint8_t*>(base0);
    uint32_t raw[kFastSlots];
#pragma unroll
    for (int sl = 0; sl < kFastSlots; ++sl) {
      if (sl < kFastSlotsMin || (uint32_t)sl < n_cov) {
        const uint8_t* const mine = base_b + (sl < 8 ? off0 : off8);
        raw[sl] = *reinterpret_cast<const uint16_t*>(mine + (sl & 7) * (kStageCap * 2));
      }
      else raw[sl] = lo12;  // (any 32-bit value the compiler cannot see through: without one it keeps the sixteen as a
                            // tuple of registers it spills, with a constant it narrows them to 16 bits and widens each again)
    }
#pragma unroll
    for (int sl = 0; sl < kFastSlots; ++sl) {
      if (!(sl < kFastSlotsMin || (uint32_t)sl < n_cov)) continue;
      const uint32_t rel = (uint32_t)__builtin_amdgcn_readlane((int)rel0, jfirst + sl);
      uint32_t chunk_hi = (uint32_t)(jfirst + sl) << 16;
      asm("" : "+s"(chunk_hi));  // (one OR: what the compiler knows of the two halves it joins with a mask and a shift)
      const uint32_t val = chunk_hi | raw[sl];
      // chunk jfirst + sl begins at rank -63 .. 0 of the step (sl = 0), at 1 .. 64 sl behind it: only the first slot can
      // reach in front of the step's ranks, only those from 513 - 64 - 7 ranks on can reach beyond the row
      if (sl > 0 && 64 * sl + kWave - 1 < (int)kFastRow) row[rel + (uint32_t)lane] = val;
      else {
        const uint32_t idx = rel + (uint32_t)lane;  // >= 2^31 in front of the step
        row[idx < kDump ? idx : kDump] = val;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- the line index, the checks, the statistics: every record of the step is complete ----
#pragma unroll
    for (int q = 0; q < kLinesPer; ++q) {
      const uint64_t g = step * kLinesPer + q;  // (scalar, like everything made of it)
      uint32_t call = call_flags;
      asm volatile("" : "+s"(call));  // (tested where it is used: hoisted out of the loop the tests become lane masks)
      const uint32_t at = 4u * ((uint32_t)q * kWave + (uint32_t)lane);   // entry of rank 4r - 1
      const uint4 e03 = *reinterpret_cast<const uint4*>(&row[at]);  // (16-byte aligned: at is a multiple of 4)
      const uint32_t en[5] = {e03.x, e03.y, e03.z, e03.w, row[at + 4]};
      // positions relative to the window's first chunk, 32 bits (a step's ranks live in at most 16 chunks): the lengths
      // and the checks need no more; the 64-bit ends only where the index is stored.  An entry is chunk << 16 | staged
      // entry (offset 12 bits, class and look-ahead above them): the offset as it is under the chunk moved down by four
      uint32_t rel[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) rel[k] = __builtin_amdgcn_bitop3_b32(en[k] >> 4, en[k], lo12, 0xD8);  // (A & ~C) | (B & C)
      // the index: a group in front of keep_from stores nothing - its LAST record decides for all of them -, and the
      // addresses are formed only where something is stored
      if ((call & kStoreIndex) && !((call & kNoIndex) && 4 * (g * kWave + (kWave - 1)) + 4 <= A.keep_from)) {
        const uint64_t L0 = 4 * (g * kWave + (uint64_t)lane);
        if (!((call & kNoIndex) && L0 + 4 <= A.keep_from)) {
          typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
          const uint64_t wbase = (uint64_t)win0 * kChunkBytes;
          u64x2 lo2, hi2;
          lo2.x = wbase + rel[1]; lo2.y = wbase + rel[2]; hi2.x = wbase + rel[3]; hi2.y = wbase + rel[4];
          __builtin_nontemporal_store(lo2, reinterpret_cast<u64x2*>(A.line_end + L0));
          __builtin_nontemporal_store(hi2, reinterpret_cast<u64x2*>(A.line_end + L0 + 2));
        }
      }
      if (call & kIndexOnly) continue;
      // header line: '@' and not empty; third line: exactly "+\n"  (what the entry BEFORE a line says about it)
      bool sus = !(((en[0] >> 12) & 3u) == kClsAt && !((en[0] >> 14) & 1u));
      sus |= !(((en[2] >> 12) & 3u) == kClsPlus && ((en[2] >> 14) & 1u));
      const uint32_t l0 = rel[1] - rel[0] - 1, l1 = rel[2] - rel[1] - 1, l2 = rel[3] - rel[2] - 1, l3 = rel[4] - rel[3] - 1;
      sus |= l1 < 1 || l1 != l3;
      sus |= l0 + 1 > FQG_MAX_LABEL_LENGTH - 1 || l2 + 1 > FQG_MAX_LABEL_LENGTH - 1 ||
             l1 + 1 > FQG_MAX_READ_LENGTH - 1 || l3 + 1 > FQG_MAX_READ_LENGTH - 1;
      const uint32_t rl = l1 + 1;  // strlen(seq): the sequence line ends in '\n'
      // statistics and the length histogram (above; 64 lanes adding 1 to one LDS word are 64 serialised atomics, see
      // k_stream_lines)
      const unsigned long long cm = (call & kHasAcc) ? __ballot(rl <= FQG_MAX_READ_LENGTH - 1) : 0ull;
      if (cm) {
        const bool counted = rl <= FQG_MAX_READ_LENGTH - 1;
        const uint32_t rl0 = (uint32_t)__builtin_amdgcn_readlane((int)rl, __builtin_ctzll(cm));
        const unsigned long long same = __ballot(counted && rl == rl0);
        const uint32_t n_same = (uint32_t)__builtin_popcountll(same);
        if (rl0 != run_len) {
          run_flush();
          run_len = rl0;
          run_cnt = 0;
        }
        run_cnt += n_same;
        if (same != cm) {
          if (counted && rl != rl0) {
            atomicAdd(&row[kOddOk], 1u);
            atomicMin(&row[kOddMin], rl);
            atomicMax(&row[kOddMax], rl);
            if (rl < (uint32_t)kLinesFastHist) atomicAdd(&s_hist[rl], 1u);
            else atomicAdd(&A.hist[rl], (unsigned long long)A.weight);
          }
        }
      }
      const unsigned long long sm = (call & kSusAll) ? ~0ull : __ballot(sus);
      if (sm) {
        if (lane == 0) store_suspect_words(A.suspect_bits, g, sm);
      }
    }
    __builtin_amdgcn_wave_barrier();  // (s_ent is rewritten by the next step)
  }
  run_flush();
  if (!A.acc) return;
  // the wavefront's count, minimum and maximum: the scalar share and what the other records left in its row
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  unsigned long long n_ok = 0, min_rl = ~0ull, max_rl = 0;
  if (lane == 0) {
    const uint32_t odd_min = row[kOddMin], odd_max = row[kOddMax];
    const uint32_t lo = u_min < odd_min ? u_min : odd_min;
    n_ok = (unsigned long long)u_ok + row[kOddOk];
    min_rl = lo == ~0u ? ~0ull : (unsigned long long)lo;
    max_rl = u_max > odd_max ? u_max : odd_max;
    s_red[0][threadIdx.x >> 6] = n_ok;
    s_red[1][threadIdx.x >> 6] = min_rl;
    s_red[2][threadIdx.x >> 6] = max_rl;
  }
  lines_workgroup_end(A, s_red, s_hist, n_ok, min_rl, max_rl);
}

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_stream_lines_fast(LinesArgs A, uint8_t* __restrict__ todo) {
  __shared__ LinesFastLds lds;
  stream_lines_fast_body(A, todo, blockIdx.x, gridDim.x, lds);
}

// ------------------------------------------------------------------------------------------
// Pass 1 of one part of the image and the line workers of the part BEFORE it in ONE kernel (round 6).  Pass 1 is bound by
// vector-ALU cycles, the line kernel by the latency of its dependent loads: side by side they hide each other (two
// streams with priorities: 7.97 -> 7.58 ms, profiles/r04c_kbench_overlap.txt).  As one launch the overlap needs no second
// stream, no host in between, no priorities: the first `line_workers` workgroups are the persistent line workers - they
// start first and keep one slot per CU -, the others are pass-1 workgroups of chunks [chunk_first, n_chunks).  The line
// workers take what they need from DEVICE memory: the newline count behind the parts scanned so far (CallState::
// part_newlines, k_scan_b) gives their steps - every step whose ranks are all staged - and the flags that send an image
// to the two-pass path (NUL, CR, high bytes, a chunk with too many newlines) make them do nothing.  A part whose newline
// density the kernel without a search is not made for is left to the launches behind the parts, and so is every part
// after it: the steps the workers have done are [0, CallState::lines_done_steps), without a gap (fqg_part_steps.h).
// Their statistics go
// to accumulators the caller merges once the whole image has passed (k_acc_merge): a later part can still raise a flag.
// ------------------------------------------------------------------------------------------
// the mark packs of the pass-1 workgroups in this kernel: on the matrix pipe (61 / 62 / 61 vector registers).  With v_dot4
// (57 / 61 / 57) the three launches of a step are 4.96 ms against 4.88 ms at eight workgroups per CU
// (profiles/r18_ab_bench_waves.txt).
constexpr bool kFusedWavePack = true;
template <int NAMES>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_stream_pass1_lines(
    const uint8_t* __restrict__ img, uint64_t n, uint32_t chunk_first, uint32_t n_chunks, StreamOut o, CallState* __restrict__ cs,
    LinesArgs A, uint8_t* __restrict__ todo, uint32_t line_workers, uint32_t part /* whose lines: >= 0 */, NameCapture nc) {
  union Lds {
    Pass1Lds<NAMES> p1;
    LinesFastLds lf;
  };
  __shared__ Lds lds;
  // eight workgroups per CU, as k_stream_pass1 has alone: one is the line worker, seven are pass 1.  A byte more than an
  // eighth of the CU's 160 KiB and the hardware holds seven - six for pass 1, which is bound by what the vector ALU issues
  // and pays for every resident wavefront it loses.
  static_assert(sizeof(Lds) <= (160u << 10) / 8, "the LDS of k_stream_pass1_lines: eight workgroups per CU");
  if (blockIdx.x >= line_workers) {
    stream_pass1_body<0u, NAMES, kFusedWavePack>(img, n, n_chunks, o, cs, nc, chunk_first / (kBlock / kWave) + (blockIdx.x - line_workers), lds.p1);
    return;
  }
  // ---- a line worker: the steps of part `part`, from what the scans have left in the call state ----
  if (__hip_atomic_load(&cs->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (kFlagNul | kFlagCr | kFlagHigh | kFlagStageOverflow)) return;
  // (the host decides the same way for the whole image - stream_lines -, and begins at lines_done_steps: the workers of a
  // part run only directly behind the steps that are done, fqg_part_steps.h.  lines_done[part - 1] is of the launch before
  // this one, lines_done[part] for the next: nobody reads it in this launch)
  static_assert(kPartStepRanks == (uint64_t)(4 * kWave * kLinesPer), "a step of the line kernels");
  // (what is read here is the same in every lane, and every lane is active: saying so keeps it in scalar registers - as
  // vector values the three counts cost two vector registers more, and the kernel has 64 at eight wavefronts per SIMD: what
  // does not fit is scratch in a kernel whose other workgroups are pass 1)
  const unsigned long long R = readlane64(cs->part_newlines[part], 0), R0 = part ? readlane64(cs->part_newlines[part - 1], 0) : 0ull;
  const PartSteps ps = part_steps(R0, R, chunk_first, part ? readlane64(cs->lines_done[part - 1], 0) : 0ull);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cs->lines_done[part] = ps.done;
    if (ps.run) cs->lines_done_steps = ps.step_hi;
  }
  if (!ps.run) return;
  A.n_newlines = R;
  A.n_lines = R;
  A.limit = R & ~3ull;
  A.cr.n_chunks = chunk_first;
  A.step_lo = ps.step_lo;
  A.step_hi = ps.step_hi;  // full steps only: every rank of theirs has a staged entry
  if (A.step_hi <= A.step_lo) return;
  stream_lines_fast_body(A, todo, blockIdx.x, line_workers, lds.lf);
}

// the statistics of the line workers -> the caller's accumulator (discard: only the clearing), and the scratch cleared
__global__ __launch_bounds__(kBlock) void k_acc_merge(AccState* __restrict__ src, unsigned long long* __restrict__ src_hist,
                                                      AccState* __restrict__ dst, unsigned long long* __restrict__ dst_hist,
                                                      int discard) {
  __shared__ unsigned long long s_lo, s_hi;
  if (threadIdx.x == 0) {
    s_lo = src->min_rl;
    s_hi = src->max_rl;
  }
  __syncthreads();
  const unsigned long long lo = s_lo, hi = s_hi;
  if (lo <= hi)
    for (unsigned long long i = lo + (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i <= hi; i += (unsigned long long)gridDim.x * kBlock) {
      const unsigned long long v = src_hist[i];
      if (v) {
        if (!discard && dst_hist) atomicAdd(&dst_hist[i], v);
        src_hist[i] = 0;
      }
    }
  if (!discard && dst && blockIdx.x == 0 && threadIdx.x == 0 && src->num_rds) {
    atomicAdd(&dst->num_rds, src->num_rds);
    atomicMin(&dst->min_rl, src->min_rl);
    atomicMax(&dst->max_rl, src->max_rl);
  }
}
__global__ void k_acc_scratch_reset(AccState* __restrict__ a) {
  a->num_rds = 0;
  a->min_rl = FQG_MAX_READ_LENGTH;
  a->max_rl = 0;
  a->min_qbyte = 255;
  a->max_qbyte = 0;
}

// After every marking kernel: the suspect bitmap -> the list the exact validator walks; the image's quality range
// -> the statistics (what k_records_fast does at its end on the other paths)
__global__ __launch_bounds__(kBlock) void k_suspect_list(const uint32_t* __restrict__ bits, uint64_t n_records,
                                                         unsigned long long* __restrict__ list,
                                                         unsigned long long list_cap,
                                                         unsigned long long* __restrict__ list_count,
                                                         AccState* __restrict__ acc, const CallState* __restrict__ cs) {
  const uint64_t n_words = (n_records + 31) / 32;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  // one reservation per wavefront and step (a file whose every read is a suspect - lower-case bases, say - would
  // otherwise add to one address a hundred million times)
  const int lane = lane_id();
  for (uint64_t w0 = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); w0 < n_words; w0 += stride) {
    const uint64_t w = w0 + (uint64_t)lane;
    uint32_t m = w < n_words ? bits[w] : 0u;
    if (w * 32 + 32 > n_records) m &= w * 32 < n_records ? (uint32_t)((1ull << (n_records - w * 32)) - 1ull) : 0u;
    const uint32_t cnt = (uint32_t)__popc(m);
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (!total) continue;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(list_count, (unsigned long long)total);
    base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
    unsigned long long at = base + (incl - cnt);
    while (m) {
      const uint32_t j = (uint32_t)__builtin_ctz(m);
      m &= m - 1;
      if (at < list_cap) list[at] = w * 32 + j;
      ++at;
    }
  }
  if (acc && blockIdx.x == 0 && threadIdx.x == 0 && cs->qmin_byte <= cs->qmax_byte) {
    atomicMin(&acc->min_qbyte, cs->qmin_byte);
    atomicMax(&acc->max_qbyte, cs->qmax_byte);
  }
}

// queued suspect byte positions -> records
__global__ __launch_bounds__(kBlock) void k_stream_queue(const unsigned long long* __restrict__ queue,
                                                         unsigned long long queue_cap,
                                                         const uint64_t* __restrict__ line_end, uint64_t n_lines,
                                                         uint64_t n_records, SuspectMap suspect,
                                                         CallState* __restrict__ cs) {
  unsigned long long cnt = cs->queue_count;
  if (cnt > queue_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&cs->flags, kFlagQueueOverflow);
    cnt = queue_cap;
  }
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < cnt; i += stride) {
    const uint64_t pos = queue[i];
    // first line whose end is >= pos
    uint64_t lo = 0, hi = n_lines;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (line_end[mid] < pos) lo = mid + 1;
      else hi = mid;
    }
    const uint64_t rec = lo >> 2;
    if (rec < n_records) mark_suspect(suspect, rec);
  }
}

}  // namespace fqg
