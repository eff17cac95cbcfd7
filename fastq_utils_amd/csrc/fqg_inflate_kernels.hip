// fqg_inflate_kernels.hip - the BGZF blocks of a file inflated on the device (fqg_bgzf_inflate, include/fqg.h).
//
// Every BGZF block is an independent raw deflate stream of at most 64 KiB whose payload, ISIZE and - the ISIZEs summed -
// place in the output are known from the headers before a bit is decoded: the host walks the headers and uploads one
// InfBlockRow per block, and k_inflate_blocks, a persistent grid with the blocks dealt by number, writes every block
// straight to its final place.  No scan, no gather.
//
// A workgroup is ONE wavefront and takes one block at a time.  A deflate stream is serial in its bit position, so lane 0
// walks it (fqg_inflate_core.h: inf_round, the state in registers for the length of a round) and the wavefront does what
// is not serial:
//   stage     the payload, kInfStage bytes at a time, with 16-byte loads to the LDS address that has the source's
//             alignment (the skewed staging of k_deflate_members); a new window whenever the walk comes within
//             kInfMargin of the staged end
//   tables    the look-up tables of a block's two codes, one sorted symbol per lane, from the lengths lane 0 parsed
//   copy      the queue of a round: up to kInfQueue matches and stored runs, in order, each by all lanes - a match with
//             distance >= length as a plain copy, an overlapping one as its period repeated (byte i comes from
//             i % distance of the pattern, which is complete: distance 1 is a run), a stored run from global memory.
//             Literals are NOT queued: a literal costs the walking lane one LDS store to its final place either way,
//             and the queue then holds sixty-four matches, not sixty-four symbols
//   window    the block's output, up to 65 536 bytes, lies in LDS until the block is done, at the LDS address that has
//             the destination's alignment
//   crc       256 stripes of 255 bytes that end at the block's end, four per lane, joined in eight levels with the GF(2)
//             operators of GzTables (as k_deflate_members); the up to 256 bytes in front of them (ISIZE > 65 280) by
//             lane 0, its register moved over the 65 280 bytes behind it by the last operator applied twice
//   flush     a good block to out + out_off: 16-byte stores for the words that lie wholly inside it, byte stores for the
//             up to 15 bytes at either end (the neighbours' bytes in those words belong to other workgroups)
// One wavefront, not 256 threads: the walk dominates, three more wavefronts would wait at every barrier of every round,
// and with one wavefront the entries of a queue need no barrier between them (a wavefront's LDS instructions execute in
// issue order: a fence of wavefront scope is enough); CRC and flush are a small part of a block's time with 64 lanes.
// LDS: 65 552 (window) + 4 112 (stage) + tables, queue, CRC scratch < 80 KiB: two workgroups per CU.
//
// Every validity decision is fqg_inflate_core.h's; per block the kernel writes the reason it was refused (0: good) and
// whether its CRC-32 differs from the stored one, and the first block of either kind by atomicMin.
#pragma once
#include "fqg_deflate_kernels.hip"
#include "fqg_inflate_core.h"

namespace fqg {

constexpr uint32_t kInfBlock = kWave;  // one wavefront
constexpr uint32_t kInfStage = 4096, kInfQueue = 64;
constexpr uint32_t kInfWinLds = inf::kInfMaxIsize + 16, kInfStageLds = kInfStage + 16;
constexpr uint32_t kInfCrcWrong = 1u << 16;  // in a block's status word, beside the reason
static_assert(kInfStage >= 2 * inf::kInfMargin + 16, "a fresh window holds more than one step");

struct InfBlockRow {
  uint64_t in_off;   // the payload in the file
  uint64_t out_off;  // the exclusive sum of the ISIZEs
  uint32_t in_len, isize;
};

struct InfArgs {
  const uint8_t* raw;  // the file; 16-byte words that hold a payload byte are loaded whole
  const InfBlockRow* rows;
  uint64_t n_blocks;
  uint8_t* out;
  uint32_t* status;           // per block: the reason | kInfCrcWrong
  unsigned long long* first;  // [0] the first refused block, [1] the first with a wrong CRC (atomicMin)
  const GzTables* tab;
};

struct InfShared {
  inf::InfCode lit, dist;
  inf::InfState st;
  uint64_t q[kInfQueue];
  uint32_t crc_tab[256];
  uint32_t crc_part[256];
  uint8_t lens[352];
};
constexpr uint32_t kInfLds = kInfWinLds + kInfStageLds + (((uint32_t)sizeof(InfShared) + 15u) & ~15u);
static_assert((kInfWinLds + kInfStageLds) % 16 == 0 && 2 * kInfLds <= 160u * 1024u, "two workgroups per CU");

__global__ __launch_bounds__(kInfBlock) void k_inflate_blocks(InfArgs A) {
  extern __shared__ uint4 inf_lds[];
  uint8_t* const win8 = reinterpret_cast<uint8_t*>(inf_lds);
  uint4* const stage16 = reinterpret_cast<uint4*>(win8 + kInfWinLds);
  uint8_t* const stage8 = win8 + kInfWinLds;
  InfShared& S = *reinterpret_cast<InfShared*>(win8 + kInfWinLds + kInfStageLds);
  const uint32_t lane = threadIdx.x;
  for (uint32_t k = lane; k < 256; k += kInfBlock) S.crc_tab[k] = A.tab->crc[k];

  for (uint64_t b = blockIdx.x; b < A.n_blocks; b += gridDim.x) {
    const InfBlockRow row = A.rows[b];
    if (row.isize == 0 || row.isize > inf::kInfMaxIsize) {  // (the end-of-file block: its payload is not looked at)
      if (lane == 0) A.status[b] = row.isize ? inf::kInfBadSize : 0u;
      if (lane == 0 && row.isize) atomicMin(&A.first[0], (unsigned long long)b);
      continue;
    }
    const uint32_t n = row.isize;
    uint8_t* const dst = A.out + row.out_off;
    const uint32_t oskew = (uint32_t)((uintptr_t)dst & 15u);
    uint8_t* const win = win8 + oskew;
    const uintptr_t g = (uintptr_t)A.raw + (uintptr_t)row.in_off;
    const uint8_t* const pay = reinterpret_cast<const uint8_t*>(g);
    __syncthreads();  // (the block before: its window and scratch are read no more)
    if (lane == 0) inf::inf_begin(S.st, row.in_len, n, win);
    __syncthreads();

    // ---- rounds ----
    for (;;) {
      const uint32_t wait = S.st.wait;
      if (wait == inf::kInfWaitDone) break;
      if (wait == inf::kInfWaitInput) {
        const uintptr_t at = g + inf::inf_byte_pos(S.st);
        const uintptr_t a0 = at & ~(uintptr_t)15, all = (g + row.in_len + 15) & ~(uintptr_t)15;
        const uintptr_t a1 = a0 + kInfStage < all ? a0 + kInfStage : all;  // (a0 <= all: the walk does not pass the end by a byte)
        const uint32_t words = a1 > a0 ? (uint32_t)((a1 - a0) >> 4) : 0u;   // <= kInfStage / 16
        const uint32_t lead = a0 < g ? (uint32_t)(g - a0) : 0u;             // bytes of the first word in front of the payload
        const uint4* src = reinterpret_cast<const uint4*>(a0);
        __syncthreads();
        for (uint32_t k = lane; k < words; k += kInfBlock) stage16[k] = src[k];
        __syncthreads();
        if (lane == 0) inf::inf_staged(S.st, stage8 + lead, (uint32_t)(a0 + lead - g), (uint32_t)(a0 + 16u * words - g));
      } else if (wait == inf::kInfWaitTables) {
        for (uint32_t k = lane; k < (1u << inf::kInfLitRoot); k += kInfBlock) inf::inf_fast_clear(S.lit, k);
        for (uint32_t k = lane; k < (1u << inf::kInfDistRoot); k += kInfBlock) inf::inf_fast_clear(S.dist, k);
        __syncthreads();
        const uint32_t nl = S.lit.n_sorted, nd = S.dist.n_sorted, nlen = S.st.nlen;
        for (uint32_t i = lane; i < nl && i < 288u; i += kInfBlock) inf::inf_fast_fill(S.lit, S.lens, i);
        for (uint32_t i = lane; i < nd && i < 32u; i += kInfBlock) inf::inf_fast_fill(S.dist, S.lens + (nlen <= 288u ? nlen : 288u), i);
      }
      __syncthreads();
      if (lane == 0) {
        inf::InfState st = S.st;  // (in registers for the round; the two pointers spelled as the LDS addresses they are)
        st.win = win;
        st.buf = stage8 + (st.buf ? (uint32_t)(st.buf - stage8) : 0u);
        inf::inf_round(st, S.lit, S.dist, S.lens, S.q, kInfQueue);
        S.st = st;
      }
      __syncthreads();
      // The queue in order.  Lane k holds entry k; each entry is broadcast from its lane and copied by all lanes.  Between
      // two entries stands a fence of WAVEFRONT scope, not a workgroup barrier: the workgroup is this one wavefront, whose
      // LDS instructions are executed in the order they were issued, so a load of the next entry sees what the stores
      // of this one wrote whichever lanes wrote it; the fence keeps the compiler from moving one across the other.
      const uint32_t ntok = S.st.ntok <= kInfQueue ? S.st.ntok : kInfQueue;
      const uint64_t mine = lane < ntok ? S.q[lane] : 0ull;
      for (uint32_t k = 0; k < ntok; ++k) {
        const uint64_t tok = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(mine >> 32), (int)k) << 32) | (uint32_t)__shfl((int)(uint32_t)mine, (int)k);
        const uint32_t o = inf::inf_tok_out(tok), len = inf::inf_tok_len(tok), arg = inf::inf_tok_arg(tok);
        if (o + len <= n) {  // (the core queued nothing else)
          if (inf::inf_tok_kind(tok) == inf::kInfTokStored) {
            if ((uint64_t)arg + len <= row.in_len)
              for (uint32_t i = lane; i < len; i += kInfBlock) win[o + i] = pay[arg + i];
          } else if (arg && arg <= o) {
            if (arg >= len)
              for (uint32_t i = lane; i < len; i += kInfBlock) win[o + i] = win[o - arg + i];
            else
              for (uint32_t i = lane; i < len; i += kInfBlock) win[o + i] = win[o - arg + i % arg];
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      __syncthreads();
    }
    const uint32_t status = S.st.status;

    // ---- crc ----
    uint32_t wrong = 0;
    if (status == inf::kInfOk) {
      const uint32_t head = n > kGzMember ? n - kGzMember : 0u, m = n - head;  // stripes over [head, n)
      const uint8_t* const text = win + head;
      for (uint32_t s4 = 0; s4 < 4; ++s4) {
        const uint32_t t = lane * 4 + s4;
        uint32_t r = 0;
        const int64_t lo = (int64_t)m - (int64_t)(256 - t) * 255;
        for (int64_t i = lo < 0 ? 0 : lo; i < lo + 255; ++i) {
          const uint32_t x = text[(uint32_t)i] ^ (!head && i < 4 ? 0xFFu : 0u);  // (the register's start value, as text)
          r = S.crc_tab[(r ^ x) & 0xFFu] ^ (r >> 8);
        }
        S.crc_part[t] = r;
      }
      for (uint32_t level = 0; level < 8; ++level) {
        __syncthreads();
        const uint32_t stride = 1u << level;
        for (uint32_t k = lane; k < (128u >> level); k += kInfBlock) {
          const uint32_t t = k * 2 * stride;
          S.crc_part[t] = gz_crc_shift(A.tab->shift[level], S.crc_part[t]) ^ S.crc_part[t + stride];
        }
      }
      __syncthreads();
      uint32_t crc = 0;
      if (lane == 0) {
        if (head || m < 4) {  // what stands in front of the stripes, or a text too short to carry the start value
          uint32_t r = 0xFFFFFFFFu;
          const uint32_t upto = head ? head : m;
          for (uint32_t i = 0; i < upto; ++i) r = S.crc_tab[(r ^ win[i]) & 0xFFu] ^ (r >> 8);
          if (head) r = gz_crc_shift(A.tab->shift[7], gz_crc_shift(A.tab->shift[7], r)) ^ S.crc_part[0];  // over 2 * (255 << 7) bytes
          crc = ~r;
        } else crc = ~S.crc_part[0];
        const uint8_t* z = pay + row.in_len;
        const uint32_t stored = (uint32_t)z[0] | ((uint32_t)z[1] << 8) | ((uint32_t)z[2] << 16) | ((uint32_t)z[3] << 24);
        wrong = crc != stored;
      }
      // ---- flush ----
      const uint32_t a = oskew, e = oskew + n, w0 = (a + 15) >> 4, w1 = e >> 4;  // whole words [w0, w1)
      uint8_t* const d0 = dst - oskew;
      if (w0 < w1) {
        uint4* dw = reinterpret_cast<uint4*>(d0);
        for (uint32_t k = w0 + lane; k < w1; k += kInfBlock) dw[k] = inf_lds[k];
        for (uint32_t i = a + lane; i < w0 * 16; i += kInfBlock) d0[i] = win8[i];
        for (uint32_t i = w1 * 16 + lane; i < e; i += kInfBlock) d0[i] = win8[i];
      } else {
        for (uint32_t i = a + lane; i < e; i += kInfBlock) d0[i] = win8[i];
      }
    }
    if (lane == 0) {
      A.status[b] = status | (wrong ? kInfCrcWrong : 0u);
      if (status != inf::kInfOk) atomicMin(&A.first[0], (unsigned long long)b);
      if (wrong) atomicMin(&A.first[1], (unsigned long long)b);
    }
  }
}

}  // namespace fqg
