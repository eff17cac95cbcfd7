// fqg_deflate_kernels.hip - gzip members compressed on the device (fqg_deflate / fqg_text_deflate, include/fqg.h).
//
// The text is cut at multiples of FQG_GZ_MEMBER_TEXT; every cut becomes one RFC 1952 member: the ten header bytes, ONE
// final deflate block (dynamic Huffman, or stored where that is no larger), CRC-32 and ISIZE.  k_deflate_members is a
// persistent grid of 256-thread workgroups, one member per workgroup at a time, the member's whole text in LDS:
//
//   stage     the text, with 16-byte loads, to the LDS address that has the source's alignment (`skew`)
//   crc       256 stripes of 255 bytes that END at the member's end (leading stripes of a short member are empty: zero
//             bytes in front do not move a zero CRC register), each by table look-ups; eight levels of
//             left = shift(left, bytes of right) ^ right with the GF(2) operators of 255 * 2^level bytes (GzTables)
//   match     256 positions a step: every lane hashes its four bytes, reads the newest EARLIER-STEP position with the same
//             hash, then all insert with atomicMax on position + 1 - the table after a step depends on positions alone,
//             never on the order lanes arrive in - and extends its candidate (and the one at distance 1, which the table
//             cannot hold inside a step: runs) word by word, up to 258 bytes, the member's end and 32768 back
//   parse     greedy, by wavefront 0 on the step's 256 match lengths: a ballot of the lanes that hold a match, the first
//             one at or behind `next` is taken, `next` moves behind it - one round per TAKEN match, none per literal.
//             Tokens go to the call's arena in order, their symbols into the LDS histograms; positions below `next` skip
//             their match search in the following steps
//   codes     fqg_deflate_codes.h: symbols ranked by count one per lane, the two trees on one lane each, the header
//   bits      token bit lengths -> (round, wavefront) sums -> one scan; pass two puts every token at its bit offset with
//             LDS atomicOr into the member image, which takes the hash table's place
//   flush     the image to the member's slot (stride kGzStride) with 16-byte stores, its size to sizes[member]
//
// k_deflate_gather then packs the slots at the offsets scan64 made of the sizes.  The bytes of a member are a function of
// its text alone: nothing above looks at the grid, at the member's number or at where the text lies.
//
// GzArgs::frame chooses what stands around the deflate block: the ten header bytes of a plain gzip member, or BGZF's
// eighteen (SAM/BAM specification 4.1: the extra field 'B' 'C' 2 0 BSIZE, BSIZE = the member's bytes - 1).  The block,
// CRC-32 and ISIZE are the same bytes in both; only the image's first bit (80 or 144) differs.
#pragma once
#include "fqg_deflate_codes.h"
#include "fqg_device.h"
#include "fqg_tile.h"

namespace fqg {

constexpr uint32_t kGzMember = FQG_GZ_MEMBER_TEXT;
constexpr uint32_t kGzStride = 65536;     // a member's slot: text + 23 at most (BGZF: + 31), whole 16-byte words
constexpr uint32_t kGzTextLds = kGzMember + 48;  // skew in front, the words an unaligned read touches behind
constexpr uint32_t kGzHashBits = 14;
constexpr uint32_t kGzTokStride = kGzMember + 64;  // tokens of one member (and the end-of-block) per workgroup
constexpr uint32_t kGzEob = 0xFFFFFFFFu, kGzMatch = 0x80000000u;
constexpr uint32_t kGzWindow = 32768;
static_assert(kGzMember % 255 == 0 && kGzMember / 255 == kBlock, "the CRC stripes are 255 bytes per thread");
constexpr uint32_t kGzFrameGzip = 0, kGzFrameBgzf = 1;
constexpr uint32_t kGzHeadGzip = 10, kGzHeadBgzf = 18;  // header bytes in front of the deflate block
static_assert(kGzMember + 23 + 16 <= kGzStride && (1u << kGzHashBits) * 4 == kGzStride, "the member image takes the hash table's place");
static_assert(kGzMember + (kGzHeadBgzf + 5 + 8) + 16 <= kGzStride && kGzMember + (kGzHeadBgzf + 5 + 8) - 1 <= 0xFFFFu,
              "a BGZF block fits its slot and BSIZE its sixteen bits");

struct GzTables {
  uint32_t crc[256];
  uint32_t shift[8][32];  // [level][bit]: the CRC register after 255 << level zero bytes, for a register of that one bit
};

struct GzArgs {
  const uint8_t* carry;  // text positions [0, carry_bytes)
  const uint8_t* src;    // ... and [carry_bytes, ...)
  uint64_t carry_bytes;  // (any length: whole members may lie inside it)
  uint32_t frame;        // kGzFrameGzip or kGzFrameBgzf
  uint64_t member_text;  // bytes that become members
  uint64_t n_members;
  uint8_t* slots;        // n_members x kGzStride
  uint32_t* sizes;       // bytes of every member
  uint32_t* toks;        // gridDim.x x kGzTokStride
  const GzTables* tab;
};

struct GzShared {
  dfl::CodeWork work[2];
  dfl::DynHeader hdr;
  uint32_t lit_freq[dfl::kMaxSyms], dist_freq[32];
  uint16_t lc[dfl::kMaxSyms], dc[32];
  uint8_t ll[dfl::kMaxSyms], dl[32];
  uint32_t step[kBlock];
  uint32_t crc_tab[256];
  uint32_t crc_part[kBlock];
  uint32_t sums[4 * kBlock + 4];
  uint32_t wave_tot[4];
  uint32_t next, ntok, used[2], crc;
};
constexpr uint32_t kGzLds = kGzTextLds + kGzStride + (uint32_t)sizeof(GzShared);
static_assert(kGzTextLds % 16 == 0 && kGzLds <= 160u * 1024u, "one workgroup's LDS");

// four text bytes at LDS byte address a (any alignment) of the word array w
__device__ __forceinline__ uint32_t gz_ld32(const uint32_t* w, uint32_t a) {
  return __builtin_amdgcn_alignbyte(w[(a >> 2) + 1], w[a >> 2], a & 3u);
}

// bytes [from + 4, ...) that agree between positions c < p (LDS addresses, the first four are known to agree): the
// length of the match, at most maxlen
__device__ __forceinline__ uint32_t gz_extend(const uint32_t* w, uint32_t c, uint32_t p, uint32_t maxlen) {
  uint32_t len = 4;
  while (len < maxlen) {
    const uint32_t x = gz_ld32(w, c + len) ^ gz_ld32(w, p + len);
    if (x) {
      len += (uint32_t)__builtin_ctz(x) >> 3;
      break;
    }
    len += 4;
  }
  return len < maxlen ? len : maxlen;
}

// nbits (<= 48) of v at bit `at` of the image
__device__ __forceinline__ void gz_or_bits(uint32_t* out, uint32_t at, uint64_t v, uint32_t nbits) {
  if (!nbits) return;
  const uint32_t w = at >> 5, sh = at & 31u;
  const uint64_t lo = v << sh;
  const uint32_t hi = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
  if ((uint32_t)lo) atomicOr(&out[w], (uint32_t)lo);
  if ((uint32_t)(lo >> 32)) atomicOr(&out[w + 1], (uint32_t)(lo >> 32));
  if (hi) atomicOr(&out[w + 2], hi);
}

// the bits of a token under the member's codes
__device__ __forceinline__ uint32_t gz_token_bits(const GzShared& S, uint32_t tok, uint64_t* value) {
  if (tok == kGzEob) {
    *value = S.lc[256];
    return S.ll[256];
  }
  if (!(tok & kGzMatch)) {
    *value = S.lc[tok];
    return S.ll[tok];
  }
  const uint32_t len = tok & 0x1FFu, dist = ((tok >> 9) & 0x7FFFu) + 1;
  const uint32_t ls = dfl::dc_len_sym(len), ds = dfl::dc_dist_sym(dist);
  uint64_t v = S.lc[257 + ls];
  uint32_t n = S.ll[257 + ls];
  v |= (uint64_t)(len - dfl::dc_len_base(ls)) << n;
  n += dfl::dc_len_extra(ls);
  v |= (uint64_t)S.dc[ds] << n;
  n += S.dl[ds];
  v |= (uint64_t)(dist - dfl::dc_dist_base(ds)) << n;
  n += dfl::dc_dist_extra(ds);
  *value = v;
  return n;
}

__device__ __forceinline__ uint32_t gz_wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t y = __shfl_up(v, d);
    if (lane >= d) v += y;
  }
  return v;
}

__device__ __forceinline__ uint32_t gz_crc_shift(const uint32_t* op, uint32_t v) {
  uint32_t r = 0;
#pragma unroll 4
  for (int b = 0; b < 32; ++b) r ^= (v >> b) & 1u ? op[b] : 0u;
  return r;
}

__global__ __launch_bounds__(kBlock) void k_deflate_members(GzArgs A) {
  extern __shared__ uint4 gz_lds[];
  uint8_t* const text8 = reinterpret_cast<uint8_t*>(gz_lds);
  const uint32_t* const textw = reinterpret_cast<const uint32_t*>(gz_lds);
  uint32_t* const hash = reinterpret_cast<uint32_t*>(text8 + kGzTextLds);  // ... and later the member's image
  uint8_t* const img8 = text8 + kGzTextLds;
  GzShared& S = *reinterpret_cast<GzShared*>(text8 + kGzTextLds + kGzStride);
  const int t = threadIdx.x, lane = t & (kWave - 1), wave = t >> 6;
  uint32_t* const toks = A.toks + (size_t)blockIdx.x * kGzTokStride;

  for (uint64_t m = blockIdx.x; m < A.n_members; m += gridDim.x) {
    const uint64_t L0 = m * kGzMember;
    const uint32_t n = (uint32_t)(A.member_text - L0 < kGzMember ? A.member_text - L0 : kGzMember);
    // ---- stage ----
    // A member wholly inside the carry is staged from the carry as from a source of its own (16-byte loads, the skew of
    // where it lies there); the member on the seam takes its carry part byte by byte, as a carry shorter than a member.
    const bool in_carry = L0 + n <= A.carry_bytes;
    const uintptr_t a0 = in_carry ? (uintptr_t)A.carry + (uintptr_t)L0
                                  : (uintptr_t)A.src + (uintptr_t)L0 - (uintptr_t)A.carry_bytes;  // where position L0 lies, or would lie
    const uint32_t skew = (uint32_t)(a0 & 15u);
    const uint32_t cpart = !in_carry && L0 < A.carry_bytes ? (uint32_t)(A.carry_bytes - L0) : 0u;  // (< n)
    if (n > cpart) {
      const uint4* g = reinterpret_cast<const uint4*>(a0 - skew);
      for (uint32_t k = ((skew + cpart) >> 4) + t; k < ((skew + n + 15) >> 4); k += kBlock) gz_lds[k] = g[k];
    }
    for (uint32_t k = t; k < (1u << kGzHashBits); k += kBlock) hash[k] = 0;
    for (uint32_t k = t; k < dfl::kMaxSyms; k += kBlock) S.lit_freq[k] = 0;
    if (t < 32) S.dist_freq[t] = 0;
    S.crc_tab[t] = A.tab->crc[t];
    if (t == 0) S.next = 0, S.ntok = 0, S.used[0] = 0, S.used[1] = 0;
    __syncthreads();
    for (uint32_t k = t; k < cpart; k += kBlock) text8[skew + k] = A.carry[L0 + k];  // (behind the words: they overlap it)
    __syncthreads();

    // ---- crc ----
    {
      uint32_t r = 0;
      if (n >= 4) {
        const int64_t lo = (int64_t)n - (int64_t)(kBlock - t) * 255;
        for (int64_t i = lo < 0 ? 0 : lo; i < lo + 255; ++i) {
          const uint32_t b = text8[skew + (uint32_t)i] ^ (i < 4 ? 0xFFu : 0u);  // (the register's start value, as text)
          r = S.crc_tab[(r ^ b) & 0xFFu] ^ (r >> 8);
        }
      } else if (t == kBlock - 1) {
        r = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < n; ++i) r = S.crc_tab[(r ^ text8[skew + i]) & 0xFFu] ^ (r >> 8);
      }
      S.crc_part[t] = r;
      for (int level = 0; level < 8; ++level) {
        __syncthreads();
        const int stride = 1 << level;
        if ((t & (2 * stride - 1)) == 0 && n >= 4) S.crc_part[t] = gz_crc_shift(A.tab->shift[level], S.crc_part[t]) ^ S.crc_part[t + stride];
      }
      __syncthreads();
      if (t == 0) S.crc = ~(n >= 4 ? S.crc_part[0] : S.crc_part[kBlock - 1]);
    }

    // ---- match and parse ----
    for (uint32_t base = 0; base < n; base += kBlock) {
      const uint32_t p = base + t;
      const bool can = p + 4 <= n;
      uint32_t w4 = 0, h = 0, cand = 0;
      if (can) {
        w4 = gz_ld32(textw, skew + p);
        h = (w4 * 0x9E3779B1u) >> (32 - kGzHashBits);
        cand = hash[h];
      }
      const uint32_t covered_to = S.next;
      __syncthreads();
      uint32_t found = 0;
      if (can) {
        atomicMax(&hash[h], p + 1);  // the newest position wins whoever comes first
        if (p >= covered_to) {
          const uint32_t maxlen = n - p < 258u ? n - p : 258u;
          uint32_t len = 0, dist = 0;
          if (cand && p + 1 - cand <= kGzWindow && gz_ld32(textw, skew + cand - 1) == w4) {
            len = gz_extend(textw, skew + cand - 1, skew + p, maxlen);
            dist = p + 1 - cand;
          }
          if (p && dist != 1 && len < maxlen && gz_ld32(textw, skew + p - 1) == w4) {
            const uint32_t l1 = gz_extend(textw, skew + p - 1, skew + p, maxlen);
            if (l1 >= len) len = l1, dist = 1;
          }
          // a match must pay for its distance (host/fq_fastdeflate.h)
          if (len >= 6 || (len == 5 && dist <= 4096) || (len == 4 && dist <= 512)) found = len | ((dist - 1) << 9);
        }
      }
      S.step[t] = found;
      __syncthreads();
      if (wave == 0) {
        uint32_t next = S.next, K = S.ntok;
        for (uint32_t wb = base; wb < base + kBlock && wb < n; wb += kWave) {
          const uint32_t v = S.step[wb - base + lane];
          const uint64_t valid = n - wb >= 64 ? ~0ull : (1ull << (n - wb)) - 1;
          const uint64_t mm = __ballot(v != 0);
          uint64_t lit = 0, sel = 0;
          uint32_t cur = next > wb ? next - wb : 0u;
          while (cur < 64) {
            const uint64_t rest = mm & (~0ull << cur);
            if (!rest) {
              lit |= ~0ull << cur;
              cur = 64;
              break;
            }
            const uint32_t f = (uint32_t)__builtin_ctzll(rest);
            lit |= (~0ull << cur) & ((1ull << f) - 1);
            sel |= 1ull << f;
            cur = f + (__shfl(v, (int)f) & 0x1FFu);
          }
          if (wb + cur > next) next = wb + cur;
          lit &= valid;
          const uint64_t tokens = lit | sel, below = (1ull << lane) - 1;
          const uint32_t at = K + (uint32_t)__popcll(tokens & below);
          K += (uint32_t)__popcll(tokens);
          if ((lit >> lane) & 1) {
            const uint32_t b = text8[skew + wb + lane];
            toks[at] = b;
            atomicAdd(&S.lit_freq[b], 1u);
          } else if ((sel >> lane) & 1) {
            toks[at] = kGzMatch | v;
            atomicAdd(&S.lit_freq[257 + dfl::dc_len_sym(v & 0x1FFu)], 1u);
            atomicAdd(&S.dist_freq[dfl::dc_dist_sym(((v >> 9) & 0x7FFFu) + 1)], 1u);
          }
        }
        if (lane == 0) S.next = next, S.ntok = K;
      }
      __syncthreads();
    }
    if (t == 0) {
      toks[S.ntok] = kGzEob;
      S.lit_freq[256] = 1;
    }
    __syncthreads();
    const uint32_t ntok = S.ntok + 1;

    // ---- codes: symbols ranked one per lane, the trees on lane 0 of wavefronts 0 and 1 ----
    for (uint32_t k = t; k < dfl::kMaxSyms; k += kBlock) {
      const uint32_t f = k < dfl::kLitSyms ? S.lit_freq[k] : 0u;
      S.work[0].freq[k] = f;
      if (f) atomicAdd(&S.used[0], 1u);
    }
    if (t < 32) {
      const uint32_t f = t < (int)dfl::kDistSyms ? S.dist_freq[t] : 0u;
      S.work[1].freq[t] = f;
      if (f) atomicAdd(&S.used[1], 1u);
    }
    for (uint32_t k = t; k < kGzStride / 16; k += kBlock) reinterpret_cast<uint4*>(img8)[k] = uint4{0, 0, 0, 0};
    __syncthreads();
    if (t == 0 && S.used[0] < 2) S.used[0] = dfl::dc_patch(S.work[0].freq, dfl::kLitSyms);
    if (t == kWave && S.used[1] < 2) S.used[1] = dfl::dc_patch(S.work[1].freq, dfl::kDistSyms);
    __syncthreads();
    for (uint32_t k = t; k < dfl::kLitSyms; k += kBlock)
      if (S.work[0].freq[k]) S.work[0].sym[dfl::dc_rank(S.work[0].freq, dfl::kLitSyms, k)] = (uint16_t)k;
    if (t < (int)dfl::kDistSyms && S.work[1].freq[t]) S.work[1].sym[dfl::dc_rank(S.work[1].freq, dfl::kDistSyms, t)] = (uint16_t)t;
    __syncthreads();
    if (t == 0) {
      dfl::dc_lengths_sorted(S.work[0], S.used[0], dfl::kLitSyms, 15, S.ll);
      dfl::dc_canonical_codes(S.ll, dfl::kLitSyms, S.lc);
    }
    if (t == kWave) {
      dfl::dc_lengths_sorted(S.work[1], S.used[1], dfl::kDistSyms, 15, S.dl);
      dfl::dc_canonical_codes(S.dl, dfl::kDistSyms, S.dc);
    }
    __syncthreads();
    if (t == 0) dfl::dc_build_header(S.ll, S.dl, S.hdr, S.work[0]);

    // ---- bits: lengths per (round, wavefront), their scan ----
    const uint32_t rounds = (ntok + kBlock - 1) / kBlock;
    for (uint32_t r = 0; r < rounds; ++r) {
      const uint32_t k = r * kBlock + t;
      uint64_t value;
      const uint32_t nb = k < ntok ? gz_token_bits(S, toks[k], &value) : 0u;
      const uint32_t incl = gz_wave_incl_scan(nb, lane);
      if (lane == kWave - 1) S.sums[r * 4 + wave] = incl;
    }
    __syncthreads();
    uint32_t body_bits;
    {
      uint32_t v[4], mine = 0;
      for (int i = 0; i < 4; ++i) {
        v[i] = (uint32_t)(t * 4 + i) < rounds * 4 ? S.sums[t * 4 + i] : 0u;
        mine += v[i];
      }
      const uint32_t incl = gz_wave_incl_scan(mine, lane);
      if (lane == kWave - 1) S.wave_tot[wave] = incl;
      __syncthreads();
      uint32_t before = incl - mine;
      for (int w = 0; w < wave; ++w) before += S.wave_tot[w];
      body_bits = S.wave_tot[0] + S.wave_tot[1] + S.wave_tot[2] + S.wave_tot[3];
      for (int i = 0; i < 4; ++i) {
        if ((uint32_t)(t * 4 + i) < rounds * 4) S.sums[t * 4 + i] = before;
        before += v[i];
      }
      __syncthreads();
    }
    const uint32_t dyn_bytes = (S.hdr.bits + body_bits + 7) >> 3, stored_bytes = 5 + n;
    const bool bgzf = A.frame == kGzFrameBgzf;
    const uint32_t head_bytes = bgzf ? kGzHeadBgzf : kGzHeadGzip;
    uint32_t block_bytes;
    if (dyn_bytes <= stored_bytes) {
      block_bytes = dyn_bytes;
      const uint32_t at0 = head_bytes * 8 + S.hdr.bits;
      if (t == 0) {
        if (bgzf) {  // 1f 8b 08 04 | mtime | 00 ff 06 00 | 'B' 'C' 02 00 | BSIZE (with the trailer, below)
          gz_or_bits(hash, 0, 0x04088B1Full, 32);
          gz_or_bits(hash, 64, 0x0006FF00ull, 32);
          gz_or_bits(hash, 96, 0x00024342ull, 32);
        } else {
          gz_or_bits(hash, 0, 0x00088B1Full, 32);
          gz_or_bits(hash, 64, 0x0304ull, 16);
        }
        uint32_t at = head_bytes * 8;
        dfl::dc_put_header(S.hdr, true, [&](uint32_t v, uint32_t nbits) {
          gz_or_bits(hash, at, v, nbits);
          at += nbits;
        });
      }
      for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t k = r * kBlock + t;
        uint64_t value = 0;
        const uint32_t nb = k < ntok ? gz_token_bits(S, toks[k], &value) : 0u;
        const uint32_t incl = gz_wave_incl_scan(nb, lane);
        gz_or_bits(hash, at0 + S.sums[r * 4 + wave] + incl - nb, value, nb);
      }
    } else {
      block_bytes = stored_bytes;
      if (t == 0) {
        if (bgzf) {
          const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
          for (int i = 0; i < 16; ++i) img8[i] = head[i];
        } else {
          const uint8_t head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 3};
          for (int i = 0; i < 10; ++i) img8[i] = head[i];
        }
        const uint8_t stored[5] = {1, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)(~n >> 8)};
        for (int i = 0; i < 5; ++i) img8[head_bytes + i] = stored[i];
      }
      for (uint32_t k = t; k < n; k += kBlock) img8[head_bytes + 5 + k] = text8[skew + k];
    }
    __syncthreads();
    const uint32_t member_bytes = head_bytes + block_bytes + 8;
    if (t < 8) img8[head_bytes + block_bytes + t] = (uint8_t)((t < 4 ? S.crc : n) >> (8 * (t & 3)));
    if (bgzf && (t == 8 || t == 9)) img8[16 + (t - 8)] = (uint8_t)((member_bytes - 1) >> (8 * (t - 8)));
    __syncthreads();
    // ---- flush ----
    {
      uint4* dst = reinterpret_cast<uint4*>(A.slots + m * kGzStride);
      const uint4* img = reinterpret_cast<const uint4*>(img8);
      for (uint32_t k = t; k < (member_bytes + 15) >> 4; k += kBlock) dst[k] = img[k];
      if (t == 0) A.sizes[m] = member_bytes;
    }
    __syncthreads();  // (the next member's staging writes what this one still read)
  }
}

// the members, slot by slot, to their places behind each other: off = local + sums of the sizes' scan64
__global__ __launch_bounds__(kBlock) void k_deflate_gather(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                           const unsigned long long* __restrict__ local,
                                                           const unsigned long long* __restrict__ sums, uint64_t n_members,
                                                           uint8_t* __restrict__ dst) {
  const uint32_t t = threadIdx.x;
  for (uint64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
    const uint32_t size = sizes[m];
    const uint8_t* s = slots + m * kGzStride;
    uint8_t* d = dst + local[m] + sums[m / kScan64Span];
    uint32_t lead = (uint32_t)(-(uintptr_t)d & 3u);
    if (lead > size) lead = size;
    if (t < lead) d[t] = s[t];
    const uint32_t nw = (size - lead) >> 2;
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(s);  // (a slot has whole words behind the member)
    uint32_t* dw = reinterpret_cast<uint32_t*>(d + lead);
    for (uint32_t j = t; j < nw; j += kBlock) {
      const uint32_t a = lead + 4 * j;
      dw[j] = __builtin_amdgcn_alignbyte(sw[(a >> 2) + 1], sw[a >> 2], a & 3u);
    }
    for (uint32_t i = lead + 4 * nw + t; i < size; i += kBlock) d[i] = s[i];
  }
}

}  // namespace fqg
