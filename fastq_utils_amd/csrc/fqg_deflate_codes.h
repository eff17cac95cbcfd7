// fqg_deflate_codes.h - the code construction of a dynamic deflate block (RFC 1951 3.2.7): length-limited Huffman code
// lengths from symbol counts, canonical codes, and the run-length coded header that carries the lengths.
//
// The device compressor (fqg_deflate_kernels.hip) builds one code per gzip member with it; the text restates what the
// host compressor does (host/fq_fastdeflate.h: code_lengths, canonical_codes, flush_block's header) without the standard
// library and without a stack frame of its own: all scratch lives in a CodeWork the caller provides (LDS on the device).
// The order of the symbols by count is split from the tree so that a workgroup can rank the symbols in parallel
// (dc_rank: one symbol per lane) and leave only the linear part to one lane; dc_code_lengths is the serial whole.
//
// No HIP header is needed: a CPU program includes this file and runs the very text the kernel compiles
// (tests/test_deflate_codes.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQG_DC_HD __host__ __device__ inline
#else
#define FQG_DC_HD inline
#endif

namespace fqg {
namespace dfl {

constexpr unsigned kLitSyms = 286, kDistSyms = 30, kClSyms = 19, kMaxSyms = 288;
constexpr unsigned kMaxHeaderSyms = kLitSyms + kDistSyms;  // entries of the run-length coded sequence, at most

struct CodeWork {                // scratch of one dc_lengths_sorted
  uint32_t f[2 * kMaxSyms];      // node counts: leaves in order of count, inner nodes behind them in creation order
  uint16_t left[2 * kMaxSyms], right[2 * kMaxSyms];  // children (inner nodes only)
  uint16_t depth[2 * kMaxSyms];
  uint16_t sym[kMaxSyms];        // rank -> symbol: the used symbols in order of (count, symbol)
  uint32_t freq[kMaxSyms];       // the counts the code is built from (dc_patch: at least two of them non-zero)
};

// an inflater wants a complete code: at least two symbols get one.  Returns the number of used symbols.
FQG_DC_HD unsigned dc_patch(uint32_t* freq, unsigned n) {
  unsigned used = 0;
  for (unsigned s = 0; s < n; ++s) used += freq[s] != 0;
  for (unsigned s = 0; used < 2 && s < n; ++s)
    if (!freq[s]) {
      freq[s] = 1;
      ++used;
    }
  return used;
}

// place of symbol s among the used symbols in order of (count, symbol); freq[s] != 0
FQG_DC_HD unsigned dc_rank(const uint32_t* freq, unsigned n, unsigned s) {
  const uint32_t fs = freq[s];
  unsigned r = 0;
  for (unsigned t = 0; t < n; ++t) {
    const uint32_t ft = freq[t];
    r += (ft != 0) & ((ft < fs) | ((ft == fs) & (t < s)));
  }
  return r;
}

// Code lengths (<= maxbits) of the m >= 2 used symbols W.sym[0, m) (in order of count, W.freq their counts) into
// lens[0, n); unused symbols get 0.  Two queues: the sorted leaves and the inner nodes, whose counts never decrease.
// Limiting the lengths is zlib's gen_bitlen: every node deeper than maxbits is counted, every leaf deeper than it is
// lifted to it, and each round of the loop makes one place for two of the lifted by sending a leaf of the deepest
// level that still has one a level down.  The rarest symbols then take the longest codes.
FQG_DC_HD void dc_lengths_sorted(CodeWork& W, unsigned m, unsigned n, unsigned maxbits, uint8_t* lens) {
  for (unsigned i = 0; i < m; ++i) W.f[i] = W.freq[W.sym[i]];
  unsigned leaf = 0, inner = m, next = m;
  while ((m - leaf) + (next - inner) > 1) {
    unsigned pick[2];
    for (unsigned k = 0; k < 2; ++k) {
      if (leaf < m && (inner >= next || W.f[leaf] <= W.f[inner])) pick[k] = leaf++;
      else pick[k] = inner++;
    }
    W.f[next] = W.f[pick[0]] + W.f[pick[1]];
    W.left[next] = (uint16_t)pick[0];
    W.right[next] = (uint16_t)pick[1];
    ++next;
  }
  unsigned bl_count[16];
  for (unsigned b = 0; b < 16; ++b) bl_count[b] = 0;
  int overflow = 0;
  W.depth[next - 1] = 0;
  for (unsigned i = next; i-- > 0;) {  // from the root down: children have smaller indices than their parent
    const unsigned d = W.depth[i];
    if (d > maxbits) ++overflow;
    if (i >= m) {
      W.depth[W.left[i]] = (uint16_t)(d + 1);
      W.depth[W.right[i]] = (uint16_t)(d + 1);
    } else {
      ++bl_count[d < maxbits ? d : maxbits];
    }
  }
  while (overflow > 0) {
    unsigned bits = maxbits - 1;
    while (bl_count[bits] == 0) --bits;
    --bl_count[bits];
    bl_count[bits + 1] += 2;
    --bl_count[maxbits];
    overflow -= 2;
  }
  for (unsigned s = 0; s < n; ++s) lens[s] = 0;
  unsigned at = 0;
  for (unsigned b = maxbits; b >= 1; --b)
    for (unsigned k = 0; k < bl_count[b]; ++k) lens[W.sym[at++]] = (uint8_t)b;
}

// the whole on one thread: counts freq_in[0, n) -> lens[0, n)
FQG_DC_HD void dc_code_lengths(const uint32_t* freq_in, unsigned n, unsigned maxbits, uint8_t* lens, CodeWork& W) {
  for (unsigned s = 0; s < n; ++s) W.freq[s] = freq_in[s];
  const unsigned m = dc_patch(W.freq, n);
  for (unsigned s = 0; s < n; ++s)
    if (W.freq[s]) W.sym[dc_rank(W.freq, n, s)] = (uint16_t)s;
  dc_lengths_sorted(W, m, n, maxbits, lens);
}

FQG_DC_HD uint32_t dc_reverse(uint32_t c, unsigned nbits) {
  uint32_t r = 0;
  for (unsigned i = 0; i < nbits; ++i) {
    r = (r << 1) | (c & 1u);
    c >>= 1;
  }
  return r;
}

// canonical codes of lens[0, n), bit-reversed: ready to be put LSB first
FQG_DC_HD void dc_canonical_codes(const uint8_t* lens, unsigned n, uint16_t* codes) {
  unsigned count[16], next[16];
  for (unsigned b = 0; b < 16; ++b) count[b] = 0;
  for (unsigned s = 0; s < n; ++s) ++count[lens[s]];
  count[0] = 0;
  unsigned code = 0;
  next[0] = 0;
  for (unsigned b = 1; b <= 15; ++b) {
    code = (code + count[b - 1]) << 1;
    next[b] = code;
  }
  for (unsigned s = 0; s < n; ++s) codes[s] = lens[s] ? (uint16_t)dc_reverse(next[lens[s]]++, lens[s]) : (uint16_t)0;
}

// The header of a dynamic block: HLIT, HDIST, HCLEN, the code-length code and the two length arrays as one run-length
// coded sequence.
struct DynHeader {
  uint8_t sym[kMaxHeaderSyms], extra[kMaxHeaderSyms];  // the sequence: symbols 0..18 and the extra bits of 16 / 17 / 18
  uint32_t ncl, hlit, hdist, hclen;
  uint8_t cll[kClSyms];   // lengths (<= 7) and codes of the code-length code
  uint16_t clc[kClSyms];
  uint32_t bits;          // of the whole header, the three bits of BFINAL and BTYPE included
};

FQG_DC_HD unsigned dc_cl_order(unsigned k) {
  const uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return order[k];
}
FQG_DC_HD unsigned dc_cl_extra_bits(unsigned sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }

// ll[0, 286), dl[0, 30): the lengths of the two codes
FQG_DC_HD void dc_build_header(const uint8_t* ll, const uint8_t* dl, DynHeader& H, CodeWork& W) {
  unsigned hlit = kLitSyms, hdist = kDistSyms;
  while (hlit > 257 && !ll[hlit - 1]) --hlit;
  while (hdist > 1 && !dl[hdist - 1]) --hdist;
  H.hlit = hlit;
  H.hdist = hdist;
  const unsigned total = hlit + hdist;
  uint32_t cl_freq[kClSyms];
  for (unsigned k = 0; k < kClSyms; ++k) cl_freq[k] = 0;
  unsigned ncl = 0;
  for (unsigned k = 0; k < total;) {
    const unsigned v = k < hlit ? ll[k] : dl[k - hlit];
    unsigned run = 1;
    while (k + run < total && (k + run < hlit ? ll[k + run] : dl[k + run - hlit]) == v) ++run;
    unsigned left = run;
    if (v == 0) {
      while (left >= 11) {
        const unsigned r = left < 138u ? left : 138u;
        H.sym[ncl] = 18, H.extra[ncl++] = (uint8_t)(r - 11);
        left -= r;
      }
      if (left >= 3) {
        H.sym[ncl] = 17, H.extra[ncl++] = (uint8_t)(left - 3);
        left = 0;
      }
    } else {
      H.sym[ncl] = (uint8_t)v, H.extra[ncl++] = 0;
      --left;
      while (left >= 3) {
        const unsigned r = left < 6u ? left : 6u;
        H.sym[ncl] = 16, H.extra[ncl++] = (uint8_t)(r - 3);
        left -= r;
      }
    }
    while (left) {
      H.sym[ncl] = (uint8_t)v, H.extra[ncl++] = 0;
      --left;
    }
    k += run;
  }
  H.ncl = ncl;
  for (unsigned k = 0; k < ncl; ++k) ++cl_freq[H.sym[k]];
  dc_code_lengths(cl_freq, kClSyms, 7, H.cll, W);
  dc_canonical_codes(H.cll, kClSyms, H.clc);
  unsigned hclen = kClSyms;
  while (hclen > 4 && !H.cll[dc_cl_order(hclen - 1)]) --hclen;
  H.hclen = hclen;
  uint32_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
  for (unsigned k = 0; k < ncl; ++k) bits += H.cll[H.sym[k]] + dc_cl_extra_bits(H.sym[k]);
  H.bits = bits;
}

// the header's bits through put(value, nbits), nbits <= 16
template <class Put>
FQG_DC_HD void dc_put_header(const DynHeader& H, bool final, Put&& put) {
  put(final ? 1u : 0u, 1u);
  put(2u, 2u);
  put(H.hlit - 257, 5u);
  put(H.hdist - 1, 5u);
  put(H.hclen - 4, 4u);
  for (unsigned k = 0; k < H.hclen; ++k) put((uint32_t)H.cll[dc_cl_order(k)], 3u);
  for (unsigned k = 0; k < H.ncl; ++k) {
    const unsigned s = H.sym[k];
    put((uint32_t)H.clc[s], (uint32_t)H.cll[s]);
    if (s >= 16) put((uint32_t)H.extra[k], dc_cl_extra_bits(s));
  }
}

// length 3..258 -> symbol 0..28 (+257), extra bits, base; distance 1..32768 -> symbol 0..29, extra bits, base
FQG_DC_HD unsigned dc_len_sym(unsigned len) {  // len in 3..258
  if (len == 258) return 28;
  const unsigned l = len - 3;
  if (l < 8) return l;
  const unsigned e = (31u - (unsigned)__builtin_clz(l)) - 2;  // extra bits
  return 4 * e + 4 + ((l >> e) & 3u);
}
FQG_DC_HD unsigned dc_len_extra(unsigned sym) { return sym < 8 || sym == 28 ? 0u : (sym - 4) >> 2; }
FQG_DC_HD unsigned dc_len_base(unsigned sym) {
  if (sym < 8) return sym + 3;
  if (sym == 28) return 258;
  const unsigned e = (sym - 4) >> 2;
  return ((4 + (sym & 3u)) << e) + 3;
}
FQG_DC_HD unsigned dc_dist_sym(unsigned dist) {  // dist in 1..32768
  const unsigned d = dist - 1;
  if (d < 4) return d;
  const unsigned e = (31u - (unsigned)__builtin_clz(d)) - 1;
  return 2 * e + 2 + ((d >> e) & 1u);
}
FQG_DC_HD unsigned dc_dist_extra(unsigned sym) { return sym < 4 ? 0u : (sym - 2) >> 1; }
FQG_DC_HD unsigned dc_dist_base(unsigned sym) {
  if (sym < 4) return sym + 1;
  const unsigned e = (sym - 2) >> 1;
  return ((2 + (sym & 1u)) << e) + 1;
}

}  // namespace dfl
}  // namespace fqg
