// fqg_inflate_core.h - the decoder of one BGZF block's raw deflate stream (RFC 1951): the decode tables from code
// lengths, the parse of a dynamic block's header, and EVERY validity decision.  The device inflater
// (fqg_inflate_kernels.hip) and its CPU model (tests/cxx/inflate_model.cpp) both get their verdicts from this text; no
// standard library, no stack of its own beyond a few scalars: the state, the tables and the queue live where the caller
// puts them (LDS on the device).
//
// The verdict is the one of zlib's inflate() called raw (-15) with Z_FINISH and exactly ISIZE bytes of room, a block
// with an empty window in front: good iff the stream reaches the end-of-block of its final deflate block having written
// exactly ISIZE bytes; compressed bytes behind that point are not looked at.  The decisions follow zlib's inflate.c /
// inftrees.c in the order of the stream:
//   block type 3; a stored block whose LEN != ~NLEN; HLIT > 286 or HDIST > 30; a code-length code that is
//   over-subscribed or incomplete; a repeat with nothing to repeat or past HLIT + HDIST; no code for end-of-block; an
//   over-subscribed literal/length or distance code; an incomplete one unless its longest code has ONE bit (zlib's
//   inflate_table: "left > 0 && (type == CODES || max != 1)" - a single one-bit code, of either alphabet; a distance
//   alphabet without any code is complete enough as long as none is used); a bit pattern no symbol owns; length symbols
//   286 / 287 and distance symbols 30 / 31; a distance beyond what this block has written; output past ISIZE or short of
//   it at the end; input that ends before the final block does.
//
// How it runs.  inf_round() is ONE lane's serial walk: it decodes symbols until something needs the other lanes, and
// says what in InfState::wait -
//   kInfWaitInput   the staged window of the payload is used up: stage [pos, ...) again
//   kInfWaitTables  a block header was parsed (or a fixed block begun): fill the look-up tables (inf_fast_clear /
//                   inf_fast_fill, one entry of the sorted symbols per call: any lane may take any entry)
//   kInfWaitDrain   the queue is full: copy its matches and stored runs
//   kInfWaitDone    the stream is over: `status` is the verdict
// Literals are written by the walking lane itself, straight to their place in the output; matches and stored runs go to
// the queue with the output position they start at, and must be copied IN ORDER (a match may read what an earlier one
// wrote) before the next round.
//
// Bounds.  The bit reader never reads outside [base, stage_end) of `buf` nor at or behind `end` (zeros stand in, and
// the position says afterwards that the input was over); nothing is written or queued beyond ISIZE; every table index
// that comes from input is masked or range-checked where it is used.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQG_INF_HD __host__ __device__ inline
#else
#define FQG_INF_HD inline
#endif

namespace fqg {
namespace inf {

// why a block was refused (include/fqg_codes.h: FQG_E_INFLATE_* have these values)
constexpr uint32_t kInfOk = 0, kInfBadType = 32, kInfBadStored = 33, kInfBadHeader = 34, kInfBadCode = 35, kInfBadDistance = 36,
                   kInfBadSize = 37, kInfBadInput = 38;

constexpr uint32_t kInfMaxIsize = 65536;
constexpr uint32_t kInfLitRoot = 10, kInfDistRoot = 8;  // bits the look-up tables resolve at once
constexpr uint32_t kInfMargin = 1024;  // bytes one step may read at most (a dynamic header: 71 + 316 * 14 bits = 562 bytes)
constexpr uint32_t kInfWaitNone = 0, kInfWaitInput = 1, kInfWaitTables = 2, kInfWaitDrain = 3, kInfWaitDone = 4;
constexpr uint32_t kInfTokMatch = 1, kInfTokStored = 2;

// One canonical code: the symbols in order of (length, symbol), how many of every length, and a table over the next
// `root` bits of input for the codes that short: (symbol << 4) | length, 0 where a longer code (or none) begins.
struct InfCode {
  uint16_t count[16];
  uint16_t offs[16];   // where the symbols of a length start in sym[]
  uint16_t first[16];  // the canonical code of the first of them
  uint16_t sym[288];
  uint16_t n_sorted;   // symbols with a code
  uint16_t root;
  uint16_t fast[1u << kInfLitRoot];
};

struct InfState {
  // input: payload bytes [0, end); buf[k] is byte base + k for base + k < stage_end
  const uint8_t* buf;
  uint32_t base, stage_end, end;
  uint32_t pos;    // the next byte the reader loads (runs on past `end`: zeros)
  uint32_t nbits;  // bits in hold
  uint64_t hold;
  // output
  uint8_t* win;  // ISIZE bytes of room
  uint32_t out, isize;
  // the walk
  uint32_t in_block;  // inside a Huffman block: the tables stand
  uint32_t last;      // ... of the final block
  uint32_t wait, status;
  uint32_t ntok;
  uint32_t nlen, ndist;  // of the block's codes: lens[0, nlen) and lens[nlen, nlen + ndist) at kInfWaitTables
};

// a queued copy: kind, where it starts in the output, its length, and the distance (match) or payload offset (stored)
FQG_INF_HD uint64_t inf_tok(uint32_t kind, uint32_t out, uint32_t len, uint32_t arg) {
  return (uint64_t)out | ((uint64_t)kind << 17) | ((uint64_t)len << 19) | ((uint64_t)arg << 36);
}
FQG_INF_HD uint32_t inf_tok_out(uint64_t t) { return (uint32_t)t & 0x1FFFFu; }
FQG_INF_HD uint32_t inf_tok_kind(uint64_t t) { return (uint32_t)(t >> 17) & 3u; }
FQG_INF_HD uint32_t inf_tok_len(uint64_t t) { return (uint32_t)(t >> 19) & 0x1FFFFu; }
FQG_INF_HD uint32_t inf_tok_arg(uint64_t t) { return (uint32_t)(t >> 36) & 0x1FFFFu; }

FQG_INF_HD void inf_begin(InfState& s, uint32_t payload_bytes, uint32_t isize, uint8_t* win) {
  s.buf = nullptr;
  s.base = s.stage_end = 0;
  s.end = payload_bytes;
  s.pos = 0;
  s.nbits = 0;
  s.hold = 0;
  s.win = win;
  s.out = 0;
  s.isize = isize;
  s.in_block = 0;
  s.last = 0;
  s.status = kInfOk;
  s.ntok = 0;
  s.nlen = s.ndist = 0;
  s.wait = kInfWaitInput;
  if (isize > kInfMaxIsize) {  // (the callers refuse such a file before they come here)
    s.status = kInfBadSize;
    s.wait = kInfWaitDone;
  }
}

// the caller staged payload bytes [base, stage_end) at buf
FQG_INF_HD void inf_staged(InfState& s, const uint8_t* buf, uint32_t base, uint32_t stage_end) {
  s.buf = buf;
  s.base = base;
  s.stage_end = stage_end < s.end ? stage_end : s.end;
  if (s.wait == kInfWaitInput) s.wait = kInfWaitNone;
}

// the byte position the next unread bit lies in (bits of whole bytes still in hold are given back)
FQG_INF_HD uint32_t inf_byte_pos(const InfState& s) { return s.pos - (s.nbits >> 3); }

FQG_INF_HD void inf_refill(InfState& s) {
  if (s.nbits <= 32 && s.pos >= s.base && s.stage_end - s.pos >= 4 && s.pos < s.stage_end) {  // four loads that do not wait for each other
    const uint8_t* p = s.buf + (s.pos - s.base);
    const uint64_t w = (uint64_t)p[0] | ((uint64_t)p[1] << 8) | ((uint64_t)p[2] << 16) | ((uint64_t)p[3] << 24);
    s.hold |= w << s.nbits;
    s.nbits += 32;
    s.pos += 4;
  }
  while (s.nbits < 32) {  // (at a window's or the payload's end; no step uses more than 32 bits between two refills)
    uint64_t b = 0;
    if (s.pos >= s.base && s.pos < s.stage_end) b = s.buf[s.pos - s.base];
    s.hold |= b << s.nbits;
    s.nbits += 8;
    ++s.pos;
  }
}
FQG_INF_HD uint32_t inf_bits(InfState& s, uint32_t n) {  // n <= 16; the hold has them (inf_refill leaves 32 bits or more)
  const uint32_t v = (uint32_t)s.hold & ((1u << n) - 1u);
  s.hold >>= n;
  s.nbits -= n;
  return v;
}
// has the walk used bits the payload does not have?
FQG_INF_HD bool inf_overrun(const InfState& s) { return (uint64_t)s.pos * 8 - s.nbits > (uint64_t)s.end * 8; }
// would a step of at most kInfMargin bytes leave the staged window?
FQG_INF_HD bool inf_starved(const InfState& s) {
  const uint32_t p = inf_byte_pos(s);
  return s.stage_end < s.end && (p < s.base || p + kInfMargin > s.stage_end);
}

// count / offs / first / sym of the code with these lengths (each <= 15).  Returns 0 for a complete code, 1 for an
// incomplete one, -1 for an over-subscribed one; *max_len: its longest code.
FQG_INF_HD int inf_code_build(InfCode& c, const uint8_t* lens, uint32_t n, uint32_t root, uint32_t* max_len) {
  for (uint32_t l = 0; l < 16; ++l) c.count[l] = 0;
  for (uint32_t k = 0; k < n; ++k) ++c.count[lens[k] & 15u];
  c.root = (uint16_t)root;
  int left = 1;
  uint32_t mx = 0, at = 0, code = 0;
  c.offs[0] = 0;
  c.first[0] = 0;
  for (uint32_t l = 1; l < 16; ++l) {
    left <<= 1;
    left -= (int)c.count[l];
    if (left < 0) return -1;
    if (c.count[l]) mx = l;
    code = (code + (l > 1 ? c.count[l - 1] : 0u)) << 1;
    c.first[l] = (uint16_t)code;
    c.offs[l] = (uint16_t)at;
    at += c.count[l];
  }
  c.n_sorted = (uint16_t)at;  // (<= n <= 288)
  for (uint32_t k = 0; k < n; ++k) {  // (offs runs along as the cursor of its length and is set back: no array of its own)
    const uint32_t l = lens[k] & 15u;
    if (l) c.sym[c.offs[l]++] = (uint16_t)k;
  }
  for (uint32_t l = 1; l < 16; ++l) c.offs[l] = (uint16_t)(c.offs[l] - c.count[l]);
  *max_len = mx;
  return left > 0 ? 1 : 0;
}

FQG_INF_HD void inf_fast_clear(InfCode& c, uint32_t k) {  // k < 1 << root
  c.fast[k & ((1u << kInfLitRoot) - 1u)] = 0;
}
// the table entries of sorted symbol i < n_sorted (no other i writes them: the code is prefix-free)
FQG_INF_HD void inf_fast_fill(InfCode& c, const uint8_t* lens, uint32_t i) {
  const uint32_t s = c.sym[i], l = lens[s] & 15u, root = c.root;
  if (!l || l > root) return;
  const uint32_t code = (uint32_t)c.first[l] + (i - c.offs[l]);
  uint32_t rev = 0;
  for (uint32_t b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
  const uint16_t e = (uint16_t)((s << 4) | l);
  for (uint32_t k = rev & ((1u << root) - 1u); k < (1u << root); k += 1u << l) c.fast[k] = e;
}

// the next symbol of the code from the hold (refilled: 32 bits are there, a code and its extra bits take 28 at most); -1: a bit pattern no symbol owns
FQG_INF_HD int inf_decode(InfState& s, const InfCode& c) {
  const uint32_t e = c.fast[(uint32_t)s.hold & ((1u << c.root) - 1u)];
  if (e) {
    s.hold >>= (e & 15u);
    s.nbits -= (e & 15u);
    return (int)(e >> 4);
  }
  uint32_t code = 0, first = 0, index = 0;  // (puff.c's walk: one bit at a time from the shortest length up)
  for (uint32_t l = 1; l < 16; ++l) {
    code |= (uint32_t)(s.hold >> (l - 1)) & 1u;
    const uint32_t count = c.count[l];
    if (code < first + count) {
      s.hold >>= l;
      s.nbits -= l;
      const uint32_t k = index + (code - first);
      return k < 288u ? (int)c.sym[k] : -1;
    }
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return -1;
}

FQG_INF_HD uint32_t inf_len_base(uint32_t k) {  // k = symbol - 257 < 29
  return k < 8 ? 3 + k : k == 28 ? 258u : 3u + ((4u + (k & 3u)) << ((k >> 2) - 1u));
}
FQG_INF_HD uint32_t inf_len_extra(uint32_t k) { return k < 8 || k == 28 ? 0u : (k >> 2) - 1u; }
FQG_INF_HD uint32_t inf_dist_base(uint32_t k) {  // k < 30
  return k < 4 ? 1 + k : 1u + ((2u + (k & 1u)) << ((k >> 1) - 1u));
}
FQG_INF_HD uint32_t inf_dist_extra(uint32_t k) { return k < 4 ? 0u : (k >> 1) - 1u; }

FQG_INF_HD void inf_refuse(InfState& s, uint32_t why) {
  s.status = why;
  s.wait = kInfWaitDone;
}

// both codes from lens[0, nlen) and lens[nlen, nlen + ndist); false: refused
FQG_INF_HD bool inf_codes(InfState& s, InfCode& lit, InfCode& dist, const uint8_t* lens, uint32_t nlen, uint32_t ndist) {
  uint32_t mx = 0;
  s.nlen = nlen;
  s.ndist = ndist;
  int rc = inf_code_build(lit, lens, nlen, kInfLitRoot, &mx);
  if (rc < 0 || (rc > 0 && mx != 1)) return inf_refuse(s, kInfBadHeader), false;
  rc = inf_code_build(dist, lens + nlen, ndist, kInfDistRoot, &mx);
  if (rc < 0 || (rc > 0 && mx > 1)) return inf_refuse(s, kInfBadHeader), false;  // (mx == 0: no distance codes at all)
  return true;
}

// The header of a dynamic block into lens[0, 320): HLIT, HDIST, HCLEN, the code-length code (built in `lit`, which the
// literal/length code replaces afterwards), the run-length coded lengths.  false: refused.
FQG_INF_HD bool inf_dynamic_header(InfState& s, InfCode& lit, InfCode& dist, uint8_t* lens) {
  inf_refill(s);
  const uint32_t nlen = inf_bits(s, 5) + 257, ndist = inf_bits(s, 5) + 1, ncode = inf_bits(s, 4) + 4;
  if (nlen > 286 || ndist > 30) return inf_refuse(s, kInfBadHeader), false;
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  for (uint32_t k = 0; k < 19; ++k) lens[k] = 0;
  for (uint32_t k = 0; k < ncode; ++k) {  // (ncode <= 19)
    inf_refill(s);
    lens[order[k]] = (uint8_t)inf_bits(s, 3);
  }
  uint32_t mx = 0;
  if (inf_code_build(lit, lens, 19, 7, &mx) != 0 || mx == 0) return inf_refuse(s, kInfBadHeader), false;
  for (uint32_t k = 0; k < 128; ++k) inf_fast_clear(lit, k);
  for (uint32_t i = 0; i < lit.n_sorted; ++i) inf_fast_fill(lit, lens, i);
  const uint32_t total = nlen + ndist;  // <= 316
  uint32_t have = 0;
  while (have < total) {
    inf_refill(s);
    const int sym = inf_decode(s, lit);
    if (sym < 0 || sym > 18) return inf_refuse(s, kInfBadHeader), false;
    if (sym < 16) {
      lens[32 + have++] = (uint8_t)sym;
      continue;
    }
    uint32_t len = 0, copy;
    if (sym == 16) {
      if (!have) return inf_refuse(s, kInfBadHeader), false;
      len = lens[32 + have - 1];
      copy = 3 + inf_bits(s, 2);
    } else if (sym == 17) copy = 3 + inf_bits(s, 3);
    else copy = 11 + inf_bits(s, 7);
    if (have + copy > total) return inf_refuse(s, kInfBadHeader), false;
    while (copy--) lens[32 + have++] = (uint8_t)len;
  }
  if (inf_overrun(s)) return inf_refuse(s, kInfBadInput), false;
  if (lens[32 + 256] == 0) return inf_refuse(s, kInfBadHeader), false;
  // (the lengths stand at lens + 32: the code-length code's own nineteen were read through `lit` until here)
  for (uint32_t k = 0; k < total; ++k) lens[k] = lens[32 + k];
  return inf_codes(s, lit, dist, lens, nlen, ndist);
}

FQG_INF_HD bool inf_fixed_header(InfState& s, InfCode& lit, InfCode& dist, uint8_t* lens) {
  for (uint32_t k = 0; k < 288; ++k) lens[k] = k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : 8;
  for (uint32_t k = 0; k < 32; ++k) lens[288 + k] = 5;
  return inf_codes(s, lit, dist, lens, 288, 32);
}

// One lane's walk until something needs the others (s.wait says what).  lens: 352 bytes of scratch that hold the code
// lengths from kInfWaitTables until the tables are filled; q[qcap]: the queue, s.ntok entries of it are filled.
FQG_INF_HD void inf_round(InfState& s, InfCode& lit, InfCode& dist, uint8_t* lens, uint64_t* q, uint32_t qcap) {
  s.ntok = 0;
  if (s.wait == kInfWaitDone) return;
  s.wait = kInfWaitNone;
  for (;;) {
    if (inf_starved(s)) {
      s.wait = kInfWaitInput;
      return;
    }
    if (!s.in_block) {
      if (s.last) {  // the final block is over
        if (s.out != s.isize) return inf_refuse(s, kInfBadSize);
        s.wait = kInfWaitDone;
        return;
      }
      inf_refill(s);
      s.last = inf_bits(s, 1);
      const uint32_t type = inf_bits(s, 2);
      if (inf_overrun(s)) return inf_refuse(s, kInfBadInput);
      if (type == 3) return inf_refuse(s, kInfBadType);
      if (type == 0) {
        inf_bits(s, s.nbits & 7u);  // to the byte boundary
        inf_refill(s);
        const uint32_t len = inf_bits(s, 16), nlen = inf_bits(s, 16);
        if (inf_overrun(s)) return inf_refuse(s, kInfBadInput);
        if (len != (nlen ^ 0xFFFFu)) return inf_refuse(s, kInfBadStored);
        const uint32_t from = inf_byte_pos(s);  // (<= end: no overrun)
        if (len) {
          if (len > s.end - from) return inf_refuse(s, kInfBadInput);
          if (len > s.isize - s.out) return inf_refuse(s, kInfBadSize);
          q[s.ntok++] = inf_tok(kInfTokStored, s.out, len, from);
          s.out += len;
        }
        s.pos = from + len;
        s.nbits = 0;
        s.hold = 0;
        if (s.ntok == qcap) {
          s.wait = kInfWaitDrain;
          return;
        }
        continue;
      }
      if (!(type == 1 ? inf_fixed_header(s, lit, dist, lens) : inf_dynamic_header(s, lit, dist, lens))) return;
      s.in_block = 1;
      s.wait = kInfWaitTables;
      return;
    }
    inf_refill(s);
    const int sym = inf_decode(s, lit);
    if (sym < 0) return inf_refuse(s, inf_overrun(s) ? kInfBadInput : kInfBadCode);
    if (sym < 256) {
      if (inf_overrun(s)) return inf_refuse(s, kInfBadInput);
      if (s.out >= s.isize) return inf_refuse(s, kInfBadSize);
      s.win[s.out++] = (uint8_t)sym;
      continue;
    }
    if (sym == 256) {
      if (inf_overrun(s)) return inf_refuse(s, kInfBadInput);
      s.in_block = 0;
      continue;
    }
    if (sym > 285) return inf_refuse(s, inf_overrun(s) ? kInfBadInput : kInfBadCode);
    const uint32_t lk = (uint32_t)sym - 257;
    const uint32_t len = inf_len_base(lk) + inf_bits(s, inf_len_extra(lk));
    inf_refill(s);
    const int ds = inf_decode(s, dist);
    if (ds < 0 || ds > 29) return inf_refuse(s, inf_overrun(s) ? kInfBadInput : kInfBadCode);
    const uint32_t d = inf_dist_base((uint32_t)ds) + inf_bits(s, inf_dist_extra((uint32_t)ds));
    if (inf_overrun(s)) return inf_refuse(s, kInfBadInput);
    if (d > s.out) return inf_refuse(s, kInfBadDistance);
    if (len > s.isize - s.out) return inf_refuse(s, kInfBadSize);
    q[s.ntok++] = inf_tok(kInfTokMatch, s.out, len, d);
    s.out += len;
    if (s.ntok == qcap) {
      s.wait = kInfWaitDrain;
      return;
    }
  }
}

}  // namespace inf
}  // namespace fqg
