// fqg_name_capture.h - pass 1 of the streaming framing: the header lines that begin in a chunk, captured while the chunk
// is in LDS (NameCapture, fqg_device.h) - as 16-byte digests (capture_digests) or as 64-byte records (capture_records).
// Included by fqg_stream_kernels.hip behind what it builds on: dpp0, eq_bytes (fqg_kernels.hip), pack_marks16, ChunkLane,
// Speculation, NlRanks and the geometry of the LDS copy.
//
// Both read what the steps in front of them left: the staged entries in the wave's LDS table (slots[i] & 0xFFF = offset of
// the chunk's i-th newline), the copy of the chunk (with its slack in front and behind), the speculated type t0 of the
// chunk's first byte.  The line that starts at v (v = 0: the chunk's first byte, else behind the chunk's v-th newline) has
// type t0 + v.  Neither uses the type masks of the class tests.
#pragma once

namespace fqg {

// minimum over the four lanes of a quad, in every lane of it
__device__ __forceinline__ uint32_t quad_min(uint32_t x) {
  uint32_t o = dpp0<0xB1, 0xf, 0xf>(x);  // quad_perm [1,0,3,2]
  x = o < x ? o : x;
  o = dpp0<0x4E, 0xf, 0xf>(x);           // quad_perm [2,3,0,1]
  return o < x ? o : x;
}
// sum over the four lanes of a quad, in every lane of it
__device__ __forceinline__ uint64_t quad_sum(uint64_t part) {
  uint32_t plo = (uint32_t)part, phi = (uint32_t)(part >> 32);
  uint64_t oth = ((uint64_t)dpp0<0xB1, 0xf, 0xf>(phi) << 32) | dpp0<0xB1, 0xf, 0xf>(plo);
  part += oth;
  plo = (uint32_t)part;
  phi = (uint32_t)(part >> 32);
  oth = ((uint64_t)dpp0<0x4E, 0xf, 0xf>(phi) << 32) | dpp0<0x4E, 0xf, 0xf>(plo);
  return part + oth;
}
// where among the 64 bytes a quad looks at (lane `sub` holds bytes [16 sub, 16 sub + 16) in x) the first byte of the
// pattern `pat` stands; ~0 when there is none
__device__ __forceinline__ uint32_t quad_first_byte(const uint4& x, uint32_t pat, uint32_t sub) {
  const uint32_t m = pack_marks16(eq_bytes(x.x, pat), eq_bytes(x.y, pat), eq_bytes(x.z, pat), eq_bytes(x.w, pat));
  return quad_min(m ? 16u * sub + (uint32_t)__builtin_ctz(m) : ~0u);
}

// ---- header lines that begin in this chunk -> 16-byte digests: canonical name + hash, four lanes per header ----
// Headers are every fourth line start from v0 on, so quad q of the wavefront takes the header at v0 + 4 q without a
// compaction.  Lane `sub` of a quad looks at name bytes [16 sub, 16 sub + 16) - the bytes behind the '@'.
// prev: the byte in front of the chunk
__device__ __forceinline__ void capture_digests(const uint8_t* img, uint64_t n, const ChunkLane& c,
                                                const NameCapture& nc, const uint16_t* slots, bool first_is_start,
                                                Speculation sp, NlRanks r) {
  const uint8_t* const copy = c.copy;
  const uint32_t tot = r.staged;
  uint32_t hc = kNoCapture;
  if (sp.found && r.total <= (uint32_t)kStageCap) {
    hc = 0;
    uint32_t v0 = (0u - sp.t0) & 3u;
    if (v0 == 0u && !first_is_start) v0 = 4u;
    const uint32_t sub = (uint32_t)c.lane & 3u, q = (uint32_t)c.lane >> 2;
    const bool casava = nc.fmt == FQG_NAME_CASAVA18;
    const uint32_t pe_cut = (nc.fmt == FQG_NAME_DEFAULT && nc.is_pe) ? 1u : 0u;
    for (uint32_t base = 0; v0 + 4u * base <= tot; base += kWave / 4) {
      const uint32_t j = base + q, vv = v0 + 4u * j;
      bool is_hdr = vv <= tot;
      uint32_t at = 0;
      if (is_hdr && vv > 0) {
        at = (slots[vv - 1] & 0xFFFu) + 1u;
        is_hdr = at < (uint32_t)kChunkBytes;
      }
      hc += (uint32_t)__builtin_popcountll(__ballot(is_hdr && sub == 0u));
      if (is_hdr && j < nc.K) {
        const bool end_known = vv < tot;
        uint32_t lnm = end_known ? (uint32_t)(slots[vv] & 0xFFFu) - at - 1u : ~0u;  // name bytes in front of the '\n'
        const bool at_sign = copy[at] == '@';
        bool ok = true;
        uint4 x;
        if (end_known) {
          __builtin_memcpy(&x, copy + at + 1u + 16u * sub, 16);
        } else if (c.cb + at + 1u + kDigestText <= n) {
          // the line runs into the next chunk (one header in eight at 150 bp): its bytes from the image - the
          // wavefront next door is loading them anyway - and its length from the '\n' among them, if there is one
          __builtin_memcpy(&x, img + c.cb + at + 1u + 16u * sub, 16);
          lnm = quad_first_byte(x, 0x0A0A0A0Au, sub);
        } else {
          x = make_uint4(0, 0, 0, 0);
          ok = false;
        }
        uint32_t nlen = 0, acct = 0;
        if (casava) {
          // the name ends at the first blank of the line (src/fastq.c:496-503); "/1" in front of it is dropped
          const uint32_t blank = quad_first_byte(x, 0x20202020u, sub);
          if (blank >= lnm || blank >= kDigestText) ok = false;  // no blank in the line (or none in what the quad sees of it)
          // the byte two places in front of the blank: with the lane that holds it
          const uint32_t two = blank - 2u;
          uint32_t slash = 0;
          if (ok && blank >= 2u && (two >> 4) == sub) {
            const uint32_t wsel = (two >> 2) & 3u;
            const uint32_t wd = wsel == 0u ? x.x : wsel == 1u ? x.y : wsel == 2u ? x.z : x.w;
            slash = ((wd >> (8u * (two & 3u))) & 0xFFu) == '/' ? 1u : 0u;
          }
          slash |= dpp0<0xB1, 0xf, 0xf>(slash);
          slash |= dpp0<0x4E, 0xf, 0xf>(slash);
          nlen = acct = ok ? blank - 2u * slash : 0u;
        } else {
          // strlen(&hdr[1]) counts the '\n' (src/fastq.c:505-511); a line whose end nobody saw, or one so short that
          // the name would hold the '\n', is left to the byte-wise path
          const uint32_t L = lnm + 1u;
          if (lnm == ~0u || L < 1u + pe_cut) ok = false;
          const uint32_t l = L - pe_cut;
          acct = l;
          nlen = l - 1u;
          if (nlen > kDigestText) ok = false;
        }
        if (nlen > 1023u || acct > 1023u) ok = false;
        if (!ok) nlen = acct = 0;
        // the hash: this lane's two words, bytes behind the name zeroed, summed over the quad
        const uint32_t lo = 16u * sub;
        const uint32_t k0 = nlen > lo ? nlen - lo : 0u;             // name bytes in this lane's first word and beyond
        const uint32_t k1 = nlen > lo + 8u ? nlen - lo - 8u : 0u;   // ... in its second word and beyond
        uint64_t w0 = ((uint64_t)x.y << 32) | x.x, w1 = ((uint64_t)x.w << 32) | x.z;
        w0 = k0 >= 8u ? w0 : (w0 & ((1ull << (8u * k0)) - 1ull));
        w1 = k1 >= 8u ? w1 : (w1 & ((1ull << (8u * k1)) - 1ull));
        // (the keys by selection: sub is one of four; a word counts when it holds a name byte - name_word)
        const uint32_t a0 = sub == 0u ? name_key_a(0) : sub == 1u ? name_key_a(2) : sub == 2u ? name_key_a(4) : name_key_a(6);
        const uint32_t b0 = sub == 0u ? name_key_b(0) : sub == 1u ? name_key_b(2) : sub == 2u ? name_key_b(4) : name_key_b(6);
        const uint32_t a1 = sub == 0u ? name_key_a(1) : sub == 1u ? name_key_a(3) : sub == 2u ? name_key_a(5) : name_key_a(7);
        const uint32_t b1 = sub == 0u ? name_key_b(1) : sub == 1u ? name_key_b(3) : sub == 2u ? name_key_b(5) : name_key_b(7);
        uint64_t part = 0;
        if (k0) part = (uint64_t)((uint32_t)w0 + a0) * (uint64_t)((uint32_t)(w0 >> 32) + b0);
        if (k1) part += (uint64_t)((uint32_t)w1 + a1) * (uint64_t)((uint32_t)(w1 >> 32) + b1);
        part = quad_sum(part);
        if (sub == 0u) {
          typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
          u64x2 dg;
          dg.x = name_fin(name_seed(nlen) + part);
          dg.y = (unsigned long long)(nlen | (acct << 10) | (vv << 20) | (at_sign ? kDigestAt : 0u) | (ok ? kDigestOk : 0u));
          *reinterpret_cast<u64x2*>(nc.recs + ((uint64_t)c.chunk * nc.K + j) * kDigestWords) = dg;
        }
      }
    }
    if (hc >= kNoCapture) hc = kNoCapture - 1u;
  }
  if (c.lane == 0) nc.hcount[c.chunk] = (uint16_t)hc;
}

// ---- header lines that begin in this chunk -> 64-byte records (NameCapture) ----
// Line starts: the chunk's first byte when the byte in front of it (prev) is a '\n' (v = 0), and the byte behind the
// chunk's v-th newline unless that newline is the chunk's last byte.  A lane per line start.
__device__ __forceinline__ void capture_records(const uint8_t* img, uint64_t n, const ChunkLane& c,
                                                const NameCapture& nc, const uint16_t* slots, bool first_is_start,
                                                Speculation sp, NlRanks r) {
  const uint8_t* const copy = c.copy;
  const uint32_t tot = r.staged;
  uint32_t hc = kNoCapture;
  if (sp.found && r.total <= (uint32_t)kStageCap) {
    hc = 0;
    for (uint32_t base = 0; base <= tot; base += kWave) {
      const uint32_t vv = base + (uint32_t)c.lane;
      bool is_hdr = vv <= tot && ((sp.t0 + vv) & 3u) == 0u && (vv > 0 || first_is_start);
      uint32_t at = 0;
      if (is_hdr && vv > 0) {
        at = (slots[vv - 1] & 0xFFFu) + 1u;
        is_hdr = at < (uint32_t)kChunkBytes;
      }
      const unsigned long long hm = __ballot(is_hdr);
      const uint32_t j = hc + (uint32_t)__builtin_popcountll(hm & ((1ull << c.lane) - 1ull));
      hc += (uint32_t)__builtin_popcountll(hm);
      if (is_hdr && j < nc.K) {
        bool end_known = vv < tot, real = false;
        uint32_t len = (end_known ? (uint32_t)(slots[vv] & 0xFFFu) : (uint32_t)kChunkBytes) - at;
        unsigned long long w[kNameRecWords];
        if (end_known || c.cb + at + kNameRecText + 1 > n) {
#pragma unroll
          for (uint32_t k = 0; k < kNameRecWords; ++k) __builtin_memcpy(&w[k], copy + at + 8u * k - 3u, 8);  // byte 3 = the line's first byte
        } else {
          // the line runs into the next chunk (one header in eight does at 150 bp): its bytes from the image - the
          // wavefront next door is loading them anyway - and its length from the '\n' among them, if there is one
          const uint8_t* g = img + c.cb + at - 3u;
          unsigned long long nlm[kNameRecWords];
#pragma unroll
          for (uint32_t k = 0; k < kNameRecWords; ++k) {
            __builtin_memcpy(&w[k], g + 8u * k, 8);
            const unsigned long long y = w[k] ^ 0x0A0A0A0A0A0A0A0Aull;
            nlm[k] = ~(((y & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | y | 0x7F7F7F7F7F7F7F7Full);
          }
          nlm[0] &= ~0xFFFFFFull;  // (the three bytes in front of the line)
          real = true;
          len = kNameRecText + 1;  // at least: no '\n' among the bytes of the record
#pragma unroll
          for (int k = (int)kNameRecWords - 1; k >= 0; --k)
            if (nlm[k]) {
              len = 8u * (uint32_t)k + ((uint32_t)__builtin_ctzll(nlm[k]) >> 3) - 3u;
              end_known = true;
            }
        }
        len = len > 1023u ? 1023u : len;
        const uint32_t meta = len | (vv << 10) | (end_known ? 1u << 19 : 0u) | (((w[0] >> 24) & 0xFFu) == '@' ? 1u << 20 : 0u) |
                              (real ? 1u << 21 : 0u);
        w[0] = (w[0] & 0xFFFFFFFF00000000ull) | meta;
        typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
        u64x2* dst = reinterpret_cast<u64x2*>(nc.recs + ((uint64_t)c.chunk * nc.K + j) * kNameRecWords);
#pragma unroll
        for (uint32_t k = 0; k < kNameRecWords / 2; ++k) {
          u64x2 x;
          x.x = w[2 * k];
          x.y = w[2 * k + 1];
          dst[k] = x;
        }
      }
    }
    if (hc >= kNoCapture) hc = kNoCapture - 1u;
  }
  if (c.lane == 0) nc.hcount[c.chunk] = (uint16_t)hc;
}

}  // namespace fqg
