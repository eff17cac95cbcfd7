// deflate_codes_check.cpp - fastq_utils_amd/csrc/fqg_deflate_codes.h on the CPU (tests/test_deflate_codes.py): on many
// tables of counts the code lengths respect their limit and form a complete code, at least two symbols have a code, the
// canonical codes are prefix-free, the run-length coded header decodes - through the small decoder below, written from
// RFC 1951 3.2.7 alone - back to the same lengths, and the length / distance symbol arithmetic agrees with the RFC's tables.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../fastq_utils_amd/csrc/fqg_deflate_codes.h"

using namespace fqg::dfl;

static int failures = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      if (++failures < 20) {                \
        fprintf(stderr, "FAIL %s: ", #cond); \
        fprintf(stderr, __VA_ARGS__);       \
        fprintf(stderr, "\n");              \
      }                                     \
    }                                       \
  } while (0)

struct Bits {
  std::vector<uint8_t> v;
  uint64_t n = 0;
  void put(uint32_t x, uint32_t k) {
    for (uint32_t i = 0; i < k; ++i, ++n) {
      if ((n >> 3) >= v.size()) v.push_back(0);
      v[n >> 3] |= (uint8_t)(((x >> i) & 1u) << (n & 7));
    }
  }
  uint64_t at = 0;
  uint32_t get(uint32_t k) {
    uint32_t x = 0;
    for (uint32_t i = 0; i < k; ++i, ++at) x |= (uint32_t)((v[at >> 3] >> (at & 7)) & 1u) << i;
    return x;
  }
};

// a symbol of the Huffman code (lens) whose codes are read MSB first from an LSB-first bit stream
static int decode_symbol(Bits& b, const uint8_t* lens, unsigned n) {
  unsigned count[16] = {0}, first[16] = {0};
  for (unsigned s = 0; s < n; ++s) ++count[lens[s]];
  count[0] = 0;
  unsigned code = 0;
  for (unsigned l = 1; l <= 15; ++l) {
    code = (code + count[l - 1]) << 1;
    first[l] = code;
  }
  unsigned c = 0;
  for (unsigned l = 1; l <= 15; ++l) {
    c = (c << 1) | b.get(1);
    if (count[l] && c >= first[l] && c < first[l] + count[l]) {
      unsigned k = c - first[l];
      for (unsigned s = 0; s < n; ++s)
        if (lens[s] == l && k-- == 0) return (int)s;
    }
  }
  return -1;
}

static void check_code(const char* what, const uint8_t* lens, unsigned n, unsigned maxbits, const uint32_t* freq) {
  unsigned used_in = 0, coded = 0;
  uint64_t kraft = 0;
  for (unsigned s = 0; s < n; ++s) {
    used_in += freq[s] != 0;
    CHECK(lens[s] <= maxbits, "%s: symbol %u has %u bits", what, s, lens[s]);
    if (freq[s]) CHECK(lens[s] != 0, "%s: used symbol %u has no code", what, s);
    if (lens[s]) {
      ++coded;
      kraft += 1ull << (15 - lens[s]);
    }
  }
  CHECK(coded >= 2, "%s: %u codes", what, coded);
  if (used_in >= 2) {
    CHECK(coded == used_in, "%s: %u codes for %u symbols", what, coded, used_in);
    CHECK(kraft == 1ull << 15, "%s: Kraft sum %llu / 32768", what, (unsigned long long)kraft);
  } else {
    CHECK(kraft <= 1ull << 15, "%s: Kraft sum %llu / 32768", what, (unsigned long long)kraft);
  }
  // canonical codes: reversed back they are the RFC's numbering, so distinct symbols of one length differ
  uint16_t codes[kMaxSyms];
  dc_canonical_codes(lens, n, codes);
  for (unsigned s = 0; s < n; ++s)
    for (unsigned t = s + 1; t < n; ++t)
      if (lens[s] && lens[s] == lens[t]) CHECK(codes[s] != codes[t], "%s: symbols %u and %u share a code", what, s, t);
}

static uint64_t tables = 0, header_bits = 0, limited15 = 0, limited7 = 0;

// a literal/length table and a distance table: both codes, the header, and the header read back
static void check_tables(const char* what, const uint32_t* lf, const uint32_t* df) {
  static CodeWork W;
  uint8_t ll[kMaxSyms], dl[32];
  dc_code_lengths(lf, kLitSyms, 15, ll, W);
  dc_code_lengths(df, kDistSyms, 15, dl, W);
  check_code(what, ll, kLitSyms, 15, lf);
  check_code(what, dl, kDistSyms, 15, df);
  for (unsigned s = 0; s < kLitSyms; ++s) limited15 += ll[s] == 15;
  static DynHeader H;
  dc_build_header(ll, dl, H, W);
  uint32_t cf[kClSyms] = {0};
  for (unsigned k = 0; k < H.ncl; ++k) ++cf[H.sym[k]];
  check_code(what, H.cll, kClSyms, 7, cf);
  for (unsigned s = 0; s < kClSyms; ++s) limited7 += H.cll[s] == 7;
  Bits b;
  dc_put_header(H, true, [&](uint32_t v, uint32_t n) { b.put(v, n); });
  CHECK(b.n == H.bits, "%s: header of %llu bits, %u announced", what, (unsigned long long)b.n, H.bits);
  header_bits += b.n;
  b.put(0, 32);  // (room for a decoder that has lost its way)
  b.put(0, 32);
  // RFC 1951 3.2.7
  CHECK(b.get(1) == 1 && b.get(2) == 2, "%s: block type", what);
  const unsigned hlit = b.get(5) + 257, hdist = b.get(5) + 1, hclen = b.get(4) + 4;
  CHECK(hlit <= 286 && hdist <= 30, "%s: hlit %u hdist %u", what, hlit, hdist);
  static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint8_t cll[19] = {0};
  for (unsigned k = 0; k < hclen; ++k) cll[order[k]] = (uint8_t)b.get(3);
  std::vector<uint8_t> seq;
  bool ok = true;
  while (seq.size() < hlit + hdist && ok) {
    const int s = decode_symbol(b, cll, 19);
    if (s < 0) ok = false;
    else if (s < 16) seq.push_back((uint8_t)s);
    else if (s == 16) {
      if (seq.empty()) ok = false;
      else seq.insert(seq.end(), 3 + b.get(2), seq.back());
    } else if (s == 17) seq.insert(seq.end(), 3 + b.get(3), 0);
    else seq.insert(seq.end(), 11 + b.get(7), 0);
  }
  CHECK(ok && seq.size() == hlit + hdist, "%s: the header decodes to %zu lengths of %u", what, seq.size(), hlit + hdist);
  CHECK(b.at == H.bits, "%s: the decoder read %llu bits of %u", what, (unsigned long long)b.at, H.bits);
  if (ok && seq.size() == hlit + hdist) {
    for (unsigned s = 0; s < kLitSyms; ++s) CHECK((s < hlit ? seq[s] : 0) == ll[s], "%s: literal length %u", what, s);
    for (unsigned s = 0; s < kDistSyms; ++s) CHECK((s < hdist ? seq[hlit + s] : 0) == dl[s], "%s: distance length %u", what, s);
  }
  ++tables;
}

int main() {
  uint32_t lf[kMaxSyms], df[32];
  auto clear = [&] {
    memset(lf, 0, sizeof(lf));
    memset(df, 0, sizeof(df));
  };
  // all zero but one symbol (and nothing at all)
  clear();
  check_tables("nothing", lf, df);
  lf[256] = 1;
  check_tables("end of block alone", lf, df);
  lf[256] = 0, lf[0] = 77;
  check_tables("symbol 0 alone", lf, df);
  lf[0] = 0, lf[285] = 5, df[29] = 5;
  check_tables("last symbols alone", lf, df);
  // two symbols
  clear();
  lf[65] = 1000, lf[256] = 1, df[0] = 1, df[29] = 1u << 30;
  check_tables("two symbols", lf, df);
  // 286 equal
  for (unsigned s = 0; s < kLitSyms; ++s) lf[s] = 7;
  for (unsigned s = 0; s < kDistSyms; ++s) df[s] = 7;
  check_tables("all equal", lf, df);
  // Fibonacci weights: the natural depths exceed 15 bits, and the lengths 1..15 all occur, so that the code-length code
  // gets Fibonacci-like counts of its own and meets its 7 bits
  clear();
  {
    uint32_t a = 1, b = 1;
    for (unsigned s = 0; s < 40; ++s) {
      lf[s * 7 % kLitSyms] = a;
      const uint32_t c = a + b;
      a = b, b = c;
    }
    a = 1, b = 1;
    for (unsigned s = 0; s < kDistSyms; ++s) {
      df[s] = a;
      const uint32_t c = a + b;
      a = b, b = c;
    }
  }
  const uint64_t l15 = limited15;
  check_tables("fibonacci", lf, df);
  CHECK(limited15 > l15, "the Fibonacci table did not reach 15 bits");
  // a header whose code-length symbols have Fibonacci counts: lengths k repeated fib(k) times, no two neighbours equal
  {
    static CodeWork W;
    uint32_t cf[kClSyms];
    uint32_t a = 1, b = 1;
    for (unsigned s = 0; s < kClSyms; ++s) {
      cf[s] = a;
      const uint32_t c = a + b;
      a = b, b = c;
    }
    uint8_t cl[kClSyms];
    dc_code_lengths(cf, kClSyms, 7, cl, W);
    check_code("fibonacci code-length code", cl, kClSyms, 7, cf);
    unsigned deepest = 0;
    for (unsigned s = 0; s < kClSyms; ++s) deepest = cl[s] > deepest ? cl[s] : deepest;
    CHECK(deepest == 7, "the Fibonacci code-length table reached %u bits", deepest);
  }
  // random tables of every shape
  std::mt19937_64 rng(20240611);
  for (unsigned t = 0; t < 2000; ++t) {
    clear();
    const unsigned shape = t % 5;
    const unsigned nl = 1 + (unsigned)(rng() % kLitSyms), nd = (unsigned)(rng() % (kDistSyms + 1));
    for (unsigned k = 0; k < nl; ++k) {
      const unsigned s = (unsigned)(rng() % kLitSyms);
      uint32_t f;
      if (shape == 0) f = 1 + (uint32_t)(rng() % 4);
      else if (shape == 1) f = 1 + (uint32_t)(rng() % 65280);
      else if (shape == 2) f = 1u << (rng() % 17);
      else if (shape == 3) f = (uint32_t)(1.0 + 60000.0 * std::generate_canonical<double, 30>(rng) * std::generate_canonical<double, 30>(rng) * std::generate_canonical<double, 30>(rng));
      else f = (uint32_t)(rng() % 3);
      lf[s] = f;
    }
    for (unsigned k = 0; k < nd; ++k) df[rng() % kDistSyms] = shape == 2 ? 1u << (rng() % 17) : 1 + (uint32_t)(rng() % 3000);
    if (shape != 4) lf[256] = 1;
    check_tables("random", lf, df);
  }
  // the symbol arithmetic against the RFC's tables (3.2.5)
  static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  static const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  static const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  unsigned symbols = 0;
  for (unsigned len = 3; len <= 258; ++len) {
    unsigned want = 28;
    if (len < 258)
      for (want = 0; !(len >= lbase[want] && len < lbase[want] + (1u << lext[want])); ++want) {}
    const unsigned s = dc_len_sym(len);
    CHECK(s == want && dc_len_extra(s) == lext[s] && dc_len_base(s) == lbase[s], "length %u -> symbol %u", len, s);
    ++symbols;
  }
  for (unsigned d = 1; d <= 32768; ++d) {
    unsigned want = 0;
    for (; !(d >= dbase[want] && d < dbase[want] + (1u << dext[want])); ++want) {}
    const unsigned s = dc_dist_sym(d);
    CHECK(s == want && dc_dist_extra(s) == dext[s] && dc_dist_base(s) == dbase[s], "distance %u -> symbol %u", d, s);
    ++symbols;
  }
  printf("tables=%llu header_bits=%llu limited15=%llu limited7=%llu symbols=%u failures=%d\n", (unsigned long long)tables,
         (unsigned long long)header_bits, (unsigned long long)limited15, (unsigned long long)limited7, symbols, failures);
  return failures ? 1 : 0;
}
