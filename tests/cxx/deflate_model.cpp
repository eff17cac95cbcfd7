// deflate_model.cpp - a sequential restatement of k_deflate_members (fastq_utils_amd/csrc/fqg_deflate_kernels.hip): the
// same cuts, the same hash and steps of 256 positions (candidates are read before any position of the step is
// inserted; the newest position keeps a slot), the same two candidates, the same rule for short matches, the same greedy
// parse, the codes of fqg_deflate_codes.h and the same stored fallback - one byte loop, no workgroup.  The bytes it writes
// are the bytes the device must write: tests/test_gpu_deflate.py compares them, tests/test_deflate_codes.py inflates them
// with zlib on the CPU.   deflate_model <text file> <gzip file> [--records] [--report <file>]
//
// --records: both files are runs of records, a little-endian uint32 length and that many bytes - one text per record in,
// its members per record out: a few thousand texts in one process (tests/deflgen.py).  --report adds one JSON line per
// member on what was decided (Report, below); it is filled beside the decisions and feeds none of them.
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fastq_utils_amd/csrc/fqg_deflate_codes.h"

using namespace fqg::dfl;

static const uint32_t kMember = 65280, kStep = 256, kHashBits = 14, kWindow = 32768;

struct Bits {
  std::vector<uint8_t> v;
  uint64_t n = 0;
  void put(uint64_t x, uint32_t k) {
    for (uint32_t i = 0; i < k; ++i, ++n) {
      if ((n >> 3) >= v.size()) v.push_back(0);
      v[n >> 3] |= (uint8_t)(((x >> i) & 1u) << (n & 7));
    }
  }
};

// A member's report line.  three_word: the tokens with (bit offset & 31) + width > 64, for which the kernel's gz_or_bits
// writes a third word; the offset counts from the start of the member, so the deflate block begins at bit 80 under the
// gzip frame and at bit 144 under BGZF's.  ntok counts the end-of-block, as the kernel's does.
struct Report {
  uint32_t n = 0, ntok = 0, matches = 0, max_ll = 0, max_dl = 0, widest = 0, three_word[2] = {0, 0}, header_bits = 0;
  uint64_t dyn_bytes = 0, stored_bytes = 0;
  bool dynamic = false;
  std::vector<uint32_t> taken;  // (position, length, distance) of every match of the parse
  std::vector<uint64_t> taken_at;  // (first bit in the deflate block, width) of the same matches
  uint8_t ll[kMaxSyms] = {0}, dl[32] = {0};  // the two codes' lengths
  void token(uint64_t at, uint64_t end, bool match) {  // bits [at, end) of the deflate block
    const uint32_t width = (uint32_t)(end - at);
    if (match) taken_at.insert(taken_at.end(), {at, width});
    widest = std::max(widest, width);
    three_word[0] += ((80 + at) & 31) + width > 64;
    three_word[1] += ((144 + at) & 31) + width > 64;
  }
  void print(FILE* f, size_t text, size_t member) const {
    fprintf(f, "{\"text\": %zu, \"member\": %zu, \"n\": %u, \"ntok\": %u, \"matches\": %u, \"max_ll\": %u, \"max_dl\": %u, \"widest\": %u, "
               "\"three_word_gzip\": %u, \"three_word_bgzf\": %u, \"header_bits\": %u, \"dyn_bytes\": %llu, \"stored_bytes\": %llu, "
               "\"written\": \"%s\", \"taken\": [",
            text, member, n, ntok, matches, max_ll, max_dl, widest, three_word[0], three_word[1], header_bits,
            (unsigned long long)dyn_bytes, (unsigned long long)stored_bytes, dynamic ? "dynamic" : "stored");
    for (size_t k = 0; k < taken.size(); k += 3) fprintf(f, "%s[%u, %u, %u]", k ? ", " : "", taken[k], taken[k + 1], taken[k + 2]);
    fprintf(f, "], \"taken_at\": [");
    for (size_t k = 0; k < taken_at.size(); k += 2) fprintf(f, "%s[%llu, %llu]", k ? ", " : "", (unsigned long long)taken_at[k], (unsigned long long)taken_at[k + 1]);
    fprintf(f, "], \"lit_len\": [");
    for (uint32_t s = 0; s < kLitSyms; ++s) fprintf(f, "%s%u", s ? ", " : "", ll[s]);
    fprintf(f, "], \"dist_len\": [");
    for (uint32_t s = 0; s < kDistSyms; ++s) fprintf(f, "%s%u", s ? ", " : "", dl[s]);
    fprintf(f, "]}\n");
  }
};

static uint32_t ld32(const uint8_t* t, size_t a) {
  uint32_t w;
  memcpy(&w, t + a, 4);
  return w;
}
static uint32_t hash_of(uint32_t w) { return (w * 0x9E3779B1u) >> (32 - kHashBits); }
static uint32_t extend(const uint8_t* t, uint32_t c, uint32_t p, uint32_t maxlen) {
  uint32_t len = 4;
  while (len < maxlen && t[c + len] == t[p + len]) ++len;
  return len;
}

static void member(const uint8_t* text, uint32_t n, std::vector<uint8_t>& out, Report* rep) {
  std::vector<uint8_t> padded(text, text + n);
  padded.resize(n + 8, 0);
  const uint8_t* t = padded.data();
  std::vector<uint32_t> hash(1u << kHashBits, 0), toks;
  uint32_t lf[kMaxSyms] = {0}, df[32] = {0}, next = 0;
  for (uint32_t base = 0; base < n; base += kStep) {
    uint32_t cand[kStep] = {0}, found[kStep] = {0};
    for (uint32_t k = 0; k < kStep; ++k)
      if (base + k + 4 <= n) cand[k] = hash[hash_of(ld32(t, base + k))];
    for (uint32_t k = 0; k < kStep; ++k)
      if (base + k + 4 <= n) {
        uint32_t& h = hash[hash_of(ld32(t, base + k))];
        h = std::max(h, base + k + 1);
      }
    for (uint32_t k = 0; k < kStep; ++k) {
      const uint32_t p = base + k;
      if (p + 4 > n || p < next) continue;  // (`next` as it stood when the step began)
      const uint32_t w4 = ld32(t, p), maxlen = std::min(258u, n - p);
      uint32_t len = 0, dist = 0;
      if (cand[k] && p + 1 - cand[k] <= kWindow && ld32(t, cand[k] - 1) == w4) {
        len = extend(t, cand[k] - 1, p, maxlen);
        dist = p + 1 - cand[k];
      }
      if (p && dist != 1 && len < maxlen && ld32(t, p - 1) == w4) {
        const uint32_t l1 = extend(t, p - 1, p, maxlen);
        if (l1 >= len) len = l1, dist = 1;
      }
      if (len >= 6 || (len == 5 && dist <= 4096) || (len == 4 && dist <= 512)) found[k] = len | ((dist - 1) << 9);
    }
    for (uint32_t k = 0; k < kStep && base + k < n; ++k) {
      const uint32_t p = base + k;
      if (p < next) continue;
      if (found[k]) {
        toks.push_back(0x80000000u | found[k]);
        next = p + (found[k] & 0x1FFu);
        ++lf[257 + dc_len_sym(found[k] & 0x1FFu)];
        ++df[dc_dist_sym(((found[k] >> 9) & 0x7FFFu) + 1)];
        if (rep) rep->taken.insert(rep->taken.end(), {p, found[k] & 0x1FFu, ((found[k] >> 9) & 0x7FFFu) + 1});
      } else {
        toks.push_back(t[p]);
        ++lf[t[p]];
        next = p + 1;
      }
    }
  }
  lf[256] = 1;
  static CodeWork W;
  static DynHeader H;
  uint8_t ll[kMaxSyms], dl[32];
  uint16_t lc[kMaxSyms], dc[32];
  dc_code_lengths(lf, kLitSyms, 15, ll, W);
  dc_canonical_codes(ll, kLitSyms, lc);
  dc_code_lengths(df, kDistSyms, 15, dl, W);
  dc_canonical_codes(dl, kDistSyms, dc);
  dc_build_header(ll, dl, H, W);
  Bits b;
  dc_put_header(H, true, [&](uint32_t v, uint32_t k) { b.put(v, k); });
  for (uint32_t tok : toks) {
    const uint64_t at = b.n;
    if (!(tok & 0x80000000u)) {
      b.put(lc[tok], ll[tok]);
    } else {
      const uint32_t len = tok & 0x1FFu, dist = ((tok >> 9) & 0x7FFFu) + 1, ls = dc_len_sym(len), ds = dc_dist_sym(dist);
      b.put(lc[257 + ls], ll[257 + ls]);
      b.put(len - dc_len_base(ls), dc_len_extra(ls));
      b.put(dc[ds], dl[ds]);
      b.put(dist - dc_dist_base(ds), dc_dist_extra(ds));
    }
    if (rep) rep->token(at, b.n, (tok & 0x80000000u) != 0);
  }
  const uint64_t eob_at = b.n;
  b.put(lc[256], ll[256]);
  const uint8_t hdr[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 3};
  out.insert(out.end(), hdr, hdr + 10);
  if (b.v.size() <= 5 + (size_t)n) {
    out.insert(out.end(), b.v.begin(), b.v.end());
  } else {
    const uint8_t s[5] = {1, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)(~n >> 8)};
    out.insert(out.end(), s, s + 5);
    out.insert(out.end(), text, text + n);
  }
  const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), text, n);
  for (int k = 0; k < 4; ++k) out.push_back((uint8_t)(crc >> (8 * k)));
  for (int k = 0; k < 4; ++k) out.push_back((uint8_t)(n >> (8 * k)));
  if (rep) {
    rep->token(eob_at, b.n, false);
    memcpy(rep->ll, ll, kLitSyms);
    memcpy(rep->dl, dl, kDistSyms);
    rep->n = n;
    rep->ntok = (uint32_t)toks.size() + 1;
    rep->matches = (uint32_t)(rep->taken.size() / 3);
    for (uint32_t s = 0; s < kLitSyms; ++s) rep->max_ll = std::max<uint32_t>(rep->max_ll, ll[s]);
    for (uint32_t s = 0; s < kDistSyms; ++s) rep->max_dl = std::max<uint32_t>(rep->max_dl, dl[s]);
    rep->header_bits = H.bits;
    rep->dyn_bytes = b.v.size();
    rep->stored_bytes = 5 + (uint64_t)n;
    rep->dynamic = b.v.size() <= 5 + (size_t)n;
  }
}

static bool read_all(const char* path, std::vector<uint8_t>& d) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + k);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  bool records = false;
  const char* report_path = nullptr;
  for (int a = 3; a < argc; ++a) {
    if (!strcmp(argv[a], "--records")) records = true;
    else if (!strcmp(argv[a], "--report") && a + 1 < argc) report_path = argv[++a];
    else return 2;
  }
  std::vector<uint8_t> d, out;
  if (!read_all(argv[1], d)) return 2;
  d.resize(d.size() + 4);  // (member() reads a text by its length alone; a record's length field may be read at the end)
  const size_t size = d.size() - 4;
  FILE* rf = report_path ? fopen(report_path, "w") : nullptr;
  if (report_path && !rf) return 2;
  size_t texts = 0;
  for (size_t at = 0; records ? at < size : !texts; ++texts) {
    size_t len = size;
    if (records) {
      if (size - at < 4) return 2;
      len = ld32(d.data(), at);
      at += 4;
      if (size - at < len) return 2;
    }
    const size_t mark = out.size();
    if (records) out.resize(mark + 4);
    for (size_t o = 0, m = 0; o < std::max<size_t>(len, 1); o += kMember, ++m) {
      Report rep;
      member(d.data() + at + o, (uint32_t)std::min<size_t>(kMember, len - o), out, rf ? &rep : nullptr);
      if (rf) rep.print(rf, texts, m);
    }
    if (records) {
      const uint32_t bytes = (uint32_t)(out.size() - mark - 4);
      memcpy(out.data() + mark, &bytes, 4);
    }
    at += len;
  }
  if (rf && fclose(rf) != 0) return 2;
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), 1, out.size(), g) != out.size() || fclose(g) != 0) return 2;
  printf("in=%zu out=%zu\n", size, out.size());
  return 0;
}
