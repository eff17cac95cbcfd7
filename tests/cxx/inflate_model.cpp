// inflate_model.cpp - the device inflater (fastq_utils_amd/csrc/fqg_inflate_kernels.hip) as one sequential program
// around the header the kernel compiles (fqg_inflate_core.h): the walk over the BGZF headers restated
// (host/fq_parallel.h: bgzf_inflate_parallel), the payload staged in windows as the kernel stages it, the rounds of
// inf_round with the tables filled and the queue drained in between, a plain CRC-32.  Every buffer is allocated to its
// exact size so that a sanitizer build sees any byte read or written outside it.
//
//   inflate_model IN OUT [stage_bytes]
// prints "frame refused" (status 3) or, per block, "block K status S crc C", then "blocks N out_bytes B raw_bytes R
// bad X crc Y" (-1: none), and writes the inflated stream (refused blocks: whatever was written before the refusal).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fastq_utils_amd/csrc/fqg_inflate_core.h"

using namespace fqg::inf;

struct Block {
  size_t in_at, in_len, isize, out_at;
};

static bool walk(const std::vector<uint8_t>& raw, std::vector<Block>& blocks, size_t* raw_bytes, size_t* total) {
  size_t p = 0;
  *total = 0;
  while (p + 18 <= raw.size()) {
    if (raw[p] != 0x1f || raw[p + 1] != 0x8b || raw[p + 2] != 8 || !(raw[p + 3] & 4)) return false;
    const size_t xlen = raw[p + 10] | (raw[p + 11] << 8);
    size_t q = p + 12, bsize = 0;
    bool found = false;
    while (q + 4 <= p + 12 + xlen && q + 4 <= raw.size()) {
      const size_t slen = raw[q + 2] | (raw[q + 3] << 8);
      if (raw[q] == 66 && raw[q + 1] == 67 && slen == 2 && q + 6 <= raw.size()) {
        bsize = (raw[q + 4] | (raw[q + 5] << 8)) + 1;
        found = true;
      }
      q += 4 + slen;
    }
    if (!found || p + bsize > raw.size() || bsize < 12 + xlen + 8) return false;
    const uint8_t* z = &raw[p + bsize - 4];
    const size_t isize = (size_t)z[0] | ((size_t)z[1] << 8) | ((size_t)z[2] << 16) | ((size_t)z[3] << 24);
    if (isize > kInfMaxIsize) return false;
    blocks.push_back({p + 12 + xlen, bsize - 12 - xlen - 8, isize, *total});
    *total += isize;
    p += bsize;
  }
  *raw_bytes = p;
  return true;
}

static uint32_t crc32_plain(const uint8_t* p, size_t n) {
  uint32_t r = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    r ^= p[i];
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (r & 1u ? 0xEDB88320u : 0u);
  }
  return ~r;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const uint32_t stage = argc > 3 ? (uint32_t)atoi(argv[3]) : 4096u;
  if (stage < 2 * kInfMargin) return 2;
  std::vector<uint8_t> raw;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) raw.insert(raw.end(), buf, buf + k);
    fclose(f);
  }
  std::vector<Block> blocks;
  size_t raw_bytes = 0, total = 0;
  if (!walk(raw, blocks, &raw_bytes, &total)) {
    printf("frame refused\n");
    return 3;
  }
  std::vector<uint8_t> out(total);
  long bad = -1, crc_bad = -1;
  constexpr uint32_t kQ = 64;
  InfCode* lit = new InfCode;
  InfCode* dist = new InfCode;
  uint8_t* lens = new uint8_t[352];
  uint64_t* q = new uint64_t[kQ];
  for (size_t bi = 0; bi < blocks.size(); ++bi) {
    const Block& b = blocks[bi];
    if (b.isize == 0) {
      printf("block %zu status 0 crc 1\n", bi);
      continue;
    }
    const uint8_t* pay = raw.data() + b.in_at;
    uint8_t* win = (uint8_t*)malloc(b.isize);  // exactly ISIZE bytes of room
    uint8_t* staged = nullptr;
    InfState s;
    inf_begin(s, (uint32_t)b.in_len, (uint32_t)b.isize, win);
    while (s.wait != kInfWaitDone) {
      if (s.wait == kInfWaitInput) {
        free(staged);
        const uint32_t from = inf_byte_pos(s);
        const uint32_t upto = (uint32_t)(b.in_len - from < stage ? b.in_len : from + stage);
        staged = (uint8_t*)malloc(upto - from ? upto - from : 1);
        memcpy(staged, pay + from, upto - from);
        inf_staged(s, staged, from, upto);
      } else if (s.wait == kInfWaitTables) {
        for (uint32_t k = 0; k < (1u << kInfLitRoot); ++k) inf_fast_clear(*lit, k);
        for (uint32_t k = 0; k < (1u << kInfDistRoot); ++k) inf_fast_clear(*dist, k);
        for (uint32_t i = 0; i < lit->n_sorted; ++i) inf_fast_fill(*lit, lens, i);
        for (uint32_t i = 0; i < dist->n_sorted; ++i) inf_fast_fill(*dist, lens + s.nlen, i);
      }
      inf_round(s, *lit, *dist, lens, q, kQ);
      for (uint32_t k = 0; k < s.ntok; ++k) {  // in order
        const uint32_t o = inf_tok_out(q[k]), len = inf_tok_len(q[k]), arg = inf_tok_arg(q[k]);
        if (inf_tok_kind(q[k]) == kInfTokStored) memcpy(win + o, pay + arg, len);
        else
          for (uint32_t i = 0; i < len; ++i) win[o + i] = win[o - arg + (arg >= len ? i : i % arg)];  // (as the lanes do it)
      }
    }
    const uint8_t* z = pay + b.in_len;
    const uint32_t stored = (uint32_t)z[0] | ((uint32_t)z[1] << 8) | ((uint32_t)z[2] << 16) | ((uint32_t)z[3] << 24);
    const bool good = s.status == kInfOk;
    const bool crc_ok = !good || crc32_plain(win, b.isize) == stored;
    if (s.out) memcpy(out.data() + b.out_at, win, good ? b.isize : s.out);
    printf("block %zu status %u crc %d\n", bi, s.status, crc_ok ? 1 : 0);
    if (!good && bad < 0) bad = (long)bi;
    if (!crc_ok && crc_bad < 0) crc_bad = (long)bi;
    free(staged);
    free(win);
  }
  printf("blocks %zu out_bytes %zu raw_bytes %zu bad %ld crc %ld\n", blocks.size(), total, raw_bytes, bad, crc_bad);
  FILE* g = fopen(argv[2], "wb");
  if (!g || (!out.empty() && fwrite(out.data(), 1, out.size(), g) != out.size())) return 2;
  fclose(g);
  delete lit;
  delete dist;
  delete[] lens;
  delete[] q;
  return 0;
}
