// fqg_barcode_kernels.hip - the per-read transform of fastq_pre_barcodes on the GPU
// (reference src/fastq_pre_barcodes.c:594-727): lock-step records of up to five files, read
// names must agree, UMI / cell / sample substrings are cut out (with an optional minimum base
// quality), the header gets the STAGS_..._ETAGS_ prefix, reads are optionally sliced, and the
// result is emitted as FASTQ text (one or two outputs), as SAM lines, or as the BAM alignment records that samtools
// 0.1.19 makes of those lines (fastq_pre_barcodes --bam: the file `... --sam | samtools view -b -` writes).
//
// Three launches per batch of iterations; plan and emit work on TILES of T consecutive iterations,
// one wavefront per tile, whose records (contiguous in every input image) are first copied into LDS
// with 16-byte loads:
//   k_bc_plan_tile  one lane per iteration: status (keep / discarded) and the exact number of output bytes of
//                   every output - from the line index and the bytes of the barcode-carrying files alone
//   scan            64-bit exclusive prefix of the byte counts -> where each iteration writes
//   k_bc_emit_tile  the name checks (on the headers of every file, which it stages anyway), then one lane per
//                   output line (SAM), alignment record (BAM) or record (FASTQ): the lane writes its text into the tile's LDS output
//                   area, which then goes to the output image with 16-byte stores; three tiles under way
// T is chosen by the host from the mean record sizes so that a tile fits its LDS areas; a tile that
// does not fit (long reads) is flagged by the plan and handled by the slower direct paths (records read
// from the images, one wavefront per iteration in k_bc_emit_direct).
// Inputs are framed images (line index from fqg_validate); nothing is re-parsed on the host.
#include "fqg_device.h"
#include "fqg_fastq_tile.h"

namespace fqg {

constexpr int kBcFiles = 6;  // index 1..5 as in the reference (READ1, READ2, INDEX1..3)
enum : uint8_t { kBcKeep = 0, kBcDiscardShort = 1, kBcDiscardQual = 2, kBcFinding = 3 };

// tile geometry of one call (host: bc_tile_for)
struct BcTile {
  uint32_t T;        // iterations per tile (<= 64 / lines per iteration)
  uint32_t in_cap;   // LDS bytes for the staged records
  uint32_t out_cap;  // LDS bytes for the output text (emit only)
  uint32_t plan_m;   // the plan kernel works on plan_m tiles at once (one lane per iteration: T * plan_m <= 64)
  uint32_t plan_cap; // LDS bytes for what the plan stages of T * plan_m iterations (bc_staged<PLAN>)
};

struct BcFile {
  FrameView fv;
  uint64_t first;  // record of iteration 0
  uint32_t step;   // records per iteration (2 for the two interleaved references)
  uint32_t add;    // 1 for the second interleaved reference
  int32_t present;
  int32_t fmt;     // read-name format of this file
  int32_t has_nul; // the image holds NUL bytes: lines are C strings (bc_clip_nul)
  int32_t pad_;
};

struct BcParams {
  BcFile f[kBcFiles];
  int32_t n_inputs;
  int32_t umi_read, cell_read, sample_read;
  int32_t phred, min_qual;
  int32_t out_sam, tenx;  // out_sam: 0 FASTQ, FQG_OUT_SAM, FQG_OUT_BAM
  int32_t has_nul;  // some input's image holds NUL bytes: every tile takes the record-by-record kernels (bc_clip_nul)
  int32_t ablate;  // measurement only (FQGPU_BC_ABL, SAM emit): 1 = no line is written, 2 = no flush, 4 = no name check, 8 = no landing of the spans
  int32_t emit[3];
  int64_t umi_off, umi_size, cell_off, cell_size, sample_off, sample_size;
  int64_t read_off[3], read_size[3];
  uint64_t first_read_number;  // processed_reads before this batch
};

struct BcCall {
  unsigned long long first_finding;  // min over iterations of (iteration << 8 | code << 3 | file)
  unsigned long long first_discard;  // first discarded iteration (interleaved input re-syncs there)
  unsigned long long discarded, short_warnings;
  unsigned long long big;  // tiles that do not fit LDS
};

// Which input files exist.  MASK = 0: ask the parameters at run time; otherwise bit x of MASK says
// it at compile time, and the code and registers of absent files disappear from the kernel.
template <int MASK>
__device__ __forceinline__ bool bc_has(const BcParams& P, int x) {
  return MASK ? ((MASK >> x) & 1) != 0 : P.f[x].present != 0;
}

// the four lines of iteration k's record of a file, where they lie in the image
__device__ __forceinline__ void bc_lines(const BcFile& f, uint64_t k, BcLine ln[4]) {
  frame_lines(f.fv, f.first + k * f.step + f.add, f.has_nul != 0, ln);
}

// 8 bytes at any alignment (LDS: one ds_read_b64; gfx950 has unaligned DS access)
__device__ __forceinline__ uint64_t ld8(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

// canonical read name with is_pe set (every input of fastq_pre_barcodes has it, :570).
// WIDE: the line is in LDS with slack behind it - scan 8 bytes per step.
template <bool WIDE>
__device__ __forceinline__ uint32_t bc_name_len(const BcLine& h, int fmt) {
  const uint32_t L = h.len + h.nl - 1;  // strlen(&hdr[1]); images with NUL bytes are refused earlier
  if (fmt == FQG_NAME_CASAVA18) {
    uint32_t sp = L;
    if (WIDE) {
      for (uint32_t i = 0; i < L; i += 8) {
        const uint64_t m = bytes_eq(ld8(h.p + 1 + i), (uint8_t)' ');
        if (m) {
          const uint32_t at = i + ((uint32_t)__builtin_ctzll(m) >> 3);
          if (at < L) sp = at;
          break;
        }
      }
    } else {
      for (uint32_t i = 0; i < L; ++i)
        if (h.p[1 + i] == ' ') {
          sp = i;
          break;
        }
    }
    if (sp >= 2 && h.p[1 + sp - 2] == '/') sp -= 2;
    return sp;
  }
  long l = (long)L;
  if (fmt == FQG_NAME_DEFAULT) l--;
  return l >= 1 ? (uint32_t)(l - 1) : L;
}
__device__ __forceinline__ bool bc_same_bytes_wide(const uint8_t* a, const uint8_t* b, uint32_t n) {
  uint32_t i = 0;
  for (; i + 8 <= n; i += 8)
    if (ld8(a + i) != ld8(b + i)) return false;
  if (i < n) return ((ld8(a + i) ^ ld8(b + i)) & ((1ull << (8 * (n - i))) - 1ull)) == 0;
  return true;
}

// slice_read's effect on one line (src/fastq_pre_barcodes.c:168-189): the result is
// s[from .. from+n) followed by '\n' when add_nl.  s = the line as a C string of length L.
struct Cut {
  uint32_t from, n, add_nl;
};
__device__ __forceinline__ Cut bc_cut(uint32_t L, long off, long size) {
  if (size == 0) return Cut{0, 0, 1};
  if (off > 0 && size == -1) return Cut{0, 0, 0};  // seq[-1]='\n'; seq[0]='\0'
  uint32_t from = 0, Lt = L;
  if (off > 0) {
    from = (uint32_t)((unsigned long)off < L ? off : L);
    Lt = L - from;
  }
  if (size < 0) return Cut{from, Lt, 0};
  if ((unsigned long)size < Lt) return Cut{from, (uint32_t)size, 1};
  if ((unsigned long)size == Lt) return Cut{from, Lt, 1};
  return Cut{from, Lt, 0};
}

__device__ __forceinline__ bool bc_slices(const BcParams& P, int x) {
  if (P.read_off[x] == -1) return false;
  if (P.read_off[x] == 0 && P.read_size[x] == -1) return false;
  return true;
}

__device__ __forceinline__ uint32_t dec_digits(unsigned long v) {
  if (!(v >> 32)) {  // compare chain: no division
    const uint32_t x = (uint32_t)v;
    return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) +
           (x >= 10000000u) + (x >= 100000000u) + (x >= 1000000000u);
  }
  uint32_t d = 1;
  while (v >= 10) {
    v /= 10;
    ++d;
  }
  return d;
}

struct BcTags {
  uint32_t n[3];   // umi, cell, sample lengths (0: absent)
  uint32_t qn[3];  // quality characters that go with them: the reference copies them with strncpy from the quality
                   // STRING (src/fastq_pre_barcodes.c:250-252), which a malformed record may end before offset + size
  const uint8_t* s[3];
  const uint8_t* q[3];
};
// characters of a quality line (with its '\n', as gzgets leaves it) inside [off, off + size)
__device__ __forceinline__ uint32_t bc_qual_chars(const BcLine& q, long off, long size) {
  const long Lq = (long)(q.len + q.nl);
  const long n = Lq - off;
  return (uint32_t)(n < 0 ? 0 : (n < size ? n : size));
}

// get_barcode for one tag (src/fastq_pre_barcodes.c:218-259).  0 ok, 1 short, 2 low quality
template <bool WIDE>
__device__ __forceinline__ int bc_get(const BcLine (&ln)[4], long off, long size, int phred, int min_qual, uint32_t* n,
                                      uint32_t* qn, const uint8_t** s, const uint8_t** q) {
  *n = 0;
  *qn = 0;
  if (off == -1 || size == 0) return 0;
  const unsigned long rl1 = (unsigned long)(ln[1].len + ln[1].nl) - 1ul;
  if ((unsigned long)off > rl1 || (unsigned long)(off + size) > rl1) return 1;
  if (min_qual > 0) {
    const long Lq = (long)(ln[3].len + ln[3].nl);
    if (WIDE && off + size <= Lq) {  // 8 quality characters per LDS access
      for (long x = off; x < off + size; x += 8) {
        const uint64_t v = ld8(ln[3].p + x);
        const int left = (int)(off + size - x);
        bool low = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) low |= j < left && (int)(signed char)(v >> (8 * j)) - phred < min_qual;
        if (low) return 2;
      }
    } else {
      for (long x = off; x < off + size; ++x) {
        const int c = (int)(signed char)(x < Lq ? ln[3].p[x] : 0);
        if (c - phred < min_qual) return 2;
      }
    }
  }
  *n = (uint32_t)size;
  *qn = bc_qual_chars(ln[3], off, size);
  *s = ln[1].p + off;
  *q = ln[3].p + off;
  return 0;
}

// Do two header lines (in LDS, 8 bytes of slack behind them) surely have the same canonical name?  One pass over the
// words of both until they differ - no search for the end of either name:
//   * no difference up to and including the '\n' of the shorter line: the lines are the same line, and so are their
//     names when both files have the same name format;
//   * CASAVA 1.8 (the name ends at the first blank, src/fastq.c:502-511): the byte in front of the first difference is
//     a blank - the first blank of both lines lies in what they share ("... 1:N:0" against "... 2:N:0": the usual case);
//   * DEFAULT with is_pe (the name is the line without its last character, :489-495): lines of one length that differ
//     in that last character first.
// Anything else - and an unterminated last line - is decided by the exact comparison (bc_names_differ).
// The first 32 bytes of both lines are fetched at once when the lines are that long (BcHead: READ1's are fetched once
// for all files): the kernel that makes this test waits for every LDS round trip, so four of them cost what one does.
struct BcHead {
  uint64_t w[4];  // bytes 0..31 of the line
  bool wide;      // ... when it has them
};
__device__ __forceinline__ BcHead bc_head(const BcLine& a) {
  BcHead h;
  h.wide = a.len >= 32;
#pragma unroll
  for (int j = 0; j < 4; ++j) h.w[j] = h.wide ? ld8(a.p + 8 * j) : 0ull;
  return h;
}
__device__ __forceinline__ bool bc_names_agree_fast(const BcLine& a, const BcHead& ha, int fa, const BcLine& b, int fb) {
  if (fa != fb || !(a.nl & b.nl)) return false;
  const uint32_t lmin = a.len < b.len ? a.len : b.len;  // position of the shorter line's '\n'
  uint32_t i = 1, at = 0;
  uint64_t d = 0;
  uint32_t before = 0x100u;  // the byte in front of the first difference, when it is known already
  if (ha.wide && b.len >= 32) {
    uint64_t x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = ha.w[j] ^ ld8(b.p + 8 * j);
    x[0] &= ~0xFFull;  // (byte 0: the '@' of both, checked by the caller)
    if (x[0] | x[1] | x[2] | x[3]) {
      const int j = x[0] ? 0 : (x[1] ? 1 : (x[2] ? 2 : 3));
      d = x[0] ? x[0] : (x[1] ? x[1] : (x[2] ? x[2] : x[3]));
      at = 8u * (uint32_t)j + ((uint32_t)__builtin_ctzll(d) >> 3);  // >= 1, < 32 <= lmin
      const uint32_t q = at - 1;
      const uint64_t wq = (q >> 3) == 0 ? ha.w[0] : ((q >> 3) == 1 ? ha.w[1] : ((q >> 3) == 2 ? ha.w[2] : ha.w[3]));
      before = (uint32_t)(wq >> (8u * (q & 7u))) & 0xFFu;
    } else {
      i = 32;
    }
  }
  if (!d) {
    for (; i <= lmin; i += 8) {
      d = ld8(a.p + i) ^ ld8(b.p + i);
      if (d) break;
    }
    if (!d) return true;  // every byte up to that '\n' is the same (lmin = 0: two empty names)
    at = i + ((uint32_t)__builtin_ctzll(d) >> 3);  // the first byte that differs
    if (at > lmin) return true;
  }
  if (fa == FQG_NAME_CASAVA18) return at >= 2 && (before < 0x100u ? before : (uint32_t)a.p[at - 1]) == ' ';
  if (fa == FQG_NAME_DEFAULT) return a.len == b.len && at + 1 == a.len && at >= 2;
  return false;
}

// canonical names: file x against READ1, exactly (src/fastq_pre_barcodes.c:606-635)
template <bool WIDE>
__device__ __forceinline__ bool bc_names_differ(const BcLine& h1, int f1, const BcLine& hx, int fx) {
  const uint32_t n1 = bc_name_len<WIDE>(h1, f1), nx = bc_name_len<WIDE>(hx, fx);
  bool same = nx == n1;
  if (WIDE) same = same && bc_same_bytes_wide(h1.p + 1, hx.p + 1, n1);
  else
    for (uint32_t i = 0; same && i < n1; ++i) same = h1.p[1 + i] == hx.p[1 + i];
  return !same;
}

// The name checks of one iteration: '@' first in every header (fastq_get_readname, src/fastq.c:448), then every file's
// canonical name against READ1's.  0, or (code << 3) | file of the first check that fails.  These checks come before
// anything else the reference does with an iteration (discards included), but nothing the plan computes depends on
// them: the EMIT kernels make them, on the header bytes they stage anyway (the plan then needs the bytes of the
// barcode-carrying files only).
template <bool WIDE, int MASK = 0>
__device__ __forceinline__ uint32_t bc_check_names(const BcParams& P, const BcLine (&L)[kBcFiles][4]) {
  if (P.n_inputs <= 1) return 0;
  uint32_t bad = 0;
#pragma unroll
  for (int x = kBcFiles - 1; x >= 1; --x)  // (all first bytes are fetched before any is looked at; the first file wins)
    if (bc_has<MASK>(P, x) && L[x][0].p[0] != '@') bad = (FQG_E_WRONG_HEADER << 3) | x;
  if (bad) return bad;
  BcHead h1;
  if (WIDE) h1 = bc_head(L[1][0]);
#pragma unroll
  for (int x = 2; x < kBcFiles; ++x)
    if (bc_has<MASK>(P, x)) {
      if (WIDE && bc_names_agree_fast(L[1][0], h1, P.f[1].fmt, L[x][0], P.f[x].fmt)) continue;
      if (bc_names_differ<WIDE>(L[1][0], P.f[1].fmt, L[x][0], P.f[x].fmt)) return (FQG_E_NAME_MISMATCH << 3) | x;
    }
  return 0;
}

// status + tags of one iteration from the lines of its records (in an image or in LDS): extract_info for each file in
// order - umi, sample, cell (src/fastq_pre_barcodes.c:262-285).  Only the lines of the barcode-carrying files are
// looked at, and their BYTES only when a minimum quality is asked for (bc_plan_staged).
template <bool WIDE, int MASK = 0>
__device__ __forceinline__ uint8_t bc_decide_lines(const BcParams& P, const BcLine (&L)[kBcFiles][4], BcTags* tags) {
  tags->n[0] = tags->n[1] = tags->n[2] = 0;
  tags->qn[0] = tags->qn[1] = tags->qn[2] = 0;
#pragma unroll
  for (int x = 1; x < kBcFiles; ++x)
    if (bc_has<MASK>(P, x)) {
      int rc = 0;
      if (P.umi_read == x) rc = bc_get<WIDE>(L[x], P.umi_off, P.umi_size, P.phred, P.min_qual, &tags->n[0], &tags->qn[0], &tags->s[0], &tags->q[0]);
      if (!rc && P.sample_read == x)
        rc = bc_get<WIDE>(L[x], P.sample_off, P.sample_size, P.phred, P.min_qual, &tags->n[2], &tags->qn[2], &tags->s[2], &tags->q[2]);
      if (!rc && P.cell_read == x)
        rc = bc_get<WIDE>(L[x], P.cell_off, P.cell_size, P.phred, P.min_qual, &tags->n[1], &tags->qn[1], &tags->s[1], &tags->q[1]);
      if (rc) return rc == 1 ? kBcDiscardShort : kBcDiscardQual;
    }
  return kBcKeep;
}

// tags of an iteration that bc_decide_lines has already found to be kept: geometry only, none of
// the byte-by-byte checks
template <int MASK = 0>
__device__ __forceinline__ void bc_tags_of_kept(const BcParams& P, const BcLine (&lines)[kBcFiles][4], BcTags* tags) {
  tags->n[0] = tags->n[1] = tags->n[2] = 0;
  tags->qn[0] = tags->qn[1] = tags->qn[2] = 0;
#pragma unroll
  for (int x = 1; x < kBcFiles; ++x)
    if (bc_has<MASK>(P, x) && (P.umi_read == x || P.sample_read == x || P.cell_read == x)) {
      const BcLine(&ln)[4] = lines[x];
      auto take = [&](int slot, long off, long size) {
        if (off == -1 || size == 0) return;
        tags->n[slot] = (uint32_t)size;
        tags->qn[slot] = bc_qual_chars(ln[3], off, size);
        tags->s[slot] = ln[1].p + off;
        tags->q[slot] = ln[3].p + off;
      };
      if (P.umi_read == x) take(0, P.umi_off, P.umi_size);
      if (P.sample_read == x) take(2, P.sample_off, P.sample_size);
      if (P.cell_read == x) take(1, P.cell_off, P.cell_size);
    }
}

// byte count of the FASTQ record written for a file (src/fastq_pre_barcodes.c:713-718);
// sliced / off / size: bc_slices(P, x), P.read_off[x], P.read_size[x]
__device__ __forceinline__ uint32_t bc_fastq_len(bool sliced, long off, long size, const BcLine (&ln)[4], const BcTags& t) {
  const bool tagged = (t.n[0] | t.n[1] | t.n[2]) != 0;
  uint32_t n = ln[0].len + ln[0].nl + (tagged ? 31u + t.n[0] + t.n[1] + t.n[2] : 0u);
  if (tagged && n >= (uint32_t)FQG_MAX_LABEL_LENGTH) {  // the tagged header runs over hdr1[] into hdr2[]: bc_emit_fastq
    n = n == (uint32_t)FQG_MAX_LABEL_LENGTH ? n : (uint32_t)FQG_MAX_LABEL_LENGTH + 2u;
    n += n == (uint32_t)FQG_MAX_LABEL_LENGTH ? 0u : 2u;
  } else
    n += (tagged || sliced) ? 2u : ln[2].len + ln[2].nl;
  if (sliced) {
    const Cut cs = bc_cut(ln[1].len + ln[1].nl, off, size);
    const Cut cq = bc_cut(ln[3].len + ln[3].nl, off, size);
    n += cs.n + cs.add_nl + cq.n + cq.add_nl;
  } else {
    n += ln[1].len + ln[1].nl + ln[3].len + ln[3].nl;
  }
  return n;
}

// what the SAM line prints for a mate: sequence / quality without their last character
// (src/fastq_pre_barcodes.c:666-700)
struct SamGeom {
  Cut cs, cq;
  uint32_t seq_n, qual_n;  // characters printed
  uint32_t shown;          // the number in column 9
  uint32_t name_n;         // characters of the on:Z: value
};
__device__ __forceinline__ SamGeom bc_sam_geom(bool sliced, long off, long size, bool mate1, const BcLine (&ln)[4]) {
  SamGeom g;
  const uint32_t Ls = ln[1].len + ln[1].nl, Lq = ln[3].len + ln[3].nl;
  if (sliced) {
    g.cs = bc_cut(Ls, off, size);
    g.cq = bc_cut(Lq, off, size);
  } else {
    g.cs = Cut{0, Ls, 0};
    g.cq = Cut{0, Lq, 0};
  }
  const uint32_t ls = g.cs.n + g.cs.add_nl, lq = g.cq.n + g.cq.add_nl;  // strlen after slicing
  g.seq_n = ls ? ls - 1 : 0;
  g.qual_n = lq ? lq - 1 : 0;
  g.shown = mate1 ? ls - 1u : ls;  // unsigned arithmetic as in the reference (len-1 for mate 1, len for mate 2)
  // format_read_name: up to the first '\n' of the header, without the '@'
  g.name_n = ln[0].len ? ln[0].len - 1 : 0;
  return g;
}

// one SAM line: number = the read number printed in column 1
__device__ __forceinline__ uint32_t bc_sam_line_len(unsigned long number, unsigned flag, const SamGeom& g, const BcTags& t) {
  uint32_t n = dec_digits(number) + 1 + dec_digits(flag);
  n += 15;  // "\t*\t0\t255\t*\t*\t0\t"
  n += dec_digits(g.shown) + 1 + g.seq_n + 1 + g.qual_n + 6 + g.name_n + 6 + g.qual_n;
  if (t.n[0]) n += 12 + t.n[0] + t.qn[0];
  if (t.n[1]) n += 12 + t.n[1] + t.qn[1];
  if (t.n[2]) n += 12 + t.n[2] + t.qn[2];
  return n + 1;
}
__device__ __forceinline__ unsigned bc_sam_flag(bool se, bool mate1) {
  return se ? 4u : (mate1 ? 77u : 141u);  // BAM_FUNMAP | FMUNMAP | FPAIRED | FREAD1/2
}

// ---- the SAM line as an alignment record (out_sam == FQG_OUT_BAM) ----
// What libbam 0.1.19 (sam_read1, bam_import.c:237-467; bam_write1) makes of the line above: the fields are cut at every
// isspace() byte but the blank (kseq.h KS_SEP_TAB), the read number is the name, "*" / "0" become -1, the bases go
// through bam_nt16_table at four bits each, the qualities are byte - 33 (a QUAL of exactly "*": 0xff), and every
// xx:Z:value becomes xx, 'Z', value, NUL.  The second mate's " CR:Z:" (a blank, no tab) stays in the value of the field
// in front of it.
// A finding that is not the reference's: the line is one that libbam aborts on or reads foreign memory for.  Internal
// value (5 bits in BcCall::first_finding, behind the name findings of the same iteration); the library reports
// FQG_E_BAM_RECORD.
constexpr uint32_t kBcFindBam = 31;
__device__ __forceinline__ uint32_t bc_bam_record_len(unsigned long number, bool mate1, const SamGeom& g, const BcTags& t) {
  uint32_t n = 36 + dec_digits(number) + 1 + ((g.seq_n + 1) >> 1) + g.seq_n + 4 + g.name_n + 4 + g.qual_n;
  if (t.n[0]) n += 8 + t.n[0] + t.qn[0];
  if (t.n[1]) n += (mate1 ? 8u : 10u) + t.n[1] + t.qn[1];
  if (t.n[2]) n += 8 + t.n[2] + t.qn[2];
  return n;
}
// what the line's GEOMETRY says against it: an empty SEQ or QUAL (an empty QUAL is an empty op:Z: as well), SEQ and QUAL
// of different lengths (a QUAL of one character may be "*": the emit kernel looks), an empty aux value
__device__ __forceinline__ bool bc_bam_refused(bool mate1, const SamGeom& g, const BcTags& t) {
  bool bad = g.seq_n == 0 || g.qual_n == 0 || g.name_n == 0 || (g.qual_n != g.seq_n && g.qual_n != 1);
  bad |= t.n[0] && !t.qn[0] && (mate1 || !t.n[1]);  // (the second mate's QX / UY value ends in " CR:Z:...")
  bad |= (t.n[1] && !t.qn[1]) || (t.n[2] && !t.qn[2]);
  return bad;
}
// the record of one mate of an iteration: its bytes; *finding becomes (code << 3 | mate) when it has none yet
__device__ __forceinline__ uint32_t bc_bam_mate_len(const BcParams& P, uint64_t k, bool mate1, const BcLine (&ln)[4],
                                                    const BcTags& t, uint32_t* finding) {
  const int x = mate1 ? 1 : 2;
  const SamGeom g = bc_sam_geom(bc_slices(P, x), P.read_off[x], P.read_size[x], mate1, ln);
  if (!*finding && bc_bam_refused(mate1, g, t)) *finding = (kBcFindBam << 3) | (uint32_t)x;
  return bc_bam_record_len(P.first_read_number + k + 1, mate1, g, t);
}

// byte counts of the outputs of a kept iteration
template <bool BAM>
__device__ __forceinline__ void bc_out_lens(const BcParams& P, uint64_t k, const BcLine (&L)[kBcFiles][4], const BcTags& t,
                                            uint32_t* a, uint32_t* b, uint32_t* c, uint32_t* finding) {
  *a = *b = *c = 0;
  if (BAM) {
    *a = bc_bam_mate_len(P, k, true, L[1], t, finding);
    if (P.f[2].present) *a += bc_bam_mate_len(P, k, false, L[2], t, finding);
  } else if (P.out_sam) {
    const bool se = !P.f[2].present;
    *a = bc_sam_line_len(P.first_read_number + k + 1, bc_sam_flag(se, true),
                         bc_sam_geom(bc_slices(P, 1), P.read_off[1], P.read_size[1], true, L[1]), t);
    if (!se)
      *a += bc_sam_line_len(P.first_read_number + k + 1, bc_sam_flag(se, false),
                            bc_sam_geom(bc_slices(P, 2), P.read_off[2], P.read_size[2], false, L[2]), t);
  } else {
    if (P.emit[1]) *b = bc_fastq_len(bc_slices(P, 1), P.read_off[1], P.read_size[1], L[1], t);
    if (P.emit[2]) *c = bc_fastq_len(bc_slices(P, 2), P.read_off[2], P.read_size[2], L[2], t);
  }
}

// bc_decide_lines and bc_out_lens for the kernels for any set of files: the lines of a file are asked for (lines_of(x, ln))
// only inside the branch that looks at them - files that carry no barcode are never asked for
template <bool WIDE, int MASK, class LinesOf>
__device__ __forceinline__ uint8_t bc_decide_with(const BcParams& P, LinesOf lines_of, BcTags* tags) {
  tags->n[0] = tags->n[1] = tags->n[2] = 0;
  tags->qn[0] = tags->qn[1] = tags->qn[2] = 0;
#pragma unroll
  for (int x = 1; x < kBcFiles; ++x)
    if (bc_has<MASK>(P, x) && (P.umi_read == x || P.sample_read == x || P.cell_read == x)) {
      BcLine ln[4];
      lines_of(x, ln);
      int rc = 0;
      if (P.umi_read == x) rc = bc_get<WIDE>(ln, P.umi_off, P.umi_size, P.phred, P.min_qual, &tags->n[0], &tags->qn[0], &tags->s[0], &tags->q[0]);
      if (!rc && P.sample_read == x)
        rc = bc_get<WIDE>(ln, P.sample_off, P.sample_size, P.phred, P.min_qual, &tags->n[2], &tags->qn[2], &tags->s[2], &tags->q[2]);
      if (!rc && P.cell_read == x)
        rc = bc_get<WIDE>(ln, P.cell_off, P.cell_size, P.phred, P.min_qual, &tags->n[1], &tags->qn[1], &tags->s[1], &tags->q[1]);
      if (rc) return rc == 1 ? kBcDiscardShort : kBcDiscardQual;
    }
  return kBcKeep;
}
template <int MASK, bool BAM, class LinesOf>
__device__ __forceinline__ void bc_out_lens_with(const BcParams& P, uint64_t k, LinesOf lines_of, const BcTags& t, uint32_t* a,
                                                 uint32_t* b, uint32_t* c, uint32_t* finding) {
  *a = *b = *c = 0;
  const bool se = !bc_has<MASK>(P, 2);
  if (BAM) {
    {
      BcLine ln[4];
      lines_of(1, ln);
      *a = bc_bam_mate_len(P, k, true, ln, t, finding);
    }
    if (!se) {
      BcLine ln[4];
      lines_of(2, ln);
      *a += bc_bam_mate_len(P, k, false, ln, t, finding);
    }
    return;
  }
  if (P.out_sam || P.emit[1]) {
    BcLine ln[4];
    lines_of(1, ln);
    if (P.out_sam)
      *a = bc_sam_line_len(P.first_read_number + k + 1, bc_sam_flag(se, true),
                           bc_sam_geom(bc_slices(P, 1), P.read_off[1], P.read_size[1], true, ln), t);
    else *b = bc_fastq_len(bc_slices(P, 1), P.read_off[1], P.read_size[1], ln, t);
  }
  if (!se && (P.out_sam || P.emit[2])) {
    BcLine ln[4];
    lines_of(2, ln);
    if (P.out_sam)
      *a += bc_sam_line_len(P.first_read_number + k + 1, bc_sam_flag(se, false),
                            bc_sam_geom(bc_slices(P, 2), P.read_off[2], P.read_size[2], false, ln), t);
    else *c = bc_fastq_len(bc_slices(P, 2), P.read_off[2], P.read_size[2], ln, t);
  }
}

// ---- tiles: the records of T consecutive iterations of every file, copied into LDS ----------------
// Two dependent round trips to memory per tile: the line index of the tile's records (what a lane
// needs to know its iteration's lines, and lane 0 / the last lane to know the tile's byte span),
// then the spans themselves.  The emit kernel keeps three tiles under way (tile_walk, fqg_fastq_tile.h); the plan
// kernel requests the next tile's index with the current tile's spans.
struct TileGeo {
  BcGeo f[kBcFiles];
  // emit: the iteration's place in each output is off + sum (added where it is used: an addition inside the function
  // that requests the loads would make the wavefront wait for them there)
  unsigned long long off[3], sum[3];
  uint32_t olen[3];             // emit: ... and the bytes it has there (what the plan computed)
  uint8_t st;                   // emit: status
  uint8_t big;                  // emit: tile flag
};
__device__ __forceinline__ void bc_geo_load(const BcFile& f, uint64_t k, BcGeo& g) {
  const uint64_t r = f.first + k * f.step + f.add;
  const uint64_t* __restrict__ le = f.fv.line_end + 4 * r;
  g.r0 = r == 0 ? 1u : 0u;
  g.praw = le[r == 0 ? 0 : -1];
#pragma unroll
  for (int i = 0; i < 4; ++i) g.e[i] = le[i];
}
// which files a kernel stages.  The emit kernels (and the record filters): every input - they print the records and
// compare the names.  PLAN: only the files a barcode is cut from, and those only when a minimum quality is asked for
// (get_barcode reads quality characters then); everything else the plan needs - line lengths - is in the line index.
template <bool PLAN, int MASK>
__device__ __forceinline__ bool bc_staged(const BcParams& P, int x) {
  if (!bc_has<MASK>(P, x)) return false;
  if (PLAN && (P.min_qual <= 0 || (P.umi_read != x && P.cell_read != x && P.sample_read != x))) return false;
  return true;
}

// Where the spans of a tile lie: the tile's records of every staged file are one byte span, cut into 16-byte units
// aligned on the image ADDRESS; the units of all files are numbered through.
struct SpanPlan {
  const uint8_t* gbase[kBcFiles];  // address of the file's unit 0 minus 16 * its first unit number
  uint32_t first_unit[kBcFiles], skew[kBcFiles];
  uint64_t s0[kBcFiles];
  uint32_t units;
  bool fit;  // the spans fit in_cap
};
template <bool PLAN, int MASK>
__device__ __forceinline__ void bc_span_plan(const BcParams& P, const TileGeo& tg, int last_lane, uint32_t in_cap, SpanPlan& sp) {
  sp.units = 0;
  sp.fit = true;
#pragma unroll
  for (int x = 1; x < kBcFiles; ++x) {
    sp.first_unit[x] = 0xFFFFFFFFu;  // never selected
    sp.gbase[x] = P.f[1].fv.img;
    sp.skew[x] = 0;
    sp.s0[x] = 0;
    if (!bc_staged<PLAN, MASK>(P, x)) continue;
    const BcFile& f = P.f[x];
    sp.s0[x] = rfl64(tg.f[x].start());
    const uint64_t e3l = rl64(tg.f[x].e[3], last_lane);
    const uint64_t n = (e3l < f.fv.nbytes ? e3l + 1 : e3l) - sp.s0[x];
    sp.skew[x] = (uint32_t)((uintptr_t)(f.fv.img + sp.s0[x]) & 15u);
    sp.first_unit[x] = sp.units;
    sp.gbase[x] = f.fv.img + sp.s0[x] - sp.skew[x] - 16ull * sp.units;
    if (!span_fits(sp.skew[x], n, in_cap, sp.units)) sp.fit = false;
  }
}
// where unit u of the plan lies (span_unit)
__device__ __forceinline__ const uint8_t* span_base(const SpanPlan& sp, uint32_t u) {
  const uint8_t* base = sp.gbase[1];  // (the staged file that comes first has first_unit 0: READ1, or the loop finds it)
#pragma unroll
  for (int x = 2; x < kBcFiles; ++x) {
    // (a VALUE on either side: "c ? sp.gbase[x] : base" is an lvalue - the compiler selects between the two ADDRESSES and
    // loads once, the plan stays in scratch memory, and every unit of the any-set-of-files kernels waited for that load)
    const uint8_t* const gx = sp.gbase[x];
    base = u >= sp.first_unit[x] ? static_cast<const uint8_t*>(gx) : static_cast<const uint8_t*>(base);
  }
  return base;
}
// the lane's lines: pointers into the staged spans (a file that is not staged: the lengths of its lines, no bytes -
// pointers that are never followed)
// (one file's lines: the kernels for any set of files ask for them where they use them - five files' lines at once are 80
// registers)
template <bool PLAN, int MASK>
__device__ __forceinline__ void bc_file_lines(const BcParams& P, const TileGeo& tg, const SpanPlan& sp, uint8_t* s_in, int x,
                                              BcLine (&ln)[4]) {
  const BcGeo& g = tg.f[x];
  const uint64_t nb = P.f[x].fv.nbytes;
  const bool st = bc_staged<PLAN, MASK>(P, x);
  uint8_t* b = st ? s_in + 16u * sp.first_unit[x] + sp.skew[x] : s_in;
  const uint64_t s0 = st ? sp.s0[x] : g.start();
  ln[0] = BcLine{b + (uint32_t)(g.start() - s0), (uint32_t)(g.e[0] - g.start()), g.e[0] < nb ? 1u : 0u};
  ln[1] = BcLine{b + (uint32_t)(g.e[0] + 1 - s0), (uint32_t)(g.e[1] - g.e[0] - 1), g.e[1] < nb ? 1u : 0u};
  ln[2] = BcLine{b + (uint32_t)(g.e[1] + 1 - s0), (uint32_t)(g.e[2] - g.e[1] - 1), g.e[2] < nb ? 1u : 0u};
  ln[3] = BcLine{b + (uint32_t)(g.e[2] + 1 - s0), (uint32_t)(g.e[3] - g.e[2] - 1), g.e[3] < nb ? 1u : 0u};
}
template <bool PLAN, int MASK>
__device__ __forceinline__ void bc_span_lines(const BcParams& P, const TileGeo& tg, const SpanPlan& sp, uint8_t* s_in,
                                              BcLine (&L)[kBcFiles][4]) {
#pragma unroll
  for (int x = 1; x < kBcFiles; ++x) {
    if (!bc_has<MASK>(P, x)) continue;
    bc_file_lines<PLAN, MASK>(P, tg, sp, s_in, x, L[x]);
  }
}

// Copies the spans into s_in and gives the lane its lines (pointers into LDS).  Returns false
// (uniformly, before copying anything) when the spans do not fit in_cap.
template <bool PLAN, int MASK>
__device__ __forceinline__ bool bc_stage_tile(const BcParams& P, const TileGeo& tg, int last_lane, int lane, uint8_t* s_in,
                                              uint32_t in_cap, BcLine (&L)[kBcFiles][4]) {
  SpanPlan sp;
  bc_span_plan<PLAN, MASK>(P, tg, last_lane, in_cap, sp);
  if (!sp.fit) return false;
  span_copy(sp, 0, lane, s_in);
  bc_span_lines<PLAN, MASK>(P, tg, sp, s_in, L);
  return true;
}

// Would the records of the iterations held by lanes first_lane .. last_lane fit the input area of ONE emit
// tile?  The unit count that bc_span_plan makes for that tile (the emit kernels stage every input), by the same rule.
template <int MASK>
__device__ __forceinline__ bool bc_emit_tile_fits(const BcParams& P, const TileGeo& tg, int first_lane, int last_lane,
                                                  uint32_t in_cap) {
  uint32_t units = 0;
  bool fit = true;
#pragma unroll
  for (int x = 1; x < kBcFiles; ++x) {
    if (!bc_has<MASK>(P, x)) continue;
    const BcFile& f = P.f[x];
    const uint64_t s0 = rl64(tg.f[x].start(), first_lane);
    const uint64_t e3l = rl64(tg.f[x].e[3], last_lane);
    const uint64_t n = (e3l < f.fv.nbytes ? e3l + 1 : e3l) - s0;
    const uint32_t skew = (uint32_t)((uintptr_t)(f.fv.img + s0) & 15u);
    if (!span_fits(skew, n, in_cap, units)) fit = false;
  }
  return fit;
}

template <int MASK = 0>
__device__ __forceinline__ void bc_lines_all(const BcParams& P, uint64_t k, BcLine (&L)[kBcFiles][4]) {
#pragma unroll
  for (int x = 1; x < kBcFiles; ++x)
    if (bc_has<MASK>(P, x)) bc_lines(P.f[x], k, L[x]);
}

// a finding of an iteration (the names: the emit kernels; a refused BAM record: the plan too): the smallest (iteration << 8 | code << 3 | file) wins
__device__ __forceinline__ void bc_report_finding(BcCall* __restrict__ call, bool active, uint64_t k, uint32_t finding) {
  if (!__ballot(active && finding != 0)) return;  // (the usual case: one ballot)
  const unsigned long long none = ~0ull;
  const unsigned long long fnd = wave_min64(active && finding ? (unsigned long long)((k << 8) | finding) : none);
  if ((threadIdx.x & 63) == 0 && fnd < __atomic_load_n(&call->first_finding, __ATOMIC_RELAXED)) atomicMin(&call->first_finding, fnd);
}

// One wavefront per PLAN tile = plan_m consecutive tiles of the emit kernel, one lane per iteration.  The plan decides
// what the iteration's output is made of - keep / discard (get_barcode's bounds and minimum quality) and the byte count
// of every output - from the line index and the bytes of the barcode-carrying files alone (bc_staged<PLAN>): its LDS
// holds little, so many wavefronts are resident.  The name checks, which need the header bytes of every file, are made
// by the emit kernels on the records they stage anyway (bc_check_names).  What the plan decides per emit tile - does
// the tile fit the emit kernel's LDS areas - is worked out per group of T lanes.  MASK: see bc_has.
//
// How each instantiation hides its round trips to memory (measured on 200 M pairs of READ1 + INDEX1 and 50 M iterations of
// four files; the other sets of files keep what they had):
//   any set of files (MASK 0): no index of a second tile in flight, a file's lines made where they are looked at
//     (bc_decide_with) - 128 registers, FOUR wavefronts per SIMD: 2.0 ms where five files' lines at once (233 registers,
//     two wavefronts) took 3.6;
//   READ1 + INDEX1: no second tile in flight either, 96 registers, FIVE wavefronts: 7.8 ms against 8.4 with the next
//     tile's index requested ahead and four wavefronts;
//   the other specialised sets: the next tile's index requested ahead (many wavefronts are resident here - little LDS -
//     and hide each other's round trips: the three-tile scheme of the emit kernel made this kernel slower, 7.7 -> 11.2 ms).
template <int MASK>
struct PlanShape {
  static constexpr bool ahead = MASK != 0 && MASK != 0x0A;
  static constexpr int waves = MASK == 0 ? 4 : (MASK == 0x0A ? 5 : 1);
};
// BAM: the byte counts are those of alignment records (out_sam == FQG_OUT_BAM), and a record that is refused is a
// finding - a kernel of its own, so that the kernels of the other two outputs stay what they were.
template <int MASK, bool BAM = false>
__global__ __launch_bounds__(kWave, PlanShape<MASK>::waves) void k_bc_plan_tile(BcParams P, BcTile tc, uint64_t n_iter, uint8_t* __restrict__ status,
                                                        uint32_t* __restrict__ len0, uint32_t* __restrict__ len1,
                                                        uint32_t* __restrict__ len2, uint8_t* __restrict__ tile_big,
                                                        BcCall* __restrict__ call) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_lds[];
  const int lane = (int)threadIdx.x;
  const uint32_t Tp = tc.T * tc.plan_m, plan_cap = tc.plan_cap;
  const uint64_t n_tiles = (n_iter + Tp - 1) / Tp;
  auto tile_size = [&](uint64_t tile) {
    const uint64_t left = n_iter - tile * Tp;
    return (uint32_t)(left < (uint64_t)Tp ? left : (uint64_t)Tp);
  };
  auto geo_of = [&](uint64_t tile, TileGeo& tg) {
    const uint32_t Tn = tile_size(tile);
    const uint64_t k = tile * Tp + ((uint32_t)lane < Tn ? (uint32_t)lane : Tn - 1);
#pragma unroll
    for (int x = 1; x < kBcFiles; ++x)
      if (bc_has<MASK>(P, x)) bc_geo_load(P.f[x], k, tg.f[x]);
  };
  TileGeo cur, nxt;
  uint32_t n_dropped = 0, n_short = 0;  // of this wavefront's tiles: added to the call's totals once, at the end
  constexpr bool kAhead = PlanShape<MASK>::ahead;  // (false: a tile's index is asked for when the wavefront gets there)
  if (kAhead && blockIdx.x < n_tiles) geo_of(blockIdx.x, cur);
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t k0 = tile * Tp;
    const uint32_t Tn = tile_size(tile);
    const bool valid = (uint32_t)lane < Tn;
    const uint64_t k = k0 + (valid ? (uint32_t)lane : Tn - 1);
    BcLine L[kBcFiles][4];
    if (kAhead) geo_of(tile + gridDim.x < n_tiles ? tile + gridDim.x : n_tiles - 1, nxt);  // the next tile's index (requested without a branch)
    else geo_of(tile, cur);
    // (an image with NUL bytes: lines are C strings, found by scanning them where they lie - bc_lines)
    BcTags t;
    uint32_t a = 0, b = 0, c = 0, refused = 0;  // refused: the iteration's line is none libbam takes (BAM records only)
    uint8_t st;
    if constexpr (MASK == 0) {
      // any set of files: a file's lines are made where they are looked at (bc_decide_with) - never all five at once
      SpanPlan sp;
      bc_span_plan<true, MASK>(P, cur, (int)Tn - 1, plan_cap, sp);
      const bool fit = !P.has_nul && sp.fit;
      if (fit) span_copy(sp, 0, lane, s_lds);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (fit) {
        auto staged = [&](int x, BcLine(&ln)[4]) { bc_file_lines<true, MASK>(P, cur, sp, s_lds, x, ln); };
        st = bc_decide_with<true, MASK>(P, staged, &t);
        if (st == kBcKeep) bc_out_lens_with<MASK, BAM>(P, k, staged, t, &a, &b, &c, &refused);
      } else {  // long reads: from the images
        auto from_image = [&](int x, BcLine(&ln)[4]) { bc_lines(P.f[x], k, ln); };
        st = bc_decide_with<false, MASK>(P, from_image, &t);
        if (st == kBcKeep) bc_out_lens_with<MASK, BAM>(P, k, from_image, t, &a, &b, &c, &refused);
      }
    } else {
      const bool fit = !P.has_nul && bc_stage_tile<true, MASK>(P, cur, (int)Tn - 1, lane, s_lds, plan_cap, L);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (fit) {
        st = bc_decide_lines<true, MASK>(P, L, &t);
        if (st == kBcKeep) bc_out_lens<BAM>(P, k, L, t, &a, &b, &c, &refused);
      } else {  // long reads: from the images
        BcLine G[kBcFiles][4];
        bc_lines_all<MASK>(P, k, G);
        st = bc_decide_lines<false, MASK>(P, G, &t);
        if (st == kBcKeep) bc_out_lens<BAM>(P, k, G, t, &a, &b, &c, &refused);
      }
    }
    if (valid) {
      status[k] = st;
      if (P.out_sam) len0[k] = a;
      else {
        if (P.emit[1]) len1[k] = b;
        if (P.emit[2]) len2[k] = c;
      }
    } else {
      a = b = c = 0;
    }
    if (BAM) bc_report_finding(call, valid, k, valid ? refused : 0u);
    const unsigned long long none = ~0ull;
    const bool dropped = valid && (st == kBcDiscardShort || st == kBcDiscardQual);
    n_dropped += dropped ? 1u : 0u;
    n_short += valid && st == kBcDiscardShort ? 1u : 0u;
    const unsigned long long dsc = wave_min64(dropped ? (unsigned long long)k : none);
    // the emit tiles inside this plan tile
    for (uint32_t j = 0; j * tc.T < Tn; ++j) {
      const uint32_t first = j * tc.T, last = (first + tc.T < Tn ? first + tc.T : Tn) - 1;
      const bool mine = (uint32_t)lane >= first && (uint32_t)lane <= last;
      const uint32_t sa = wave_sum32(mine ? a : 0u), sb = wave_sum32(mine ? b : 0u), sc = wave_sum32(mine ? c : 0u);
      const bool fits_in = bc_emit_tile_fits<MASK>(P, cur, (int)first, (int)last, tc.in_cap);
      if (lane == 0) {
        const bool big = P.has_nul || !fits_in || sa + 32 > tc.out_cap || sb + 32 > tc.out_cap || sc + 32 > tc.out_cap;
        tile_big[tile * tc.plan_m + j] = big ? 1 : 0;
        if (big) atomicAdd(&call->big, 1ull);
      }
    }
    // tiles run roughly in order: look before the atomic, almost every later tile has nothing to add
    if (lane == 0 && dsc != none && dsc < __atomic_load_n(&call->first_discard, __ATOMIC_RELAXED))
      atomicMin(&call->first_discard, dsc);
    __builtin_amdgcn_wave_barrier();
    if (kAhead) cur = nxt;
  }
  // the discarded iterations of all n_iter (k_bc_count counts again when the batch ends earlier: interleaved input)
  n_dropped = wave_sum32(n_dropped);
  n_short = wave_sum32(n_short);
  if (lane == 0) {
    if (n_dropped) atomicAdd(&call->discarded, (unsigned long long)n_dropped);
    if (n_short) atomicAdd(&call->short_warnings, (unsigned long long)n_short);
  }
}

// discarded iterations among the first n_done: one atomic per workgroup
__global__ __launch_bounds__(kBlock) void k_bc_count(const uint8_t* __restrict__ status, uint64_t n_done,
                                                     BcCall* __restrict__ call) {
  __shared__ unsigned long long s_d[kBlock / kWave], s_s[kBlock / kWave];
  unsigned long long d = 0, sh = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < n_done; k += (uint64_t)gridDim.x * kBlock) {
    const uint8_t st = status[k];
    d += (st == kBcDiscardShort || st == kBcDiscardQual) ? 1u : 0u;
    sh += st == kBcDiscardShort ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    d += __shfl_xor(d, o, 64);
    sh += __shfl_xor(sh, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_d[threadIdx.x >> 6] = d;
    s_s[threadIdx.x >> 6] = sh;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long td = 0, ts = 0;
    for (int w = 0; w < kBlock / kWave; ++w) {
      td += s_d[w];
      ts += s_s[w];
    }
    if (td) atomicAdd(&call->discarded, td);
    if (ts) atomicAdd(&call->short_warnings, ts);
  }
}

// ---- emit -----------------------------------------------------------------------------------
// up to 16 characters of a literal as two 64-bit immediates (no memory access when written)
constexpr uint64_t lit_pack(const char* s, int n, int from) {
  uint64_t v = 0;
  for (int i = 0; i < 8 && from + i < n; ++i) v |= (uint64_t)(uint8_t)s[from + i] << (8 * i);
  return v;
}
#define BC_LIT(w, str) (w).lit_imm(lit_pack(str, (int)sizeof(str) - 1, 0), lit_pack(str, (int)sizeof(str) - 1, 8), (uint32_t)sizeof(str) - 1)

// the whole wavefront writes one text: lane i copies byte i of every piece (k_bc_emit_direct)
struct Writer {
  uint8_t* p;
  int lane;
  __device__ __forceinline__ void lit_imm(uint64_t lo, uint64_t hi, uint32_t n) {
    if ((uint32_t)lane < n) p[lane] = (uint8_t)((lane < 8 ? lo >> (8 * lane) : hi >> (8 * (lane - 8))) & 0xFFu);
    p += n;
  }
  __device__ __forceinline__ void bytes(const uint8_t* s, uint32_t n) {
    for (uint32_t i = lane; i < n; i += kWave) p[i] = s[i];
    p += n;
  }
  __device__ __forceinline__ void ch(char c) {
    if (lane == 0) p[0] = (uint8_t)c;
    p += 1;
  }
  __device__ __forceinline__ void dec(unsigned long v) {
    const uint32_t d = dec_digits(v);
    if (lane == 0) {
      for (uint32_t i = 0; i < d; ++i) {
        p[d - 1 - i] = (uint8_t)('0' + v % 10);
        v /= 10;
      }
    }
    p += d;
  }
  // header text for on:Z: - blanks become '@' (format_read_name, src/fastq_pre_barcodes.c:300-308)
  __device__ __forceinline__ void name(const uint8_t* s, uint32_t n) {
    for (uint32_t i = lane; i < n; i += kWave) p[i] = s[i] == ' ' ? (uint8_t)'@' : s[i];
    p += n;
  }
  __device__ __forceinline__ void bytes_twice(const uint8_t* s, uint32_t n, uint32_t dist) {
    for (uint32_t i = lane; i < n; i += kWave) p[i] = p[dist + i] = s[i];
    p += n;
  }
  __device__ __forceinline__ void skip(uint32_t n) { p += n; }
};

// one lane writes one text (k_bc_emit_tile: sources and destination are LDS, at any alignment).
// Copies move 8 bytes per LDS access; the last access of a piece overlaps the one before it, or
// is split 4/2/1 for pieces shorter than 8.
struct LaneWriter {
  uint8_t* p;
  template <int N>
  __device__ __forceinline__ void put(uint64_t v) {  // the low N bytes of v
    if (N == 8) __builtin_memcpy(p, &v, 8);
    else {
      uint32_t done = 0;
      if (N & 4) {
        const uint32_t w = (uint32_t)v;
        __builtin_memcpy(p, &w, 4);
        done = 4;
      }
      if (N & 2) {
        const uint16_t w = (uint16_t)(v >> (8 * done));
        __builtin_memcpy(p + done, &w, 2);
        done += 2;
      }
      if (N & 1) p[done] = (uint8_t)(v >> (8 * done));
    }
  }
  __device__ __forceinline__ void lit_imm(uint64_t lo, uint64_t hi, uint32_t n) {
    // n is a literal's length: the branches fold
    if (n >= 8) {
      put<8>(lo);
      p += 8;
      lo = hi;
      n -= 8;
    }
    switch (n) {
      case 8: put<8>(lo); break;
      case 7: put<7>(lo); break;
      case 6: put<6>(lo); break;
      case 5: put<5>(lo); break;
      case 4: put<4>(lo); break;
      case 3: put<3>(lo); break;
      case 2: put<2>(lo); break;
      case 1: put<1>(lo); break;
      default: break;
    }
    p += n;
  }
  static __device__ __forceinline__ uint64_t at_for_blank(uint64_t x) {
    const uint64_t z = bytes_eq(x, (uint8_t)' ');  // ' ' 0x20 -> '@' 0x40
    return x ^ ((z >> 1) | (z >> 2));
  }
  // TWICE: the same bytes also go to p + dist (the SAM line prints the quality string twice)
  template <bool NAME, bool TWICE = false>
  __device__ __forceinline__ void copy(const uint8_t* s, uint32_t n, uint32_t dist = 0) {
    auto st8 = [&](uint32_t at, uint64_t v) {
      if (NAME) v = at_for_blank(v);
      __builtin_memcpy(p + at, &v, 8);
      if (TWICE) __builtin_memcpy(p + dist + at, &v, 8);
    };
    if (n >= 8) {
      uint32_t i = 0;
      // (the wavefront waits for every LDS round trip: four reads are in flight per trip while the piece is long)
      for (; i + 32 <= n; i += 32) {
        const uint64_t a = ld8(s + i), b = ld8(s + i + 8), c = ld8(s + i + 16), d = ld8(s + i + 24);
        st8(i, a);
        st8(i + 8, b);
        st8(i + 16, c);
        st8(i + 24, d);
      }
      if (i + 16 <= n) {
        const uint64_t a = ld8(s + i), b = ld8(s + i + 8);
        st8(i, a);
        st8(i + 8, b);
        i += 16;
      }
      if (i + 8 <= n) {
        st8(i, ld8(s + i));
        i += 8;
      }
      if (i < n) st8(n - 8, ld8(s + n - 8));  // the last 8 bytes again: they overlap what is already there with the same values
    } else if (n) {
      uint64_t a = ld8(s);  // the sources have 8 bytes of slack
      if (NAME) a = at_for_blank(a);
#pragma unroll
      for (int rep = 0; rep < (TWICE ? 2 : 1); ++rep) {
        uint8_t* q = p + (rep ? dist : 0u);
        uint32_t done = 0;
        if (n & 4) {
          const uint32_t w = (uint32_t)a;
          __builtin_memcpy(q, &w, 4);
          done = 4;
        }
        if (n & 2) {
          const uint16_t w = (uint16_t)(a >> (8 * done));
          __builtin_memcpy(q + done, &w, 2);
          done += 2;
        }
        if (n & 1) q[done] = (uint8_t)(a >> (8 * done));
      }
    }
    p += n;
  }
  __device__ __forceinline__ void bytes_twice(const uint8_t* s, uint32_t n, uint32_t dist) { copy<false, true>(s, n, dist); }
  __device__ __forceinline__ void skip(uint32_t n) { p += n; }
  __device__ __forceinline__ void bytes(const uint8_t* s, uint32_t n) { copy<false>(s, n); }
  __device__ __forceinline__ void name(const uint8_t* s, uint32_t n) { copy<true>(s, n); }
  __device__ __forceinline__ void ch(char c) {
    p[0] = (uint8_t)c;
    p += 1;
  }
  __device__ __forceinline__ void dec(unsigned long v) {
    const uint32_t d = dec_digits(v);
    if (!(v >> 32)) {
      uint32_t x = (uint32_t)v;
      for (uint32_t i = 0; i < d; ++i) {
        const uint32_t q = x / 10u;
        p[d - 1 - i] = (uint8_t)('0' + (x - q * 10u));
        x = q;
      }
    } else {
      for (uint32_t i = 0; i < d; ++i) {
        p[d - 1 - i] = (uint8_t)('0' + v % 10);
        v /= 10;
      }
    }
    p += d;
  }
};

template <class W>
__device__ __forceinline__ void bc_put_cut(W& w, const uint8_t* s, const Cut& c) {
  w.bytes(s + c.from, c.n);
  if (c.add_nl) w.ch('\n');
}

// the FASTQ record of one file (src/fastq_pre_barcodes.c:713-718)
template <class W>
__device__ __forceinline__ void bc_emit_fastq(bool sliced, long off, long size, const BcLine (&ln)[4], const BcTags& t, W& w) {
  const bool tagged = (t.n[0] | t.n[1] | t.n[2]) != 0;
  // add_tags2readname (src/fastq_pre_barcodes.c:192-216) moves the header up by the tags' length inside hdr1[1000] -
  // and, when the tagged header has 1000 characters or more (a header line near the gzgets limit, or a piece of a longer
  // one), on into hdr2[], the next member of the struct (src/fastq.h:98-101), whose bytes [1] and [2] are then set to
  // '\n' and 0: what is printed as hdr1 runs through hdr2[0] and ends with that '\n', what is printed as hdr2 is the
  // header's character number 1000 and the '\n' (exactly 1000 characters: the string's 0 lands in hdr2[0] - hdr2 is empty)
  const uint32_t tags_n = 31u + t.n[0] + t.n[1] + t.n[2];
  const uint32_t hn = ln[0].len + ln[0].nl + (tagged ? tags_n : 0u);
  const bool spills = tagged && hn >= (uint32_t)FQG_MAX_LABEL_LENGTH;
  if (tagged) {
    w.ch((char)ln[0].p[0]);
    BC_LIT(w, "STAGS_CELL=");
    w.bytes(t.s[1], t.n[1]);
    BC_LIT(w, "_UMI=");
    w.bytes(t.s[0], t.n[0]);
    BC_LIT(w, "_SAMPLE=");
    w.bytes(t.s[2], t.n[2]);
    BC_LIT(w, "_ETAGS_");
    const uint32_t rest = ln[0].len + ln[0].nl - 1;
    if (spills && hn > (uint32_t)FQG_MAX_LABEL_LENGTH) {
      w.bytes(ln[0].p + 1, (uint32_t)FQG_MAX_LABEL_LENGTH - tags_n);  // ... up to character number 1000 of the tagged header
      w.ch('\n');
    } else w.bytes(ln[0].p + 1, rest);
  } else {
    w.bytes(ln[0].p, ln[0].len + ln[0].nl);
  }
  if (sliced) bc_put_cut(w, ln[1].p, bc_cut(ln[1].len + ln[1].nl, off, size));
  else w.bytes(ln[1].p, ln[1].len + ln[1].nl);
  if (spills) {
    if (hn > (uint32_t)FQG_MAX_LABEL_LENGTH) {
      w.ch((char)ln[0].p[(uint32_t)FQG_MAX_LABEL_LENGTH - tags_n]);
      w.ch('\n');
    }
  } else if (tagged || sliced) {
    w.ch((char)ln[2].p[0]);
    w.ch('\n');
  } else {
    w.bytes(ln[2].p, ln[2].len + ln[2].nl);
  }
  if (sliced) bc_put_cut(w, ln[3].p, bc_cut(ln[3].len + ln[3].nl, off, size));
  else w.bytes(ln[3].p, ln[3].len + ln[3].nl);
}

// one SAM line (src/fastq_pre_barcodes.c:666-711)
template <class W>
__device__ __forceinline__ void bc_emit_sam_line(const BcParams& P, unsigned long number, bool se, bool mate1,
                                                 const BcLine (&ln)[4], const SamGeom& g, const BcTags& t, W& w) {
  w.dec(number);
  w.ch('\t');
  w.dec(bc_sam_flag(se, mate1));
  BC_LIT(w, "\t*\t0\t255\t*\t*\t0\t");
  w.dec(g.shown);
  w.ch('\t');
  w.bytes(ln[1].p + g.cs.from, g.seq_n);
  w.ch('\t');
  w.bytes_twice(ln[3].p + g.cq.from, g.qual_n, g.qual_n + 6 + g.name_n + 6);  // the QUAL column and the op:Z: value
  BC_LIT(w, "\ton:Z:");
  w.name(ln[0].p + 1, g.name_n);
  BC_LIT(w, "\top:Z:");
  w.skip(g.qual_n);
  if (t.n[0]) {
    if (P.tenx) BC_LIT(w, "\tUB:Z:"); else BC_LIT(w, "\tRX:Z:");
    w.bytes(t.s[0], t.n[0]);
    if (P.tenx) BC_LIT(w, "\tUY:Z:"); else BC_LIT(w, "\tQX:Z:");
    w.bytes(t.q[0], t.qn[0]);
  }
  if (t.n[1]) {
    w.ch(mate1 ? '\t' : ' ');  // the second mate gets a blank (src/fastq_pre_barcodes.c:705)
    BC_LIT(w, "CR:Z:");
    w.bytes(t.s[1], t.n[1]);
    BC_LIT(w, "\tCY:Z:");
    w.bytes(t.q[1], t.qn[1]);
  }
  if (t.n[2]) {
    BC_LIT(w, "\tBC:Z:");
    w.bytes(t.s[2], t.n[2]);
    BC_LIT(w, "\tQT:Z:");
    w.bytes(t.q[2], t.qn[2]);
  }
  w.ch('\n');
}

// ---- the alignment record of a SAM line (bc_bam_record_len) ----
// bam_nt16_table (bam_import.c:17-34) computed: '=' 0, A C M G R S V T W Y H K D B N (either case) 1..15 in that
// order of values, '0'..'3' 1 2 4 8, everything else 15.  Two 64-bit constants hold the nibbles of 0x40..0x5f (the
// letters by c & 31; the other columns of the table are 15), one those of 0x30..0x3f.
__device__ __forceinline__ uint32_t bc_nt16(uint32_t c) {
  //                               O N M L K J I H G F E D C B A @        _ ^ ] \ [ Z Y X W V U T S R Q P
  constexpr uint64_t let_lo = 0xFF3FCFFB4FFD2E1Full, let_hi = 0xFFFFFFAF97F865FFull;
  //                               ? > = < ; : 9 8 7 6 5 4 3 2 1 0
  constexpr uint64_t dig = 0xFF0FFFFFFFFF8421ull;
  // (32-bit halves, chosen by bit 3: a 64-bit select and shift per base cost the emit kernel registers it does not have)
  const bool up = (c & 8u) != 0;
  const uint32_t l0 = up ? (uint32_t)(let_lo >> 32) : (uint32_t)let_lo, l1 = up ? (uint32_t)(let_hi >> 32) : (uint32_t)let_hi;
  const uint32_t d = up ? (uint32_t)(dig >> 32) : (uint32_t)dig;
  const uint32_t half = (c & 0x40u) ? ((c & 0x10u) ? l1 : l0) : ((c & 0xF0u) == 0x30u ? d : ~0u);
  return (c & 0x80u) ? 15u : (half >> (4u * (c & 7u))) & 15u;
}
// 0x80 in every byte of x that libbam would cut the line at (9..13: isspace() but the blank) or, HI, that is >= 0x80.
// (In 32-bit halves: their constants are literals of the instructions; 64-bit ones are registers held across the
// kernel's loop, which has none to spare.)
template <bool HI>
__device__ __forceinline__ uint32_t bc_bam_bad4(uint32_t x) {
  const uint32_t lo7 = x & 0x7F7F7F7Fu;
  const uint32_t ge9 = lo7 + 0x77777777u, ge14 = lo7 + 0x72727272u;  // bit 7: the low 7 bits are >= 9 / >= 14
  const uint32_t sp = ge9 & ~ge14 & ~x & 0x80808080u;
  return HI ? sp | (x & 0x80808080u) : sp;
}
template <bool HI>
__device__ __forceinline__ uint32_t bc_bam_bad_bytes(uint64_t x) {
  return bc_bam_bad4<HI>((uint32_t)x) | bc_bam_bad4<HI>((uint32_t)(x >> 32));
}
__device__ __forceinline__ uint64_t bc_low_bytes(uint64_t x, uint32_t n) {  // the low n bytes, n = 1..7
  return x & ((1ull << (8u * n)) - 1ull);
}
// x - 33 in every byte (no borrow between bytes)
__device__ __forceinline__ uint32_t bc_minus33_4(uint32_t x) {
  return ((x | 0x80808080u) - 0x21212121u) ^ ((x ^ ~0x21212121u) & 0x80808080u);
}
__device__ __forceinline__ uint64_t bc_minus33(uint64_t x) {
  return (uint64_t)bc_minus33_4((uint32_t)x) | ((uint64_t)bc_minus33_4((uint32_t)(x >> 32)) << 32);
}
// the bases of 8 bytes (the first r of them: the rest give zero nibbles) -> 4 bytes, high nibble first
__device__ __forceinline__ uint32_t bc_pack8(uint64_t v, uint32_t r) {
  uint32_t out = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t nib = j < r ? bc_nt16((uint32_t)(v >> (8 * j)) & 0xFFu) : 0u;
    out |= nib << (8 * (j >> 1) + ((j & 1) ? 0 : 4));
  }
  return out;
}

// 0xffffffff made where it is stored: as a constant it is lifted out of the emit kernel's loop over the tiles into
// registers of its own (three of them, and a fourth pair for the fill), which that loop does not have
__device__ __forceinline__ uint32_t bc_minus_one() {
  uint32_t v = 0xFFFFFFFFu;
  asm volatile("" : "+v"(v));
  return v;
}

// One lane writes one record in LDS (k_bc_emit_tile).  bad: a byte that refuses the record was seen.
struct BamLaneWriter : LaneWriter {
  uint32_t bad = 0;
  __device__ __forceinline__ void see(uint32_t marks) { bad |= marks; }
  __device__ __forceinline__ void le32(uint32_t v) {
    __builtin_memcpy(p, &v, 4);
    p += 4;
  }
  // the low n (1..7) bytes of a at q
  static __device__ __forceinline__ void put_low(uint8_t* q, uint64_t a, uint32_t n) {
    uint32_t done = 0;
    if (n & 4) {
      const uint32_t w = (uint32_t)a;
      __builtin_memcpy(q, &w, 4);
      done = 4;
    }
    if (n & 2) {
      const uint16_t w = (uint16_t)(a >> (8 * done));
      __builtin_memcpy(q + done, &w, 2);
      done += 2;
    }
    if (n & 1) q[done] = (uint8_t)(a >> (8 * done));
  }
  // LaneWriter::copy with the test for the bytes that refuse the record.  QUAL: p gets the bytes minus 33 (FILL: 0xff
  // over n33 bytes instead), p + dist the bytes themselves (the op:Z: value)
  template <bool NAME, bool QUAL>
  __device__ __forceinline__ void checked(const uint8_t* s, uint32_t n, uint32_t dist = 0) {
    auto st8 = [&](uint32_t at, uint64_t v) {
      see(bc_bam_bad_bytes<false>(v));
      if (NAME) v = at_for_blank(v);
      if (QUAL) {
        __builtin_memcpy(p + dist + at, &v, 8);
        v = bc_minus33(v);
      }
      __builtin_memcpy(p + at, &v, 8);
    };
    if (n >= 8) {
      uint32_t i = 0;
      // (two reads in flight per LDS round trip, where LaneWriter::copy has four)
      for (; i + 16 <= n; i += 16) {
        const uint64_t a = ld8(s + i), b = ld8(s + i + 8);
        st8(i, a);
        st8(i + 8, b);
      }
      if (i + 8 <= n) {
        st8(i, ld8(s + i));
        i += 8;
      }
      if (i < n) st8(n - 8, ld8(s + n - 8));
    } else if (n) {
      uint64_t a = bc_low_bytes(ld8(s), n);  // the sources have 8 bytes of slack
      see(bc_bam_bad_bytes<false>(a));
      if (NAME) a = at_for_blank(a);
      if (QUAL) {
        put_low(p + dist, a, n);
        a = bc_minus33(a);
      }
      put_low(p, a, n);
    }
    p += n;
  }
  __device__ __forceinline__ void bytes(const uint8_t* s, uint32_t n) { checked<false, false>(s, n); }
  __device__ __forceinline__ void name(const uint8_t* s, uint32_t n) { checked<true, false>(s, n); }
  // the quality values and, dist bytes on, the op:Z: value; fill: n_seq times 0xff instead of the values (QUAL is "*",
  // or a refused record whose QUAL has another length than its SEQ).  What lies behind the values is written later.
  __device__ __forceinline__ void quals(const uint8_t* s, uint32_t n, uint32_t n_seq, bool fill, uint32_t dist) {
    if (!fill) {
      checked<false, true>(s, n, dist);
      return;
    }
    uint8_t* const q = p;
    p += dist;
    checked<false, false>(s, n);
    p = q;
    const uint64_t ff = ((uint64_t)bc_minus_one() << 32) | bc_minus_one();
    for (uint32_t i = 0; i < n_seq; i += 8) __builtin_memcpy(p + i, &ff, 8);  // (up to 7 bytes into the aux fields: rewritten below)
    p += n_seq;
  }
  // the bases at four bits each; the last word may run up to 3 bytes into the quality values, which are written next
  __device__ __forceinline__ void bases(const uint8_t* s, uint32_t n) {
    for (uint32_t i = 0; i < n; i += 8) {
      const uint32_t r = n - i < 8u ? n - i : 8u;
      uint64_t v = ld8(s + i);
      if (r < 8) v = bc_low_bytes(v, r);
      see(bc_bam_bad_bytes<true>(v));
      const uint32_t w = bc_pack8(v, r);
      __builtin_memcpy(p + (i >> 1), &w, 4);
    }
    p += (n + 1) >> 1;
  }
  __device__ __forceinline__ bool refused() const { return bad != 0; }
};

// The whole wavefront writes one record to the output image (k_bc_emit_direct), lane i byte i of every piece.
struct BamWriter : Writer {
  uint32_t bad = 0;  // per lane
  static __device__ __forceinline__ uint32_t cuts(uint8_t c) { return c >= 9 && c <= 13 ? 1u : 0u; }
  __device__ __forceinline__ void le32(uint32_t v) {
    if (lane < 4) p[lane] = (uint8_t)(v >> (8 * lane));
    p += 4;
  }
  __device__ __forceinline__ void bytes(const uint8_t* s, uint32_t n) {
    for (uint32_t i = lane; i < n; i += kWave) {
      bad |= cuts(s[i]);
      p[i] = s[i];
    }
    p += n;
  }
  __device__ __forceinline__ void name(const uint8_t* s, uint32_t n) {
    for (uint32_t i = lane; i < n; i += kWave) {
      bad |= cuts(s[i]);
      p[i] = s[i] == ' ' ? (uint8_t)'@' : s[i];
    }
    p += n;
  }
  __device__ __forceinline__ void quals(const uint8_t* s, uint32_t n, uint32_t n_seq, bool fill, uint32_t dist) {
    for (uint32_t i = lane; i < n; i += kWave) {
      bad |= cuts(s[i]);
      p[dist + i] = s[i];
    }
    for (uint32_t i = lane; i < n_seq; i += kWave) p[i] = fill ? (uint8_t)0xff : (uint8_t)(s[i] - 33);
    p += n_seq;
  }
  __device__ __forceinline__ void bases(const uint8_t* s, uint32_t n) {
    const uint32_t nb = (n + 1) >> 1;
    for (uint32_t i = lane; i < nb; i += kWave) {
      const uint8_t a = s[2 * i], b = 2 * i + 1 < n ? s[2 * i + 1] : (uint8_t)0;
      bad |= cuts(a) | cuts(b) | ((a | b) >> 7);
      p[i] = (uint8_t)((bc_nt16(a) << 4) | (2 * i + 1 < n ? bc_nt16(b) : 0u));
    }
    p += nb;
  }
  __device__ __forceinline__ bool refused() const { return bad != 0; }
};

// one alignment record: the SAM line of bc_emit_sam_line as libbam reads it.  rec_bytes = bc_bam_record_len.
template <class W>
__device__ __forceinline__ void bc_emit_bam_record(const BcParams& P, unsigned long number, bool se, bool mate1,
                                                   const BcLine (&ln)[4], const SamGeom& g, const BcTags& t, uint32_t rec_bytes,
                                                   W& w) {
  const uint32_t l_seq = g.seq_n;
  const uint32_t none = bc_minus_one();
  w.le32(rec_bytes - 4);                                  // block_size
  w.le32(none);                                           // refID "*"
  w.le32(none);                                           // pos "0" - 1
  w.le32((4680u << 16) | (255u << 8) | (dec_digits(number) + 1));  // bin = reg2bin(-1, 0), mapq, l_read_name
  w.le32(bc_sam_flag(se, mate1) << 16);                   // flag, no CIGAR
  w.le32(l_seq);
  w.le32(none);                                           // next_refID "*"
  w.le32(none);                                           // next_pos "0" - 1
  w.le32(g.shown);                                        // tlen: column 9
  w.dec(number);
  w.ch('\0');
  const uint8_t* const seq = ln[1].p + g.cs.from;
  const uint8_t* const qual = ln[3].p + g.cq.from;
  // the characters that decide by themselves (one byte each; empty fields are the plan's finding, nothing is read of them)
  const bool seq_star = l_seq == 1 && seq[0] == '*';  // libbam: no sequence at all - and then a QUAL that is not "*" aborts
  const bool qual_star = g.qual_n == 1 && qual[0] == '*';
  const bool glue = !mate1 && t.n[1];  // " CR:Z:<cell>" ends the value of the field in front of it
  w.bases(seq, l_seq);
  w.quals(qual, g.qual_n, l_seq, qual_star || g.qual_n != l_seq, l_seq + 3 + g.name_n + 1 + 3);
  if (seq_star || (!qual_star && g.qual_n != l_seq)) w.bad |= 1;
  BC_LIT(w, "onZ");
  w.name(ln[0].p + 1, g.name_n);
  w.ch('\0');
  BC_LIT(w, "opZ");
  w.skip(g.qual_n);
  if (t.n[0]) {
    w.ch('\0');
    if (P.tenx) BC_LIT(w, "UBZ"); else BC_LIT(w, "RXZ");
    w.bytes(t.s[0], t.n[0]);
    w.ch('\0');
    if (P.tenx) BC_LIT(w, "UYZ"); else BC_LIT(w, "QXZ");
    w.bytes(t.q[0], t.qn[0]);
  }
  if (t.n[1]) {
    if (glue) BC_LIT(w, " CR:Z:");
    else {
      w.ch('\0');
      BC_LIT(w, "CRZ");
    }
    w.bytes(t.s[1], t.n[1]);
    w.ch('\0');
    BC_LIT(w, "CYZ");
    w.bytes(t.q[1], t.qn[1]);
  }
  if (t.n[2]) {
    w.ch('\0');
    BC_LIT(w, "BCZ");
    w.bytes(t.s[2], t.n[2]);
    w.ch('\0');
    BC_LIT(w, "QTZ");
    w.bytes(t.q[2], t.qn[2]);
  }
  w.ch('\0');
}

struct EmitOut {
  const uint32_t* len;
  const unsigned long long* off;
  const unsigned long long* sum;
  uint8_t* out;
};

// One wavefront per tile.  SAM lines and BAM records: one lane per line / record (two per iteration for paired
// reads); FASTQ: one lane per record, one output after the other.
enum : int { kEmitFastq = 0, kEmitSam = FQG_OUT_SAM, kEmitBam = FQG_OUT_BAM };
// (READ1 alone: the SAM kernel comes out at three wavefronts per SIMD unasked; its BAM twin is held to as many)
template <int KIND, int MASK>
__global__ __launch_bounds__(kWave, KIND == kEmitBam && MASK == 0x02 ? 3 : 2) void k_bc_emit_tile(BcParams P, BcTile tc, uint64_t n_done,
                                                        const uint8_t* __restrict__ status,
                                                        const uint8_t* __restrict__ tile_big, EmitOut o0, EmitOut o1,
                                                        EmitOut o2, BcCall* __restrict__ call) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_lds[];
  uint8_t* s_in = s_lds;
  uint8_t* s_out = s_lds + tc.in_cap;
  const int lane = (int)threadIdx.x;
  constexpr bool SAM = KIND != kEmitFastq;  // (one lane per line: the layout of both)
  const bool se = !bc_has<MASK>(P, 2);
  const uint32_t lpi = SAM && !se ? 2u : 1u;  // lanes per iteration
  const uint32_t it_raw = lpi == 2 ? (uint32_t)lane >> 1 : (uint32_t)lane;
  const bool mate1 = lpi == 2 ? !(lane & 1) : true;
  const uint64_t n_tiles = (n_done + tc.T - 1) / tc.T;
  auto tile_size = [&](uint64_t tile) {
    const uint64_t left = n_done - tile * tc.T;
    return (uint32_t)(left < (uint64_t)tc.T ? left : (uint64_t)tc.T);
  };
  auto geo_of = [&](uint64_t tile, TileGeo& tg) {
    const uint32_t Tn = tile_size(tile);
    const uint64_t k = tile * tc.T + (it_raw < Tn ? it_raw : Tn - 1);
    tg.big = tile_big[tile];
    tg.st = status[k];
#pragma unroll
    for (int x = 1; x < kBcFiles; ++x)
      if (bc_has<MASK>(P, x)) bc_geo_load(P.f[x], k, tg.f[x]);
    if (SAM) {
      tg.off[0] = o0.off[k], tg.sum[0] = o0.sum[k / kScan64Span], tg.olen[0] = o0.len[k];
    } else {
      if (P.emit[1]) tg.off[1] = o1.off[k], tg.sum[1] = o1.sum[k / kScan64Span], tg.olen[1] = o1.len[k];
      if (P.emit[2]) tg.off[2] = o2.off[k], tg.sum[2] = o2.sum[k / kScan64Span], tg.olen[2] = o2.len[k];
    }
  };
  // tile_walk (fqg_fastq_tile.h) written out - a change of the order is made in both places: the fifteen instantiations sit
  // at the edge of their registers, and through the template five came out with scratch memory or a spilled register.
  // (MASK 0 has no registers for three tiles under way: it copies a tile's spans when it gets there.)
  constexpr bool kAhead = MASK != 0;
  const uint64_t stride = gridDim.x;
  auto clamp_tile = [&](uint64_t t) { return t < n_tiles ? t : n_tiles - 1; };
  auto last_lane_of = [&](uint64_t t) { return (int)((tile_size(t) - 1) * lpi); };
  TileGeo cur, nxt, nx2;
  bc_u32x4 pf[kSpanPf];
  if (blockIdx.x < n_tiles) {
    geo_of(blockIdx.x, cur);
    if (kAhead) {
      geo_of(clamp_tile(blockIdx.x + stride), nxt);
      SpanPlan sp;
      bc_span_plan<false, MASK>(P, cur, last_lane_of(blockIdx.x), tc.in_cap, sp);
      span_fetch(sp, lane, pf);
    }
  }
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += stride, cur = kAhead ? nxt : nx2, nxt = nx2) {
    const uint64_t k0 = tile * tc.T;
    const uint32_t Tn = tile_size(tile);
    const bool valid = it_raw < Tn;
    const uint64_t k = k0 + (valid ? it_raw : Tn - 1);
    const bool big = __builtin_amdgcn_readfirstlane((int)cur.big) != 0;
    BcLine L[kBcFiles][4];
    {
      SpanPlan sp;
      bc_span_plan<false, MASK>(P, cur, last_lane_of(tile), tc.in_cap, sp);
      if (!big) {  // (fits: the plan checked)
        if (P.ablate & 8) {
        } else if (kAhead) span_land(sp, lane, pf, s_in);
        else span_copy(sp, 0, lane, s_in);
      }
      bc_span_lines<false, MASK>(P, cur, sp, s_in, L);
    }
    if (kAhead) {
      const uint64_t tn = clamp_tile(tile + stride);
      SpanPlan sp;
      bc_span_plan<false, MASK>(P, nxt, last_lane_of(tn), tc.in_cap, sp);
      span_fetch(sp, lane, pf);
    }
    geo_of(clamp_tile(tile + (kAhead ? 2 : 1) * stride), nx2);
    if (big) continue;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the name checks of every iteration, kept or not (the reference makes them first, src/fastq_pre_barcodes.c:606-635)
    if (!(P.ablate & 4)) bc_report_finding(call, valid && mate1, k, valid && mate1 ? bc_check_names<true, MASK>(P, L) : 0u);
    const bool keep = valid && cur.st == kBcKeep;
    BcTags t;
    bc_tags_of_kept<MASK>(P, L, &t);
    if (SAM) {
      BcLine own[4];
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        own[l].p = mate1 ? L[1][l].p : L[2][l].p;
        own[l].len = mate1 ? L[1][l].len : L[2][l].len;
        own[l].nl = mate1 ? L[1][l].nl : L[2][l].nl;
      }
      const bool sliced = mate1 ? bc_slices(P, 1) : bc_slices(P, 2);
      const SamGeom g = bc_sam_geom(sliced, mate1 ? P.read_off[1] : P.read_off[2], mate1 ? P.read_size[1] : P.read_size[2],
                                    mate1, own);
      const unsigned long number = P.first_read_number + k + 1;
      // (single-end: the line's length is what the plan computed for the iteration; two mates share that number)
      const uint32_t my_len = !keep ? 0u
                              : (lpi == 1 ? cur.olen[0]
                                          : (KIND == kEmitBam ? bc_bam_record_len(number, mate1, g, t)
                                                              : bc_sam_line_len(number, bc_sam_flag(se, mate1), g, t)));
      const uint32_t before = __shfl_up(my_len, 1, 64);  // (a second mate: behind the first, whose place it shares)
      const TileImage im = tile_image(o0.out, cur.off[0] + cur.sum[0], my_len, mate1 ? 0u : before);
      if constexpr (KIND == kEmitBam) {
        BamLaneWriter w;
        w.p = s_out + im.skew + im.start;
        if (keep) bc_emit_bam_record(P, number, se, mate1, own, g, t, my_len, w);
        // a byte that refuses the record (what its geometry says against it: the plan)
        bc_report_finding(call, keep, k, keep && w.refused() ? (kBcFindBam << 3) | (mate1 ? 1u : 2u) : 0u);
      } else if (keep && !(P.ablate & 1)) {
        LaneWriter w{s_out + im.skew + im.start};
        bc_emit_sam_line(P, number, se, mate1, own, g, t, w);
      }
      tile_image_flush(im, s_out, lane, !(P.ablate & 2));
    } else {
#pragma unroll
      for (int which = 1; which <= 2; ++which) {
        if (!P.emit[which]) continue;
        const EmitOut& o = which == 1 ? o1 : o2;
        const bool sliced = bc_slices(P, which);
        const uint32_t my_len = keep ? cur.olen[which] : 0u;
        const TileImage im = tile_image(o.out, cur.off[which] + cur.sum[which], my_len);
        if (keep) {
          LaneWriter w{s_out + im.skew + im.start};
          bc_emit_fastq(sliced, P.read_off[which], P.read_size[which], L[which], t, w);
        }
        tile_image_flush(im, s_out, lane);
      }
    }
  }
}

// iterations of the tiles that do not fit LDS (long reads): one wavefront per iteration, records read
// from the images, text written straight to the output image
template <bool BAM>
__global__ __launch_bounds__(kBlock) void k_bc_emit_direct(BcParams P, BcTile tc, uint64_t n_done,
                                                           const uint8_t* __restrict__ status,
                                                           const uint8_t* __restrict__ tile_big, EmitOut o0, EmitOut o1,
                                                           EmitOut o2, BcCall* __restrict__ call) {
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const int lane = (int)(threadIdx.x & 63), wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool se = !P.f[2].present;
  for (uint64_t k = (uint64_t)blockIdx.x * (kBlock / kWave) + wv; k < n_done; k += n_waves) {
    if (!tile_big[k / tc.T]) continue;
    BcLine L[kBcFiles][4];
    bc_lines_all(P, k, L);
    {  // the name checks (every lane the same bytes, from the images)
      const uint32_t finding = bc_check_names<false>(P, L);
      if (finding && lane == 0) atomicMin(&call->first_finding, (unsigned long long)((k << 8) | finding));
    }
    if (status[k] != kBcKeep) continue;
    BcTags t;
    bc_tags_of_kept(P, L, &t);
    if constexpr (BAM) {
      BamWriter w;
      w.p = o0.out + o0.off[k] + o0.sum[k / kScan64Span];
      w.lane = lane;
      const unsigned long number = P.first_read_number + k + 1;
      const SamGeom g1 = bc_sam_geom(bc_slices(P, 1), P.read_off[1], P.read_size[1], true, L[1]);
      bc_emit_bam_record(P, number, se, true, L[1], g1, t, bc_bam_record_len(number, true, g1, t), w);
      uint32_t finding = __ballot(w.refused()) ? (kBcFindBam << 3) | 1u : 0u;
      if (!se) {
        const SamGeom g2 = bc_sam_geom(bc_slices(P, 2), P.read_off[2], P.read_size[2], false, L[2]);
        w.bad = 0;
        bc_emit_bam_record(P, number, se, false, L[2], g2, t, bc_bam_record_len(number, false, g2, t), w);
        if (!finding && __ballot(w.refused())) finding = (kBcFindBam << 3) | 2u;
      }
      if (finding && lane == 0) atomicMin(&call->first_finding, (unsigned long long)((k << 8) | finding));
    } else if (P.out_sam) {
      Writer w{o0.out + o0.off[k] + o0.sum[k / kScan64Span], lane};
      bc_emit_sam_line(P, P.first_read_number + k + 1, se, true, L[1],
                       bc_sam_geom(bc_slices(P, 1), P.read_off[1], P.read_size[1], true, L[1]), t, w);
      if (!se)
        bc_emit_sam_line(P, P.first_read_number + k + 1, se, false, L[2],
                         bc_sam_geom(bc_slices(P, 2), P.read_off[2], P.read_size[2], false, L[2]), t, w);
    } else {
      if (P.emit[1]) {
        Writer w{o1.out + o1.off[k] + o1.sum[k / kScan64Span], lane};
        bc_emit_fastq(bc_slices(P, 1), P.read_off[1], P.read_size[1], L[1], t, w);
      }
      if (P.emit[2]) {
        Writer w{o2.out + o2.off[k] + o2.sum[k / kScan64Span], lane};
        bc_emit_fastq(bc_slices(P, 2), P.read_off[2], P.read_size[2], L[2], t, w);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// whitelist membership of a barcode cut out of the reads (BASELINE configs[2]: "known_cells whitelist"): the cell
// barcode that fastq_pre_barcodes puts into the read name is what bam_umi_count later packs with char2uint_64
// (src/bam_umi_count.c:364-382: base 10, A C G T N -> 1..5, from the END of the string, stopping at the first other
// character) and looks up with valid_barcode (:523-535) in the table load_whitelist (:543-579) filled.  One thread
// per record: the `size` characters at `offset` of the sequence line (get_barcode's bounds, src/fastq_pre_barcodes.c:232:
// a read too short for them has no barcode), packed in registers, looked up in a small open-addressing set that the
// L2 keeps (ten thousand entries).
// ------------------------------------------------------------------------------------------
struct WlSlot {
  unsigned long long key, used;
};
struct WlCall {
  unsigned long long n_valid, n_short;
};
__host__ __device__ inline uint64_t wl_hash(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
constexpr int kWlMaxSize = 56;  // barcode characters (the reference's arrays hold 49)

// char2uint_64's digit of a character: A C G T N (either case - & 0xDF folds it) -> 1..5, every other character 0
__device__ __forceinline__ uint32_t wl_base(uint32_t c) {
  const uint32_t u = c & 0xDFu;
  return u == 'A' ? 1u : u == 'C' ? 2u : u == 'G' ? 3u : u == 'T' ? 4u : u == 'N' ? 5u : 0u;
}
// The `size` characters at byte `at` of the image, packed; *stopped: a character that is no base ended the value early.
// Whole words while they lie inside the image; the last bytes of an image one by one.
template <int WORDS>  // 8-byte words that hold the barcode
__device__ __forceinline__ uint64_t wl_pack_at(const FrameView& f, uint64_t at, uint32_t size, bool* stopped) {
  const uint8_t* p = f.img + at;
  uint64_t w[WORDS];
#pragma unroll
  for (int i = 0; i < WORDS; ++i) {
    w[i] = 0;
    if (8u * i < size) {
      if (at + 8u * i + 8u <= f.nbytes) __builtin_memcpy(&w[i], p + 8 * i, 8);
      else
        for (uint32_t q = 0; q < 8 && 8u * i + q < size; ++q) w[i] |= (uint64_t)p[8 * i + q] << (8 * q);
    }
  }
  uint64_t v = 0;
  bool stop = false;
#pragma unroll
  for (int pos = 8 * WORDS - 1; pos >= 0; --pos) {
    const uint32_t base = wl_base((uint32_t)(w[pos >> 3] >> (8 * (pos & 7))));
    if ((uint32_t)pos < size && !stop) {
      if (!base) stop = true;
      else v = v * 10 + base;
    }
  }
  *stopped = stop;
  return v;
}
__device__ __forceinline__ bool wl_member(const WlSlot* __restrict__ set, uint64_t mask, uint64_t v) {
  for (uint64_t at = wl_hash(v) & mask;; at = (at + 1) & mask) {  // (load <= 1/4: an empty slot ends every chain)
    const WlSlot s = set[at];
    if (!s.used) return false;
    if (s.key == v) return true;
  }
}

template <int WORDS>
__global__ __launch_bounds__(kBlock) void k_bc_whitelist(FrameView f, uint64_t first, uint64_t step, uint64_t n, uint32_t offset,
                                                         uint32_t size, const WlSlot* __restrict__ set, uint64_t mask,
                                                         uint8_t* __restrict__ valid, WlCall* __restrict__ call) {
  unsigned long long n_valid = 0, n_short = 0;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
    const uint64_t r = first + k * step;
    const uint64_t b = f.line_end[4 * r] + 1, e = f.line_end[4 * r + 1];  // the sequence line
    bool ok = false;
    if ((uint64_t)offset + size > e - b) ++n_short;  // (offset + size > read_len - 1, read_len = strlen(seq) with its '\n')
    else {
      bool stopped;
      ok = wl_member(set, mask, wl_pack_at<WORDS>(f, b + offset, size, &stopped));
    }
    if (valid) valid[k] = ok ? 1 : 0;
    n_valid += ok ? 1 : 0;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    n_valid += __shfl_down(n_valid, d, 64);
    n_short += __shfl_down(n_short, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_valid) atomicAdd(&call->n_valid, n_valid);
    if (n_short) atomicAdd(&call->n_short, n_short);
  }
}

// ------------------------------------------------------------------------------------------
// whitelist rescue (include/fqg.h: fqg_barcodes_whitelist_correct): a barcode that is no member, but has exactly one
// member at Hamming distance 1, becomes that member.  On the packed value a substitution at string position p is one
// decimal digit replaced: v + (o - d) * 10^p, d the digit there and o one of the four other digits of 1..5 (the first
// character of the string is the LAST digit char2uint_64 adds: position p weighs 10^p).  4 * size neighbours - 64 for
// the 16 bases of a 10x cell barcode: one probe per lane of a wavefront.
//
// Phase one is k_bc_whitelist's, lane by lane.  Phase two belongs to the wavefront (wl_rescue_wave): the lanes that
// missed are found by ballot and served one after the other; the served lane's value and length are read by all
// (readlane), lane i takes neighbour i (position i / 4, i & 3 of the other digits) - a second pass for 17..19
// characters - and the number of hits and the one hit come back by ballot, popcount and readlane.  The neighbours of
// one value are distinct values and the table holds every key once: the number of hits is |C|.  A member of another
// length than the barcode has another number of digits than any neighbour (no digit of a neighbour is 0): never a hit.
// ------------------------------------------------------------------------------------------
enum : uint32_t { kWlMiss = 0, kWlExact = 1, kWlRescued = 2, kWlAmbiguous = 3, kWlShort = 4 };  // FQG_WL_*
constexpr int kWlMaxRescueSize = 19;  // digits that cannot wrap in 64 bits
struct WlCorrectCall {
  unsigned long long by_status[5];  // records by kWl* status
};
__device__ const unsigned long long kWlPow10[kWlMaxRescueSize + 1] = {1ull,
                                                                      10ull,
                                                                      100ull,
                                                                      1000ull,
                                                                      10000ull,
                                                                      100000ull,
                                                                      1000000ull,
                                                                      10000000ull,
                                                                      100000000ull,
                                                                      1000000000ull,
                                                                      10000000000ull,
                                                                      100000000000ull,
                                                                      1000000000000ull,
                                                                      10000000000000ull,
                                                                      100000000000000ull,
                                                                      1000000000000000ull,
                                                                      10000000000000000ull,
                                                                      100000000000000000ull,
                                                                      1000000000000000000ull,
                                                                      10000000000000000000ull};

__device__ __forceinline__ uint64_t wl_readlane64(uint64_t v, int src) {  // src: the same in every lane
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}
// the digits of a packed value of n <= 19 characters, 3 bits each, the digit of 10^p at bit 3p
__device__ __forceinline__ uint64_t wl_digits(uint64_t v, uint32_t n) {
  uint64_t dig = 0;
  for (uint32_t p = 0; p < n; ++p) {
    const uint64_t q = v / 10ull;
    dig |= (v - q * 10ull) << (3u * p);
    v = q;
  }
  return dig;
}
// Every lane of the wavefront calls this together (no lane may have left: the probes of one lane's barcode are made by
// all 64).  need: this lane's barcode v of n characters (1..19, all of them bases) is no member.  Returns the lane's
// status (kWlMiss where !need) and, for kWlRescued, the member in *out.
__device__ __forceinline__ uint32_t wl_rescue_wave(const WlSlot* __restrict__ set, uint64_t mask, bool need, uint64_t v, uint32_t n,
                                                   int lane, uint64_t* out) {
  uint32_t st = kWlMiss;
  const uint64_t dig = need ? wl_digits(v, n) : 0ull;
  unsigned long long todo = __ballot(need);
  while (todo) {
    const int src = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
    todo &= todo - 1ull;
    const uint64_t sv = wl_readlane64(v, src), sdig = wl_readlane64(dig, src);
    const uint32_t total = 4u * (uint32_t)__builtin_amdgcn_readlane((int)n, src);
    uint32_t hits = 0;
    uint64_t hit = 0;
    for (uint32_t i0 = 0; i0 < total; i0 += 64u) {  // one pass up to 16 characters, two for 17..19
      const uint32_t i = i0 + (uint32_t)lane;
      bool found = false;
      uint64_t cand = 0;
      if (i < total) {
        const uint32_t p = i >> 2;
        const uint32_t d = (uint32_t)(sdig >> (3u * p)) & 7u;  // 1..5
        const uint32_t o = (d + (i & 3u)) % 5u + 1u;           // the four others
        cand = sv + (uint64_t)(int64_t)((int)o - (int)d) * kWlPow10[p];
        found = wl_member(set, mask, cand);
      }
      const unsigned long long m = __ballot(found);
      hits += (uint32_t)__builtin_popcountll(m);
      if (m) hit = wl_readlane64(cand, __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(m)));
    }
    if (lane == src) {
      st = hits == 1u ? kWlRescued : hits ? kWlAmbiguous : kWlMiss;
      *out = hit;
    }
  }
  return st;
}

// N counters of every lane summed over the workgroup and added to dst[0 .. N).  Shuffle, then one add per WORKGROUP
// and counter: the adds of a launch go to one cache line and are served one after the other (~90 per microsecond).
// One per wavefront and counter, as k_bc_whitelist does it, was most of k_bc_whitelist_correct's time as soon as a
// second counter was not zero (0.50 ms -> 0.87 ms for 8 M reads).
template <int N>
__device__ __forceinline__ void wl_add_counters(unsigned long long (&cnt)[N], unsigned long long* __restrict__ dst) {
  __shared__ unsigned long long s_cnt[kBlock / 64][N];
#pragma unroll
  for (int s = 0; s < N; ++s) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt[s] += __shfl_down(cnt[s], d, 64);
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6][s] = cnt[s];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) sum += s_cnt[w][threadIdx.x];
    if (sum) atomicAdd(&dst[threadIdx.x], sum);
  }
}

template <int WORDS>  // 8-byte words that hold the barcode
__global__ __launch_bounds__(kBlock) void k_bc_whitelist_correct(FrameView f, uint64_t first, uint64_t step, uint64_t n, uint32_t offset,
                                                                 uint32_t size, const WlSlot* __restrict__ set, uint64_t mask,
                                                                 uint32_t max_mismatch, uint8_t* __restrict__ status,
                                                                 unsigned long long* __restrict__ cells,
                                                                 WlCorrectCall* __restrict__ call) {
  unsigned long long cnt[5] = {0, 0, 0, 0, 0};  // by status
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  const int lane = lane_id();
  // (the wavefront stays together: its lanes beyond n idle through the round, they do not leave it)
  for (uint64_t k0 = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); k0 < n; k0 += stride) {
    const uint64_t k = k0 + (uint64_t)lane;
    const bool in = k < n;
    uint32_t st = kWlShort;
    uint64_t v = 0;
    bool stopped = false;
    if (in) {
      const uint64_t r = first + k * step;
      const uint64_t b = f.line_end[4 * r] + 1, e = f.line_end[4 * r + 1];  // the sequence line
      if ((uint64_t)offset + size <= e - b) {
        v = wl_pack_at<WORDS>(f, b + offset, size, &stopped);
        st = wl_member(set, mask, v) ? kWlExact : kWlMiss;
      }
    }
    if (max_mismatch) {  // (the same in every lane; size <= 19 - the host has checked)
      uint64_t to = 0;
      const uint32_t r = wl_rescue_wave(set, mask, in && st == kWlMiss && !stopped, v, size, lane, &to);
      if (r != kWlMiss) {
        st = r;
        v = to;
      }
    }
    if (in) {
      if (status) status[k] = (uint8_t)st;
      if (cells) cells[k] = st == kWlExact || st == kWlRescued ? v : 0ull;
#pragma unroll
      for (int s = 0; s < 5; ++s) cnt[s] += st == (uint32_t)s ? 1ull : 0ull;
    }
  }
  wl_add_counters(cnt, call->by_status);
}

}  // namespace fqg
