// fqg_bam2fastq_kernels.hip - the alignment loop of bam2fastq (reference src/bam2fastq.c:249-355) on gfx950: every
// alignment of a BAM becomes up to four FASTQ records in up to six output streams (_1, _2, _cell, _sample, _umi and
// the single-end file; _R1, _R2, _I1 with a 10x option).  The read's original name and quality come from the aux tags
// `on` / `op` that sh/fastq2bam wrote, the barcodes from CR/CY, RX/QX (UB/UY), BC/QT; a BAM of any other origin gives
// its name, its bases (4 bits -> "=ACMGRSVTWYHKDBN") and its qualities (+33).
//
// Input: the inflated BAM stream and the offset of every alignment (fqg_bam_index_records), as for bam_add_tags, walked
// in the same tiles (the frame: fqg_bam_tile.h):
//   k_b2f_tile<false>  every lane walks the aux area of ITS alignment once in the staged span, decides the routing and
//               writes the bytes its record adds to every stream
//   scan        one 64-bit exclusive prefix per stream, all streams in one launch pair (k_scan64_a / _b)
//   k_b2f_tile<true>   the same tiles again: the lane writes its FASTQ records into the LDS images of the tile's output
//               span of every stream
//   Tiles that do not fit LDS (reads of thousands of bases) read the stream itself, and every lane writes its records
//   straight to the output.
// BGZF, the option table, the messages and the gzip writers are host work (host/bam2fastq.cpp).
#include "fqg_bam_tile.h"

namespace fqg {

constexpr int kB2fStreams = 6;
constexpr uint32_t kB2fMaxSeq = 10000;  // BUF_SIZE, src/bam2fastq.c:40: the reference's seq_buf / qual_buf
constexpr uint32_t kB2fInCap = 16 * 1024, kB2fOutCap = 36 * 1024;  // LDS bytes per wavefront
constexpr unsigned long long kB2fNone = ~0ull;
enum { B2F_R1 = 0, B2F_R2 = 1, B2F_CELL = 2, B2F_SAMPLE = 3, B2F_UMI = 4, B2F_SE = 5, B2F_I1 = 2 };  // FILE_LOC, :41
enum { T_ON = 0, T_OP, T_CR, T_CY, T_RX, T_QX, T_UB, T_UY, T_BC, T_QT, T_COUNT };

struct B2fCall {
  unsigned long long first_finding;            // min (record << 32 | (code & 15) << 28 | aux)
  unsigned long long warn_record;              // first alignment without `on` (not secondary)
  unsigned long long first_record[kB2fStreams];  // first alignment that writes to the stream
};
struct B2fTiles : BamTiles {
  int32_t tenx, n_streams;
  uint32_t* size[kB2fStreams];                  // pass 1 writes, pass 2 reads
  const unsigned long long* local[kB2fStreams];  // exclusive prefix of size[s]: local part + span sums
  const unsigned long long* sums[kB2fStreams];
  uint8_t* out[kB2fStreams];
  B2fCall* call;
};

// What one alignment is, as far as bam2fastq looks: offsets from the start of the record (its block_size field).
struct B2fRec {
  uint32_t len;        // 4 + block_size
  uint32_t flag, l_qseq;
  uint32_t seq, qual;  // packed bases, qualities
  uint32_t tag[T_COUNT];  // the type byte of the first field of that name, 0 = absent
  uint32_t finding, aux;
};

__device__ __forceinline__ uint32_t b2f_type2size(uint32_t t) {  // bam_aux_type2size, bam.h
  if (t == 'C' || t == 'c' || t == 'A') return 1;
  if (t == 'S' || t == 's') return 2;
  if (t == 'I' || t == 'i' || t == 'f' || t == 'F') return 4;
  return 0;
}

// The core fields and bam_aux_get's walk (bam_aux.c, __skip_tag: the type is upper-cased, so `d` has size 0), once for
// all ten names.  rec[0 .. len) is the record; nothing outside it is read.  A walk, a C string or a read that would
// leave the record, and a read the reference's buffers cannot hold, are findings: the caller emits nothing then.
__device__ __forceinline__ void b2f_parse(const uint8_t* rec, uint32_t len, B2fRec& r) {
  r.len = len;
  r.finding = r.aux = 0;
#pragma unroll
  for (int t = 0; t < T_COUNT; ++t) r.tag[t] = 0;
  const uint32_t l_qname = rec[12];
  const uint32_t flag_nc = bam_ld32(rec + 16);
  r.flag = flag_nc >> 16;
  r.l_qseq = bam_ld32(rec + 20);
  r.seq = r.qual = 0;
  if (r.flag & 0x100u) return;  // BAM_FSECONDARY: counted, never looked at (:257)
  const uint64_t seq_at = 36ull + l_qname + 4ull * (flag_nc & 0xFFFFu);
  const uint64_t aux_at = seq_at + (((uint64_t)r.l_qseq + 1) >> 1) + r.l_qseq;
  if (aux_at > len) {
    r.finding = (uint32_t)FQG_E_B2F_AUX;
    return;
  }
  r.seq = (uint32_t)seq_at;
  r.qual = (uint32_t)(seq_at + ((r.l_qseq + 1u) >> 1));
  uint32_t s = (uint32_t)aux_at;
  bool bad = false;
  while (s < len) {
    if (s + 3 > len) {  // the name and the type byte
      bad = true;
      break;
    }
    const uint32_t name = ((uint32_t)rec[s] << 8) | rec[s + 1];
    int t = -1;
    switch (name) {
      case ('o' << 8) | 'n': t = T_ON; break;
      case ('o' << 8) | 'p': t = T_OP; break;
      case ('C' << 8) | 'R': t = T_CR; break;
      case ('C' << 8) | 'Y': t = T_CY; break;
      case ('R' << 8) | 'X': t = T_RX; break;
      case ('Q' << 8) | 'X': t = T_QX; break;
      case ('U' << 8) | 'B': t = T_UB; break;
      case ('U' << 8) | 'Y': t = T_UY; break;
      case ('B' << 8) | 'C': t = T_BC; break;
      case ('Q' << 8) | 'T': t = T_QT; break;
      default: break;
    }
    s += 2;
    if (t >= 0) {
#pragma unroll
      for (int k = 0; k < T_COUNT; ++k)  // (a register array: no dynamic index)
        if (k == t && r.tag[k] == 0) r.tag[k] = s;
    }
    uint32_t type = rec[s];
    if (type >= 'a' && type <= 'z') type -= 32;
    ++s;
    if (type == 'Z' || type == 'H') {
      while (s < len && rec[s]) ++s;
      if (s >= len) {
        bad = true;
        break;
      }
      ++s;
    } else if (type == 'B') {
      if (s + 5 > len) {
        bad = true;
        break;
      }
      const int32_t cnt = (int32_t)bam_ld32(rec + s + 1);
      const uint64_t to = (uint64_t)s + 5ull + (uint64_t)b2f_type2size(rec[s]) * (uint64_t)(uint32_t)cnt;
      if (cnt < 0 || to > len) {
        bad = true;
        break;
      }
      s = (uint32_t)to;
    } else {
      s += b2f_type2size(type);
      if (s > len) {
        bad = true;
        break;
      }
    }
  }
  if (!bad) {  // bam1_qname as a C string
    uint32_t z = 36;
    while (z < len && rec[z]) ++z;
    bad = z >= len;
  }
  if (bad) r.finding = (uint32_t)FQG_E_B2F_AUX;
  else if (r.l_qseq >= kB2fMaxSeq) r.finding = (uint32_t)FQG_E_B2F_TOO_LONG;
}

// Sinks of b2f_records: begin(stream) starts a FASTQ record in that stream, put(byte) adds to it.
struct B2fCount {
  uint32_t n[kB2fStreams];
  int cur;
  __device__ __forceinline__ void begin(int s) { cur = s; }
  __device__ __forceinline__ void put(uint8_t) {
#pragma unroll
    for (int k = 0; k < kB2fStreams; ++k) n[k] += (k == cur);
  }
  __device__ __forceinline__ void put2(uint32_t, bool two) { put(0), two ? put(0) : (void)0; }
};
struct B2fWrite {
  uint8_t* w[kB2fStreams];
  uint8_t* p;
  int cur;
  __device__ __forceinline__ void begin(int s) {
    flush();
    cur = s;
#pragma unroll
    for (int k = 0; k < kB2fStreams; ++k)
      if (k == s) p = w[k];
  }
  __device__ __forceinline__ void flush() {
#pragma unroll
    for (int k = 0; k < kB2fStreams; ++k)
      if (k == cur) w[k] = p;
  }
  __device__ __forceinline__ void put(uint8_t b) { *p++ = b; }
  __device__ __forceinline__ void put2(uint32_t two_chars, bool two) {
    p[0] = (uint8_t)two_chars;
    if (two) p[1] = (uint8_t)(two_chars >> 8);
    p += two ? 2 : 1;
  }
};

// get_tag (:46-55): 0 NULL; otherwise the offset of the C string - of an empty one (the NUL that ends the record's
// read name is as good as any) when the field is not of type Z / H (bam_aux2Z looks at the type as it is written)
__device__ __forceinline__ uint32_t b2f_value(const uint8_t* rec, const B2fRec& r, int t, uint32_t empty_at) {
  uint32_t at = 0;
#pragma unroll
  for (int k = 0; k < T_COUNT; ++k)
    if (k == t) at = r.tag[k];
  if (!at) return 0;
  return (rec[at] == 'Z' || rec[at] == 'H') ? at + 1 : empty_at;
}

// The FASTQ records of one alignment (:260-353), byte by byte into the sink.  The finding of a 10x run, if any, goes
// to r.finding / r.aux (nothing of the alignment is written then); *no_on: the alignment has no `on` tag.
template <class Sink>
__device__ __forceinline__ void b2f_records(const uint8_t* rec, B2fRec& r, int tenx, Sink& o, bool* no_on) {
  *no_on = false;
  if ((r.flag & 0x100u) || r.finding) return;
  uint32_t empty_at = 36;
  while (rec[empty_at]) ++empty_at;  // (inside the record: b2f_parse found the NUL)
  auto cstr = [&](uint32_t at) {
    if (!at) return;
    for (uint8_t c; (c = rec[at]) != 0; ++at) o.put(c);
  };
  auto lit3 = [&]() { o.put('\n'), o.put('+'), o.put('\n'); };
  auto bases = [&]() {  // bam_nt16_rev_table, two bases per byte, the table in a register pair
    constexpr uint64_t t0 = 0x565352474D43413Dull, hi = 0x4E42444B48595754ull;  // "=ACMGRSV", "TWYHKDBN" (low byte first)
    const uint32_t nb = (r.l_qseq + 1u) >> 1;
    for (uint32_t k = 0; k < nb; ++k) {
      const uint32_t b = rec[r.seq + k];
      const uint32_t a = b >> 4, c = b & 15u;
      const uint32_t ca = (uint32_t)(((a & 8u) ? hi : t0) >> (8u * (a & 7u))) & 0xFFu;
      const uint32_t cc = (uint32_t)(((c & 8u) ? hi : t0) >> (8u * (c & 7u))) & 0xFFu;
      o.put2(ca | (cc << 8), 2 * k + 1 < r.l_qseq);
    }
  };
  const uint32_t hdr = b2f_value(rec, r, T_ON, empty_at);
  const uint32_t qual = b2f_value(rec, r, T_OP, empty_at);
  const bool paired = r.flag & 1u;
  if (!hdr) {  // not written by fastq2bam (:263-295)
    *no_on = true;
    if (tenx) {
      r.finding = (uint32_t)FQG_E_B2F_NOT_FASTQ2BAM;
      return;
    }
    const int to = !paired ? B2F_SE : (r.flag & 4u) ? B2F_R1 : B2F_R2;
    o.begin(to);
    o.put('@');
    cstr(36);
    if (to != B2F_SE) o.put('/'), o.put((uint8_t)('1' + to));
    o.put('\n');
    bases();
    lit3();
    for (uint32_t k = 0; k < r.l_qseq; ++k) {  // get_qual (:154-162): a byte that wraps to NUL ends the C string
      const uint8_t q = (uint8_t)(33u + rec[r.qual + k]);
      if (!q) break;
      o.put(q);
    }
    o.put('\n');
    return;
  }
  if (tenx) {  // :299-326
    const uint32_t cell = b2f_value(rec, r, T_CR, empty_at), cell_q = b2f_value(rec, r, T_CY, empty_at);
    uint32_t umi = b2f_value(rec, r, T_RX, empty_at), umi_q = b2f_value(rec, r, T_QX, empty_at);
    if (!umi) umi = b2f_value(rec, r, T_UB, empty_at);
    if (!umi_q) umi_q = b2f_value(rec, r, T_UY, empty_at);
    const uint32_t sample = b2f_value(rec, r, T_BC, empty_at), sample_q = b2f_value(rec, r, T_QT, empty_at);
    if (!cell) r.finding = (uint32_t)FQG_E_B2F_CELL;
    else if (!cell_q) r.finding = (uint32_t)FQG_E_B2F_CELL_QUAL;
    else if (!umi) r.finding = (uint32_t)FQG_E_B2F_UMI;
    else if (!umi_q) r.finding = (uint32_t)FQG_E_B2F_UMI_QUAL;
    else if (sample && !sample_q) {
      r.finding = (uint32_t)FQG_E_B2F_SAMPLE_QUAL;
      r.aux = sample;
    }
    if (r.finding) return;
    // restore_read_name (:128-143): every '@' up to the one in front of "1:" / "2:" becomes a space, that digit the
    // file's own; no such place: every '@' a space, and the files get suffixes
    uint32_t pos = 0;
    for (uint32_t i = hdr; rec[i]; ++i)
      if (rec[i] == '@') {
        const uint8_t c1 = rec[i + 1];
        if ((c1 == '1' || c1 == '2') && rec[i + 2] == ':') {
          pos = i + 1;
          break;
        }
      }
    auto name = [&](uint8_t digit, uint8_t suffix) {
      o.put('@');
      for (uint32_t i = hdr; rec[i]; ++i) {
        uint8_t c = rec[i];
        if (c == '@' && (!pos || i < pos)) c = ' ';
        if (i == pos) c = digit;
        o.put(c);
      }
      if (!pos) o.put('/'), o.put(suffix);
      o.put('\n');
    };
    o.begin(B2F_R1);
    name('1', '1');
    cstr(cell), cstr(umi);
    lit3();
    cstr(cell_q), cstr(umi_q);
    o.put('\n');
    if (sample) {
      o.begin(B2F_I1);
      name('1', '3');
      cstr(sample);
      lit3();
      cstr(sample_q);
      o.put('\n');
    }
    o.begin(B2F_R2);
    name('2', '2');
    bases();
    lit3();
    cstr(qual);
    o.put('\n');
    return;
  }
  auto plain = [&](int to, uint32_t line2, bool is_bases, uint32_t line4) {
    o.begin(to);
    o.put('@');
    cstr(hdr);
    o.put('\n');
    if (is_bases) bases();
    else cstr(line2);
    lit3();
    cstr(line4);
    o.put('\n');
  };
  if (!paired || (r.flag & 0x40u)) {  // :332-349
    plain(paired ? B2F_R1 : B2F_SE, 0, true, qual);
    uint32_t v;
    if ((v = b2f_value(rec, r, T_CR, empty_at)) != 0) plain(B2F_CELL, v, false, b2f_value(rec, r, T_CY, empty_at));
    if ((v = b2f_value(rec, r, T_RX, empty_at)) != 0) plain(B2F_UMI, v, false, b2f_value(rec, r, T_QX, empty_at));
    if ((v = b2f_value(rec, r, T_BC, empty_at)) != 0) plain(B2F_SAMPLE, v, false, b2f_value(rec, r, T_QT, empty_at));
  } else {
    plain(B2F_R2, 0, true, qual);
  }
}

// EMIT = false: what every alignment adds to every stream, the findings, who writes first (pass 1).  EMIT = true: the
// FASTQ records (pass 2, after the scans).  A tile whose span or output images do not fit LDS works on the stream itself.
template <bool EMIT>
__global__ __launch_bounds__(kWave) void k_b2f_tile(B2fTiles A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_b2f[];
  uint8_t* s_in = s_b2f;
  uint8_t* s_out = s_b2f + A.in_cap + 32;
  const int lane = (int)threadIdx.x;
  BamTileView v;
  if (!bam_tile_view(A, lane, v)) return;
  const uint32_t i0 = v.i0, Tn = v.Tn, i = v.i;
  const bool valid = v.valid;
  const uint64_t in_off = v.in_off;
  // the output spans of the tile, stream by stream, one behind the other in LDS at 16-byte boundaries + their skew
  uint64_t out_off[kB2fStreams];
  uint32_t img_at[kB2fStreams], img_len[kB2fStreams], img_skew[kB2fStreams];
  uint32_t out_need = 0;
  if (EMIT) {
#pragma unroll
    for (int s = 0; s < kB2fStreams; ++s) {
      out_off[s] = 0;
      img_at[s] = img_len[s] = img_skew[s] = 0;
      if (s < A.n_streams) {
        out_off[s] = A.local[s][i] + A.sums[s][i / kScan64Span];
        const BamImage im = bam_tile_image(A.out[s], out_off[s], A.size[s][i], Tn);
        img_skew[s] = im.skew;
        img_len[s] = im.len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)im.len;
        img_at[s] = out_need;
        const uint64_t need = (uint64_t)out_need + ((img_skew[s] + im.len + 15ull) & ~15ull);
        out_need = need > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)need;
      }
    }
  }
  const bool fits = v.in_skew + (v.in_end - v.in0) + 16 <= (uint64_t)A.in_cap && (!EMIT || (uint64_t)out_need + 16 <= (uint64_t)A.out_cap);
  const uint8_t* rec;  // the lane's record, in LDS or in the stream
  uint64_t lim;        // the end of what may be read, as a stream offset
  if (fits) {
    const uint64_t base = bam_tile_stage(A, v, lane, s_in);
    rec = s_in + (uint32_t)(in_off - base);
    lim = v.in_end;
  } else {
    rec = A.buf + in_off;
    lim = A.nbytes;
  }
  // the lane's record: its length field was read by the caller's index, but nothing vouches for it here
  B2fRec r;
  r.finding = r.aux = 0;
  r.flag = 0x100u;  // (a record that is not parsed writes nothing)
  r.len = 0;
  const uint32_t block = in_off + 4 <= lim ? bam_ld32(rec) : 0u;
  if (block < 32u || in_off + 4ull + block > lim) r.finding = (uint32_t)FQG_E_B2F_AUX;
  else b2f_parse(rec, 4u + block, r);
  bool no_on = false;
  if (!EMIT) {
    B2fCount cnt;
#pragma unroll
    for (int s = 0; s < kB2fStreams; ++s) cnt.n[s] = 0;
    cnt.cur = 0;
    b2f_records(rec, r, A.tenx, cnt, &no_on);
    if (r.aux >= (1u << 28)) r.finding = (uint32_t)FQG_E_B2F_AUX, r.aux = 0;  // (a record of 256 MiB: no room in the key)
    if (valid && r.finding)
      atomicMin(&A.call->first_finding, ((unsigned long long)i << 32) | ((unsigned long long)(r.finding & 15u) << 28) | r.aux);  // (FQG_E_B2F_* are 24 .. 31)
#pragma unroll
    for (int s = 0; s < kB2fStreams; ++s) {
      if (s < A.n_streams) {
        const uint32_t mine = r.finding ? 0u : cnt.n[s];
        if (valid) A.size[s][i] = mine;
        const unsigned long long m = __ballot(valid && mine != 0);
        if (lane == 0 && m) atomicMin(&A.call->first_record[s], (unsigned long long)i0 + (unsigned long long)__builtin_ctzll(m));
      }
    }
    const unsigned long long m = __ballot(valid && no_on);
    if (lane == 0 && m) atomicMin(&A.call->warn_record, (unsigned long long)i0 + (unsigned long long)__builtin_ctzll(m));
  } else {
    B2fWrite w;
    w.cur = 0;
#pragma unroll
    for (int s = 0; s < kB2fStreams; ++s) {
      w.w[s] = nullptr;
      if (s < A.n_streams)
        w.w[s] = fits ? s_out + img_at[s] + img_skew[s] + (uint32_t)(out_off[s] - rfl64(out_off[s])) : A.out[s] + out_off[s];
    }
    w.p = w.w[0];
    if (valid) b2f_records(rec, r, A.tenx, w, &no_on);
    if (fits) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int s = 0; s < kB2fStreams; ++s)
        if (s < A.n_streams && img_len[s]) emit_flush(s_out + img_at[s], img_skew[s], img_len[s], A.out[s] + rfl64(out_off[s]), lane);
    }
  }
}

}  // namespace fqg
