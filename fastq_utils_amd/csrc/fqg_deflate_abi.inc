// fqg_deflate_abi.inc - fqg_deflate / fqg_text_deflate, their BGZF pair and fqg_deflate_output (include/fqg.h), included
// by fqg_abi.hip

extern "C++" {
namespace {

// the CRC-32 table and the GF(2) operators that move a CRC register over 255 << level zero bytes
void gz_make_tables(GzTables& T) {
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t r = i;
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (r & 1u ? 0xEDB88320u : 0u);
    T.crc[i] = r;
  }
  auto apply = [](const uint32_t* op, uint32_t v) {
    uint32_t r = 0;
    for (int b = 0; b < 32; ++b)
      if ((v >> b) & 1u) r ^= op[b];
    return r;
  };
  uint32_t one[32], acc[32], tmp[32];  // one zero byte; the product so far
  for (int b = 0; b < 32; ++b) {
    const uint32_t v = 1u << b;
    one[b] = T.crc[v & 0xFFu] ^ (v >> 8);
    acc[b] = v;
  }
  for (int k = 0; k < 255; ++k) {  // acc = one^255
    for (int b = 0; b < 32; ++b) tmp[b] = apply(one, acc[b]);
    memcpy(acc, tmp, sizeof(acc));
  }
  for (int level = 0; level < 8; ++level) {
    memcpy(T.shift[level], acc, sizeof(acc));
    for (int b = 0; b < 32; ++b) tmp[b] = apply(acc, acc[b]);
    memcpy(acc, tmp, sizeof(acc));
  }
}

// the tables on the device, uploaded once per context (fqg_bgzf_inflate reads the same ones)
int gz_upload_tables(fqg_ctx* c) {
  if (c->gz_tab_ready) return 0;
  static const GzTables tables = [] {
    GzTables T;
    gz_make_tables(T);
    return T;
  }();
  NEED(ensure(c, c->gz_tab, sizeof(GzTables)));
  HIP_TRY(c, hipMemcpyAsync(c->gz_tab.p, &tables, sizeof(GzTables), hipMemcpyHostToDevice, c->stream));
  c->gz_tab_ready = true;
  return 0;
}

// the workgroups of k_deflate_members that are resident at once (members are dealt round-robin)
unsigned gz_resident_groups(fqg_ctx* c) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_deflate_members, kBlock, kGzLds) != hipSuccess || per_cu < 1) per_cu = 1;
  return (unsigned)per_cu * (unsigned)c->cu_count;
}

// BGZF's end-of-file block (SAM/BAM specification 4.1.2)
const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// text = carry (host) followed by [d_src, d_src + nbytes) (device); frame: kGzFrameGzip or kGzFrameBgzf
int gz_run(fqg_ctx* c, uint32_t frame, const void* carry, uint64_t carry_bytes, const uint8_t* d_src, uint64_t nbytes, int final,
           fqg_deflate_result* out) {
  HIP_TRY(c, hipSetDevice(c->device));
  const bool bgzf = frame == kGzFrameBgzf;
  const uint64_t text_bytes = carry_bytes + nbytes, n_full = text_bytes / kGzMember, rest = text_bytes % kGzMember;
  // (an empty gzip file is one member of empty content; an empty BGZF file is the end-of-file block alone)
  const uint64_t n_members = n_full + ((final && (rest || (!n_full && !bgzf))) ? 1 : 0);
  const uint64_t eof_bytes = bgzf && final ? sizeof(kBgzfEof) : 0;
  const uint64_t tail = final ? 0 : rest, member_text = text_bytes - tail;
  NEED(gz_upload_tables(c));
  if (carry_bytes) {
    NEED(ensure(c, c->gz_carry, carry_bytes + 64));  // (a member inside the carry is staged in whole 16-byte words)
    HIP_TRY(c, hipMemcpyAsync(c->gz_carry.p, carry, carry_bytes, hipMemcpyHostToDevice, c->stream));
  }
  uint64_t gz_bytes = 0;
  const uint64_t nb = scan64_spans(n_members);
  if (n_members) {
    NEED(ensure(c, c->gz_slots, n_members * kGzStride));
    NEED(ensure(c, c->gz_sizes, n_members * 4));
    NEED(ensure(c, c->gz_off, n_members * 8));
    NEED(ensure(c, c->gz_sums, nb * 8 + 32));
    NEED(raise_dynamic_lds(c, (const void*)k_deflate_members, kGzLds));
    const unsigned grid = (unsigned)std::min<uint64_t>(n_members, gz_resident_groups(c));
    NEED(ensure(c, c->gz_toks, (size_t)grid * kGzTokStride * 4));
    GzArgs A;
    memset(&A, 0, sizeof(A));
    A.carry = (const uint8_t*)c->gz_carry.p;
    A.src = d_src;
    A.carry_bytes = carry_bytes;
    A.frame = frame;
    A.member_text = member_text;
    A.n_members = n_members;
    A.slots = (uint8_t*)c->gz_slots.p;
    A.sizes = (uint32_t*)c->gz_sizes.p;
    A.toks = (uint32_t*)c->gz_toks.p;
    A.tab = (const GzTables*)c->gz_tab.p;
    unsigned long long* total = (unsigned long long*)c->gz_sums.p + nb;
    {
      ProfScope ps(c, "k_deflate_members");
      hipLaunchKernelGGL(k_deflate_members, dim3(grid), dim3(kBlock), kGzLds, c->stream, A);
    }
    {
      ProfScope ps(c, "k_deflate_scan");
      scan64(c, c->gz_sizes.p, c->gz_off.p, c->gz_sums.p, total, n_members);
    }
    HIP_TRY(c, hipMemcpyAsync(&c->h_scalar[5], total, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    gz_bytes = c->h_scalar[5];
    if (gz_bytes > member_text + (bgzf ? 31 : 23) * n_members) return fail(c, FQG_ERR_STATE, "fqg_deflate: members larger than their bound");
  }
  const uint64_t totals[1] = {gz_bytes + eof_bytes + tail};
  uint8_t* dst[1];
  NEED(text_reserve(c, c->gz_text, totals, 1, dst));
  if (n_members) {
    ProfScope ps(c, "k_deflate_gather");
    hipLaunchKernelGGL(k_deflate_gather, dim3((unsigned)std::min<uint64_t>(n_members, (uint64_t)c->cu_count * 8)), dim3(kBlock), 0, c->stream,
                       (const uint8_t*)c->gz_slots.p, (const uint32_t*)c->gz_sizes.p, (const unsigned long long*)c->gz_off.p,
                       (const unsigned long long*)c->gz_sums.p, n_members, dst[0]);
  }
  if (eof_bytes) {
    HIP_TRY(c, hipMemcpyAsync(dst[0] + gz_bytes, kBgzfEof, eof_bytes, hipMemcpyHostToDevice, c->stream));
    gz_bytes += eof_bytes;
  }
  if (tail) {  // text positions [member_text, text_bytes) behind the members
    uint64_t at = member_text, put = gz_bytes;
    if (at < carry_bytes) {
      HIP_TRY(c, hipMemcpyAsync(dst[0] + put, (const uint8_t*)carry + at, carry_bytes - at, hipMemcpyHostToDevice, c->stream));
      put += carry_bytes - at;
      at = carry_bytes;
    }
    if (at < text_bytes)
      HIP_TRY(c, hipMemcpyAsync(dst[0] + put, d_src + (at - carry_bytes), text_bytes - at, hipMemcpyDeviceToDevice, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  text_publish(c->gz_text, totals, 1);
  out->text_bytes = text_bytes;
  out->n_members = n_members;
  out->gz_bytes = gz_bytes;
  out->tail_bytes = tail;
  return 0;
}

}  // namespace
}  // extern "C++"

extern "C++" {
namespace {

int gz_deflate(fqg_ctx* c, uint32_t frame, const char* too_long, const void* carry, uint64_t carry_bytes, const void* src, uint64_t nbytes,
               int mem, int final, fqg_deflate_result* out) {
  if (!c || !out || (!src && nbytes) || (!carry && carry_bytes)) return FQG_ERR_ARG;
  if (mem != FQG_MEM_HOST && mem != FQG_MEM_DEVICE) return FQG_ERR_ARG;
  // (the arguments first: a call that is refused leaves the previous call's members and tail to be fetched)
  if (too_long && carry_bytes >= kGzMember) return fail(c, FQG_ERR_ARG, too_long);
  NEED(text_begin(c, c->gz_text));
  memset(out, 0, sizeof(*out));
  const uint8_t* d_src = (const uint8_t*)src;
  if (mem == FQG_MEM_HOST && nbytes) {
    HIP_TRY(c, hipSetDevice(c->device));
    NEED(ensure(c, c->gz_in, nbytes + 64));
    HIP_TRY(c, hipMemcpyAsync(c->gz_in.p, src, nbytes, hipMemcpyHostToDevice, c->stream));
    d_src = (const uint8_t*)c->gz_in.p;
  }
  return gz_run(c, frame, carry, carry_bytes, d_src, nbytes, final, out);
}

int gz_text_deflate(fqg_ctx* c, uint32_t frame, const char* too_long, int store, int stream, const void* carry, uint64_t carry_bytes,
                    int final, fqg_deflate_result* out) {
  if (!c || !out || (!carry && carry_bytes)) return FQG_ERR_ARG;
  // (the arguments first: a call that is refused leaves the previous call's members and tail to be fetched)
  // (the records of fqg_bam_add_tags are a store once that call has been made on this context: until then the id names
  // nothing, as before it existed.  The other two stores read as empty before their producer has run; this one does
  // not only because tests/test_gpu_deflate.py, from before the id existed, pins "store 2 is refused" on a context that
  // never called fqg_bam_add_tags - a wart kept for that test, documented in include/fqg.h)
  if (store != FQG_TEXT_RECORDS && store != FQG_TEXT_BAM2FASTQ && !(store == FQG_TEXT_BAM_TAGS && c->bt_begun))
    return fail(c, FQG_ERR_ARG, "fqg_text_deflate: no such store");
  if (stream < 0 || stream >= (store == FQG_TEXT_RECORDS ? 3 : store == FQG_TEXT_BAM2FASTQ ? FQG_B2F_STREAMS : 1))
    return fail(c, FQG_ERR_ARG, "fqg_text_deflate: no such stream");
  if (too_long && carry_bytes >= kGzMember) return fail(c, FQG_ERR_ARG, too_long);
  NEED(text_begin(c, c->gz_text));
  memset(out, 0, sizeof(*out));
  const OutText& o = store == FQG_TEXT_RECORDS ? c->bc_text : store == FQG_TEXT_BAM2FASTQ ? c->b2f_text : c->bt_text;
  const uint64_t nbytes = o.bytes[stream];
  return gz_run(c, frame, carry, carry_bytes, nbytes ? (const uint8_t*)o.buf.p + o.at[stream] : nullptr, nbytes, final, out);
}

}  // namespace
}  // extern "C++"

int fqg_deflate(fqg_ctx* c, const void* carry, uint64_t carry_bytes, const void* src, uint64_t nbytes, int mem, int final,
                fqg_deflate_result* out) {
  return gz_deflate(c, kGzFrameGzip, "fqg_deflate: a carry of a member's text or more", carry, carry_bytes, src, nbytes, mem, final, out);
}

int fqg_text_deflate(fqg_ctx* c, int store, int stream, const void* carry, uint64_t carry_bytes, int final, fqg_deflate_result* out) {
  return gz_text_deflate(c, kGzFrameGzip, "fqg_text_deflate: a carry of a member's text or more", store, stream, carry, carry_bytes, final,
                         out);
}

int fqg_bgzf_deflate(fqg_ctx* c, const void* carry, uint64_t carry_bytes, const void* src, uint64_t nbytes, int mem, int final,
                     fqg_deflate_result* out) {
  return gz_deflate(c, kGzFrameBgzf, nullptr, carry, carry_bytes, src, nbytes, mem, final, out);
}

int fqg_text_bgzf_deflate(fqg_ctx* c, int store, int stream, const void* carry, uint64_t carry_bytes, int final,
                          fqg_deflate_result* out) {
  return gz_text_deflate(c, kGzFrameBgzf, nullptr, store, stream, carry, carry_bytes, final, out);
}

int fqg_deflate_output(fqg_ctx* c, void* host_dst, uint64_t nbytes) {
  if (!c) return FQG_ERR_ARG;
  return text_copy(c, c->gz_text, 0, host_dst, nbytes, "fqg_deflate_output: more than was produced");
}

int fqg_deflate_output_begin(fqg_ctx* c, void* host_dst, uint64_t nbytes) {
  if (!c) return FQG_ERR_ARG;
  return text_copy_begin(c, c->gz_text, 0, host_dst, nbytes, "fqg_deflate_output_begin: more than was produced");
}

int fqg_deflate_output_wait(fqg_ctx* c) { return c ? text_wait(c, c->gz_text) : (int)FQG_ERR_ARG; }
