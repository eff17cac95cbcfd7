// fqg_inflate_abi.inc - fqg_bgzf_inflate, fqg_inflate_output, fqg_inflate_device (include/fqg.h), included by fqg_abi.hip

extern "C++" {
namespace {

// the workgroups of k_inflate_blocks that are resident at once (blocks are dealt round-robin)
unsigned inf_resident_groups(fqg_ctx* c) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_inflate_blocks, kInfBlock, kInfLds) != hipSuccess || per_cu < 1) per_cu = 1;
  return (unsigned)per_cu * (unsigned)c->cu_count;
}

// The walk over the block headers, with exactly the rules of host/fq_parallel.h: bgzf_inflate_parallel - the magic
// 1f 8b 08 with FLG & 4, XLEN, the BC subfield of length 2 anywhere among the subfields (the last one counts), BSIZE + 1
// inside the file and at least 12 + XLEN + 8; fewer than 18 bytes behind the last block end the walk silently.
// Returns null, or what is wrong with block rows.size().
const char* inf_walk(const uint8_t* raw, uint64_t nbytes, std::vector<InfBlockRow>& rows, uint64_t* used, uint64_t* total) {
  uint64_t p = 0, sum = 0;
  while (p + 18 <= nbytes) {
    if (raw[p] != 0x1f || raw[p + 1] != 0x8b || raw[p + 2] != 8 || !(raw[p + 3] & 4)) return "not a BGZF block header";
    const uint64_t xlen = raw[p + 10] | (raw[p + 11] << 8);
    uint64_t q = p + 12, bsize = 0;
    bool found = false;
    while (q + 4 <= p + 12 + xlen && q + 4 <= nbytes) {
      const uint64_t slen = raw[q + 2] | (raw[q + 3] << 8);
      if (raw[q] == 66 && raw[q + 1] == 67 && slen == 2 && q + 6 <= nbytes) {
        bsize = (uint64_t)(raw[q + 4] | (raw[q + 5] << 8)) + 1;
        found = true;
      }
      q += 4 + slen;
    }
    if (!found) return "no BC subfield";
    if (p + bsize > nbytes) return "BSIZE passes the end of the file";
    if (bsize < 12 + xlen + 8) return "BSIZE smaller than the block's header and trailer";
    const uint8_t* z = raw + p + bsize - 4;
    const uint32_t isize = (uint32_t)z[0] | ((uint32_t)z[1] << 8) | ((uint32_t)z[2] << 16) | ((uint32_t)z[3] << 24);
    if (isize > inf::kInfMaxIsize) return "ISIZE above 65536";
    rows.push_back({p + 12 + xlen, sum, (uint32_t)(bsize - 12 - xlen - 8), isize});
    sum += isize;
    p += bsize;
  }
  *used = p;
  *total = sum;
  return nullptr;
}

}  // namespace
}  // extern "C++"

int fqg_bgzf_inflate(fqg_ctx* c, const void* raw, uint64_t nbytes, fqg_inflate_result* out) {
  if (!c || !out || (!raw && nbytes)) return FQG_ERR_ARG;
  // (the file first: a call that is refused leaves the previous call's stream to be fetched)
  std::vector<InfBlockRow> rows;
  uint64_t used = 0, total = 0;
  if (const char* what = inf_walk((const uint8_t*)raw, nbytes, rows, &used, &total))
    return fail(c, FQG_ERR_ARG, ("fqg_bgzf_inflate: block " + std::to_string(rows.size()) + ": " + what).c_str());
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t n = rows.size();
  c->inf_valid = false;
  c->inf_bytes = 0;
  memset(out, 0, sizeof(*out));
  out->raw_bytes = used;
  out->n_blocks = n;
  out->out_bytes = total;
  out->bad_block = out->crc_block = UINT64_MAX;
  out->code = FQG_OK;
  NEED(ensure(c, c->inf_out, total + 64));  // (whole 16-byte words, and an address for an empty stream)
  if (n) {
    NEED(gz_upload_tables(c));
    NEED(ensure(c, c->inf_raw, used + 64));  // (the 16-byte word that holds a payload's last byte is loaded whole)
    NEED(ensure(c, c->inf_rows, n * sizeof(InfBlockRow)));
    NEED(ensure(c, c->inf_status, n * 4));
    NEED(ensure(c, c->inf_first, 16));
    HIP_TRY(c, hipMemcpyAsync(c->inf_raw.p, raw, used, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->inf_rows.p, rows.data(), n * sizeof(InfBlockRow), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->inf_first.p, 0xFF, 16, c->stream));
    NEED(raise_dynamic_lds(c, (const void*)k_inflate_blocks, kInfLds));
    InfArgs A;
    A.raw = (const uint8_t*)c->inf_raw.p;
    A.rows = (const InfBlockRow*)c->inf_rows.p;
    A.n_blocks = n;
    A.out = (uint8_t*)c->inf_out.p;
    A.status = (uint32_t*)c->inf_status.p;
    A.first = (unsigned long long*)c->inf_first.p;
    A.tab = (const GzTables*)c->gz_tab.p;
    {
      ProfScope ps(c, "k_inflate_blocks");
      hipLaunchKernelGGL(k_inflate_blocks, dim3((unsigned)std::min<uint64_t>(n, inf_resident_groups(c))), dim3(kInfBlock), kInfLds, c->stream, A);
    }
    HIP_TRY(c, hipMemcpyAsync(&c->h_scalar[6], c->inf_first.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the rows and, for a pageable `raw`, the file are the caller's again)
    HIP_TRY(c, hipGetLastError());
    out->bad_block = c->h_scalar[6];
    out->crc_block = c->h_scalar[7];
    if (out->bad_block != UINT64_MAX) {
      if (out->bad_block >= n) return fail(c, FQG_ERR_STATE, "fqg_bgzf_inflate: a block number that does not exist");
      HIP_TRY(c, hipMemcpyAsync(&c->h_scalar[6], (const uint32_t*)c->inf_status.p + out->bad_block, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      out->code = (int32_t)(c->h_scalar[6] & 0xFFFFu);
    }
  }
  c->inf_bytes = total;
  c->inf_valid = true;
  return 0;
}

int fqg_inflate_output(fqg_ctx* c, uint64_t first, void* host_dst, uint64_t nbytes) {
  if (!c || (!host_dst && nbytes)) return FQG_ERR_ARG;
  if (!c->inf_valid) return fail(c, FQG_ERR_STATE, "fqg_inflate_output: no inflated stream");
  if (first > c->inf_bytes || nbytes > c->inf_bytes - first) return fail(c, FQG_ERR_ARG, "fqg_inflate_output: more than was produced");
  if (!nbytes) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(host_dst, (const uint8_t*)c->inf_out.p + first, nbytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

const void* fqg_inflate_device(const fqg_ctx* c) { return c && c->inf_valid ? c->inf_out.p : nullptr; }
