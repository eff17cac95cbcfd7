// fqg_filter_abi.inc - host side of fqg_filter_kernels.hip: fqg_records_filter / _info / _output (fastq_filter_n,
// fastq_trim_poly_at) and fqg_records_gather / _output (fastq_filterpair's partitions).  Included by fqg_abi.hip inside
// extern "C", behind fqg_barcode_abi.inc (bc_tile_one, the output calls).  fqg_records_filter is its phases in order
// (rf_prepare, rf_plan, rf_write) on one RfCall; what happens on the stream happens in the order of the text.
extern "C++" {
namespace {
// one call of fqg_records_filter on its way through the phases
struct RfCall {
  BcParams F;  // the frame as the transform's READ1, alone
  RfParams P;
  BcTile tc;
  uint64_t n_rec = 0, n_tiles = 0;
};

// parameters, buffers, counters, tile
int rf_prepare(fqg_ctx* c, const fqg_frame* frame, uint64_t first_record, uint64_t n_rec, const fqg_filter_params* fp, RfCall& R) {
  BcParams& F = R.F;
  memset(&F, 0, sizeof(F));
  F.f[1].fv = frame->fv;
  F.f[1].first = first_record;
  F.f[1].step = 1;
  F.f[1].present = 1;
  F.f[1].has_nul = F.has_nul = (frame->flags & kFlagNul) ? 1 : 0;  // lines are C strings then (bc_clip_nul)
  F.n_inputs = 1;
  F.emit[1] = 1;
  R.P = RfParams{fp->mode, fp->max_n_percent > 100 ? 100 : fp->max_n_percent, fp->min_poly_at_len, (uint64_t)fp->min_len};
  R.n_rec = n_rec;
  NEED(ensure(c, c->bc_status, n_rec));
  NEED(ensure(c, c->bc_len[1], n_rec * 4));
  NEED(ensure(c, c->bc_off[1], n_rec * 8));
  NEED(ensure(c, c->bc_sum[1], scan64_spans(n_rec) * 8));
  NEED(bcall_reset(c, 0));
  // (the tiles are the EMIT kernel's alone - the plan works record by record - and that kernel likes 24 KiB per
  // wavefront better than the 20 KiB it shared with a staging plan: tools/tiles_lds_sweep.sh)
  R.tc = bc_tile_one(frame->fv, 24576u);
  R.n_tiles = (n_rec + R.tc.T - 1) / R.tc.T;
  return ensure(c, c->bc_tile_big, R.n_tiles);
}

// what every record keeps, where it goes (scan64), the tiles that do not fit LDS; the counts
int rf_plan(fqg_ctx* c, const RfCall& R, fqg_filter_result* out) {
  const uint64_t n_rec = R.n_rec;
  {
    ProfScope ps(c, "k_rf_plan");
    const bool by_n = R.P.mode == FQG_FILTER_N;  // (eight lanes a record)
    const uint64_t per_wg = by_n ? 32 : kBlock;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_rec + per_wg - 1) / per_wg, (uint64_t)c->cu_count * 32));
    const auto plan = by_n ? k_rf_plan_n : k_rf_plan_records;
    hipLaunchKernelGGL(plan, dim3(grid), dim3(kBlock), 0, c->stream, R.F, R.P, n_rec, (uint8_t*)c->bc_status.p,
                       (uint32_t*)c->bc_len[1].p, c->d_bcall);
  }
  {
    // (the plan kernels count what they drop and trim; the tile flags come behind the scan, whose offsets they use)
    ProfScope ps(c, "k_rf_scan");
    scan64(c, c->bc_len[1].p, c->bc_off[1].p, c->bc_sum[1].p, bcall_totals(c->d_bcall) + 1, n_rec);
    hipLaunchKernelGGL(k_rf_tile_flags, dim3((unsigned)((R.n_tiles + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, R.F, R.tc,
                       n_rec, (const uint32_t*)c->bc_len[1].p, (const unsigned long long*)c->bc_off[1].p,
                       (const unsigned long long*)c->bc_sum[1].p, (uint8_t*)c->bc_tile_big.p, c->d_bcall);
  }
  NEED(bcall_fetch(c, 64));
  out->n_discarded = c->h_bcall->discarded;
  out->n_trimmed = c->h_bcall->short_warnings;
  out->n_kept = n_rec - out->n_discarded;
  out->out_bytes = bcall_totals(c->h_bcall)[1];
  return 0;
}

// the text: tile by tile whenever there is any, record by record for the tiles that do not fit LDS
int rf_write(fqg_ctx* c, const RfCall& R, uint64_t out_bytes) {
  const uint64_t totals[2] = {0, out_bytes};  // (stream 1, as the transform's read1)
  uint8_t* text[2];
  NEED(text_reserve(c, c->bc_text, totals, 2, text));
  text_publish(c->bc_text, totals, 2);
  unsigned grid_t = 0;
  if (out_bytes) {
    ProfScope ps(c, "k_rf_emit");
    const EmitOut eo{(const uint32_t*)c->bc_len[1].p, (const unsigned long long*)c->bc_off[1].p,
                     (const unsigned long long*)c->bc_sum[1].p, text[1]};
    grid_t = launch_tile_pair(c, k_rf_emit_tile, true, R.n_tiles, R.tc.in_cap + R.tc.out_cap, k_rf_emit_direct, c->h_bcall->big != 0,
                              R.n_rec, 8, R.F, R.P, R.tc, R.n_rec, (const uint8_t*)c->bc_status.p, (const uint8_t*)c->bc_tile_big.p, eo);
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  // (grid 0: every record was dropped, nothing was emitted)
  const uint64_t info[6] = {R.n_tiles, c->h_bcall->big, grid_t, R.tc.T, R.tc.in_cap, R.tc.out_cap};
  for (int i = 0; i < 6; ++i) c->filter_info[i] = info[i];
  return 0;
}

}  // namespace
}  // extern "C++"

int fqg_records_filter(fqg_ctx* c, const fqg_frame* frame, uint64_t first_record, uint64_t n_rec,
                       const fqg_filter_params* fp, fqg_filter_result* out) {
  if (!c || !frame || !fp || !out) return FQG_ERR_ARG;
  NEED(text_begin(c, c->bc_text));
  memset(out, 0, sizeof(*out));
  for (uint64_t& v : c->filter_info) v = 0;
  if (fp->mode != FQG_FILTER_N && fp->mode != FQG_FILTER_POLY_AT) return fail(c, FQG_ERR_ARG, "fqg_records_filter: unknown mode");
  if (first_record > frame->fv.n_records || n_rec > frame->fv.n_records - first_record)
    return fail(c, FQG_ERR_ARG, "fqg_records_filter: records beyond the frame");
  HIP_TRY(c, hipSetDevice(c->device));
  out->n_records = n_rec;
  if (!n_rec) return 0;
  RfCall R;
  NEED(rf_prepare(c, frame, first_record, n_rec, fp, R));
  NEED(rf_plan(c, R, out));
  return rf_write(c, R, out->out_bytes);
}

int fqg_records_filter_info(const fqg_ctx* c, uint64_t info[6]) {
  if (!c || !info) return FQG_ERR_ARG;
  for (int i = 0; i < 6; ++i) info[i] = c->filter_info[i];
  return 0;
}
int fqg_records_filter_output(fqg_ctx* c, void* host_dst, uint64_t nbytes) { return fqg_barcodes_output(c, 1, host_dst, nbytes); }

// ---- ordered gather of whole records ------------------------------------------------------------------
int fqg_records_gather(fqg_ctx* c, const fqg_frame* frame, const uint64_t* records, uint64_t n, uint64_t* out_bytes) {
  if (!c || !frame || !out_bytes || (!records && n)) return FQG_ERR_ARG;
  NEED(text_begin(c, c->bc_text));
  *out_bytes = 0;
  if (!n) return 0;
  for (uint64_t k = 0; k < n; ++k)
    if (records[k] >= frame->fv.n_records) return fail(c, FQG_ERR_ARG, "fqg_records_gather: record outside the frame");
  HIP_TRY(c, hipSetDevice(c->device));
  const bool nul = (frame->flags & kFlagNul) != 0;
  const uint64_t nb = scan64_spans(n);
  NEED(ensure(c, c->bc_off[1], n * 8));  // the list
  NEED(ensure(c, c->bc_len[1], n * 4));
  NEED(ensure(c, c->bc_off[2], n * 8));  // local offsets
  NEED(ensure(c, c->bc_sum[1], nb * 8 + 16));
  const auto list = (const unsigned long long*)c->bc_off[1].p, local = (const unsigned long long*)c->bc_off[2].p,
             sums = (const unsigned long long*)c->bc_sum[1].p;
  unsigned long long* d_tot = (unsigned long long*)c->bc_sum[1].p + nb;
  HIP_TRY(c, hipMemcpyAsync(c->bc_off[1].p, records, n * 8, hipMemcpyHostToDevice, c->stream));
  {
    ProfScope ps(c, "k_gather_plan");
    const auto lens = nul ? k_gather_lens_nul : k_gather_lens;
    hipLaunchKernelGGL(lens, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, frame->fv, list, n,
                       (uint32_t*)c->bc_len[1].p);
    scan64(c, c->bc_len[1].p, c->bc_off[2].p, c->bc_sum[1].p, d_tot, n);
  }
  HIP_TRY(c, hipMemcpyAsync(&c->h_scalar[2], d_tot, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint64_t total = c->h_scalar[2], totals[2] = {0, total};  // (stream 1, as the filter)
  uint8_t* text[2];
  NEED(text_reserve(c, c->bc_text, totals, 2, text));
  {
    ProfScope ps(c, "k_gather_copy");
    if (nul)  // what gzputs writes of a line is the C string: four pieces per record
      hipLaunchKernelGGL(k_gather_copy_nul, dim3((unsigned)std::min<uint64_t>((n + 3) / 4, (uint64_t)c->cu_count * 16)), dim3(kBlock), 0,
                         c->stream, frame->fv, list, n, local, sums, text[1]);
    else
      hipLaunchKernelGGL(k_gather_copy, dim3((unsigned)std::min<uint64_t>((n + 4 * kWave - 1) / (4 * kWave), (uint64_t)c->cu_count * 16)),
                         dim3(kBlock), 0, c->stream, frame->fv, list, n, local, sums, (const uint32_t*)c->bc_len[1].p, text[1]);
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  text_publish(c->bc_text, totals, 2);
  *out_bytes = total;
  return 0;
}
int fqg_records_gather_output(fqg_ctx* c, void* host_dst, uint64_t nbytes) { return fqg_barcodes_output(c, 1, host_dst, nbytes); }
