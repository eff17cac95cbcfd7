// fqg_bamtags_abi.inc - fqg_bam_add_tags / fqg_bam_add_tags_output (include/fqg.h), included by fqg_abi.hip

int fqg_bam_add_tags(fqg_ctx* c, const void* stream, uint64_t nbytes, int mem, const uint64_t* offsets, uint64_t n_records,
                     const fqg_bam_tags_params* prm, fqg_bam_tags_result* out) {
  const uint8_t* d_buf;
  uint64_t first_offset = 0;
  auto begin = [&] {
    if (prm->n_targets && (!prm->tx_off || !prm->tx_len || !prm->gx_off || !prm->gx_len || !prm->names)) return (int)FQG_ERR_ARG;
    memset(out, 0, sizeof(*out));
    out->n_alignments = n_records;
    c->bt_begun = true;
    return text_begin(c, c->bt_text);
  };
  NEED(bam_input(c, "fqg_bam_add_tags", out && prm, stream, nbytes, mem, offsets, n_records, begin, &d_buf, &first_offset));
  if (!n_records) return 0;
  const uint32_t n = (uint32_t)n_records;
  hipStream_t st = c->stream;

  BtParams P;
  memset(&P, 0, sizeof(P));
  P.tenx = prm->tenx;
  P.tx_tag = prm->tx_tag;
  P.n_targets = prm->n_targets;
  const size_t nt = prm->n_targets;
  NEED(ensure(c, c->bt_tables, nt * 16 + prm->names_bytes + 64));
  {
    uint32_t* t = (uint32_t*)c->bt_tables.p;
    if (nt) {
      HIP_TRY(c, hipMemcpyAsync(t, prm->tx_off, nt * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(t + nt, prm->tx_len, nt * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(t + 2 * nt, prm->gx_off, nt * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(t + 3 * nt, prm->gx_len, nt * 4, hipMemcpyHostToDevice, st));
      if (prm->names_bytes)
        HIP_TRY(c, hipMemcpyAsync(t + 4 * nt, prm->names, prm->names_bytes, hipMemcpyHostToDevice, st));
      for (size_t k = 0; k < nt; ++k) {
        if ((uint64_t)prm->tx_off[k] + prm->tx_len[k] > prm->names_bytes) return fail(c, FQG_ERR_ARG, "fqg_bam_add_tags: name table");
        if (prm->gx_len[k] != FQG_NO_GENE && (uint64_t)prm->gx_off[k] + prm->gx_len[k] > prm->names_bytes)
          return fail(c, FQG_ERR_ARG, "fqg_bam_add_tags: name table");
      }
    }
    P.tx_off = t;
    P.tx_len = t + nt;
    P.gx_off = t + 2 * nt;
    P.gx_len = t + 3 * nt;
    P.names = (const uint8_t*)(t + 4 * nt);
  }

  const uint64_t nb = scan64_spans(n);
  NEED(ensure(c, c->bam_size, (size_t)n * 4));
  NEED(ensure(c, c->bam_local, (size_t)n * 8));
  NEED(ensure(c, c->bam_sums, (size_t)nb * 8 + 64));
  NEED(ensure(c, c->bt_call, sizeof(BtCall) + 16));
  BtCall h_call;
  memset(&h_call, 0, sizeof(h_call));
  h_call.first_finding = ~0ull;
  BtCall* d_call = (BtCall*)c->bt_call.p;
  unsigned long long* d_total = (unsigned long long*)((char*)c->bt_call.p + sizeof(BtCall));
  HIP_TRY(c, hipMemcpyAsync(d_call, &h_call, sizeof(h_call), hipMemcpyHostToDevice, st));
  const double mean_in = (double)(nbytes - first_offset) / (double)n;
  BtTiles A;
  memset(&A, 0, sizeof(A));
  bam_tile_shape(A, kBtInCap, kBtOutCap, mean_in, 1.15 * (mean_in + 16.0 * 4 + (prm->tx_tag ? 40.0 : 0.0)), 0, "FQGPU_BT_T");
  const unsigned lds = A.in_cap + A.out_cap + 64;
  A.buf = d_buf;
  A.nbytes = nbytes;
  A.offs = c->bam_offs;
  A.n = n;
  A.new_size = (uint32_t*)c->bam_size.p;
  A.out_local = (const unsigned long long*)c->bam_local.p;
  A.out_sums = (const unsigned long long*)c->bam_sums.p;
  A.P = P;
  A.call = d_call;
  const unsigned grid = (n + A.T - 1) / A.T;
  {
    ProfScope ps(c, "k_bt_plan");
    hipLaunchKernelGGL(k_bt_tile<false>, dim3(grid), dim3(kWave), A.in_cap + 64, st, A);
  }
  {
    ProfScope ps(c, "k_bt_scan");
    scan64(c, c->bam_size.p, c->bam_local.p, c->bam_sums.p, d_total, n);
  }
  uint64_t h_total = 0;
  HIP_TRY(c, hipMemcpyAsync(&h_call, d_call, sizeof(h_call), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&h_total, d_total, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  for (int k = 0; k < 64; ++k) out->n_tagged += h_call.n_tagged[k];
  if (h_call.first_finding != ~0ull) {
    out->record = h_call.first_finding >> 8;
    out->code = (int32_t)(h_call.first_finding & 0xFF);
    return 0;  // (nothing is written for a stream the reference has no defined output for)
  }
  out->out_bytes = h_total;
  NEED(text_reserve(c, c->bt_text, &h_total, 1, &A.out));
  {
    ProfScope ps(c, "k_bt_emit");
    hipLaunchKernelGGL(k_bt_tile<true>, dim3(grid), dim3(kWave), lds, st, A);
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  HIP_TRY(c, hipGetLastError());
  text_publish(c->bt_text, &h_total, 1);
  return 0;
}

int fqg_bam_add_tags_output(fqg_ctx* c, void* host_dst, uint64_t nbytes) {
  if (!c) return FQG_ERR_ARG;
  return text_copy(c, c->bt_text, 0, host_dst, nbytes, "fqg_bam_add_tags_output: more than the last call produced");
}
