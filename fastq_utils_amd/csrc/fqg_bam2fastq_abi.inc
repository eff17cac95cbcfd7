// fqg_bam2fastq_abi.inc - fqg_bam2fastq / fqg_bam2fastq_output (include/fqg.h), included by fqg_abi.hip

extern "C++" {
namespace {
// the three launches over alignments [0, n) of a stream that is on the device already; with a finding nothing is emitted
int b2f_run(fqg_ctx* c, const uint8_t* d_buf, uint64_t nbytes, uint32_t n, double mean_in, const fqg_b2f_params* prm,
            fqg_b2f_result* out, B2fCall* h_call) {
  hipStream_t st = c->stream;
  const int ns = prm->tenx ? 3 : kB2fStreams;
  const uint64_t nb = scan64_spans(n);
  const size_t size_stride = (((size_t)n * 4) + 255) & ~(size_t)255, local_stride = (((size_t)n * 8) + 255) & ~(size_t)255;
  const size_t sums_stride = (((size_t)nb * 8) + 64 + 255) & ~(size_t)255;
  NEED(ensure(c, c->bam_size, size_stride * ns));
  NEED(ensure(c, c->bam_local, local_stride * ns));
  NEED(ensure(c, c->bam_sums, sums_stride * ns));
  NEED(ensure(c, c->b2f_call, sizeof(B2fCall) + 8 * kB2fStreams + 64));
  memset(h_call, 0xFF, sizeof(*h_call));
  B2fCall* d_call = (B2fCall*)c->b2f_call.p;
  unsigned long long* d_total = (unsigned long long*)((char*)c->b2f_call.p + sizeof(B2fCall));
  HIP_TRY(c, hipMemcpyAsync(d_call, h_call, sizeof(*h_call), hipMemcpyHostToDevice, st));
  // (the FASTQ text of a fastq2bam record is about twice its bytes: the names repeat in every stream)
  B2fTiles A;
  memset(&A, 0, sizeof(A));
  bam_tile_shape(A, kB2fInCap, kB2fOutCap, mean_in, 2.3 * mean_in, 16u * 2u * (uint32_t)ns, "FQGPU_B2F_T");
  A.buf = d_buf;
  A.nbytes = nbytes;
  A.offs = c->bam_offs;
  A.n = n;
  A.tenx = prm->tenx ? 1 : 0;
  A.n_streams = ns;
  A.call = d_call;
  Scan64 S{};
  for (int s = 0; s < ns; ++s) {
    A.size[s] = (uint32_t*)((char*)c->bam_size.p + size_stride * s);
    A.local[s] = (const unsigned long long*)((char*)c->bam_local.p + local_stride * s);
    A.sums[s] = (const unsigned long long*)((char*)c->bam_sums.p + sums_stride * s);
    S.in[s] = A.size[s];
    S.local[s] = (unsigned long long*)A.local[s];
    S.sums[s] = (unsigned long long*)A.sums[s];
  }
  S.total = d_total;
  const unsigned grid = (n + A.T - 1) / A.T;
  {
    ProfScope ps(c, "k_b2f_plan");
    hipLaunchKernelGGL(k_b2f_tile<false>, dim3(grid), dim3(kWave), A.in_cap + 64, st, A);
  }
  {
    ProfScope ps(c, "k_b2f_scan");
    scan64(c, S, ns, n);
  }
  uint64_t h_total[kB2fStreams] = {0, 0, 0, 0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(h_call, d_call, sizeof(*h_call), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h_total, d_total, 8 * (size_t)ns, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  HIP_TRY(c, hipGetLastError());
  if (h_call->first_finding != ~0ull) return 0;  // (the caller runs the alignments in front of the finding again)
  out->n_alignments = n;
  out->warn_record = h_call->warn_record;
  for (int s = 0; s < ns; ++s) {
    out->out_bytes[s] = h_total[s];
    out->first_record[s] = h_call->first_record[s];
  }
  NEED(text_reserve(c, c->b2f_text, h_total, ns, A.out));
  {
    ProfScope ps(c, "k_b2f_emit");
    hipLaunchKernelGGL(k_b2f_tile<true>, dim3(grid), dim3(kWave), A.in_cap + A.out_cap + 64, st, A);
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  HIP_TRY(c, hipGetLastError());
  text_publish(c->b2f_text, h_total, ns);
  return 0;
}
}  // namespace
}  // extern "C++"

int fqg_bam2fastq(fqg_ctx* c, const void* stream, uint64_t nbytes, int mem, const uint64_t* offsets, uint64_t n_records,
                  const fqg_b2f_params* prm, fqg_b2f_result* out) {
  const uint8_t* d_buf;
  uint64_t first_offset = 0;
  auto begin = [&] {
    memset(out, 0, sizeof(*out));
    out->warn_record = FQG_B2F_UNUSED;
    for (int s = 0; s < FQG_B2F_STREAMS; ++s) out->first_record[s] = FQG_B2F_UNUSED;
    return text_begin(c, c->b2f_text);
  };
  NEED(bam_input(c, "fqg_bam2fastq", out && prm, stream, nbytes, mem, offsets, n_records, begin, &d_buf, &first_offset));
  if (!n_records) return 0;
  const uint32_t n = (uint32_t)n_records;
  const double mean_in = (double)(nbytes - first_offset) / (double)n;
  B2fCall call;
  NEED(b2f_run(c, d_buf, nbytes, n, mean_in, prm, out, &call));
  if (call.first_finding != ~0ull) {
    // as the reference's exit at that alignment: the result and the streams are those of the alignments in front of it
    const uint64_t k = call.first_finding >> 32;
    const int32_t code = (int32_t)((call.first_finding >> 28) & 15u) | 16;  // (FQG_E_B2F_* are 24 .. 31)
    const uint64_t aux = call.first_finding & 0xFFFFFFFull;
    if (k) {
      B2fCall before;
      NEED(b2f_run(c, d_buf, nbytes, (uint32_t)k, mean_in, prm, out, &before));
      if (before.first_finding != ~0ull) return fail(c, FQG_ERR_ARG, "fqg_bam2fastq: the two passes disagree");
    }
    out->n_alignments = k;
    out->record = k;
    out->entry = prm->first_alignment + k + 1;
    out->code = code;
    uint64_t at = 0;
    if (code == FQG_E_B2F_SAMPLE_QUAL) {
      if (mem == FQG_MEM_DEVICE_INDEXED) {
        HIP_TRY(c, hipMemcpyAsync(&c->h_scalar[5], offsets + k, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        at = c->h_scalar[5];
      } else at = offsets[k];
    }
    out->aux = code == FQG_E_B2F_SAMPLE_QUAL ? at + aux : 0;
  }
  return 0;
}

int fqg_bam2fastq_output(fqg_ctx* c, int stream_id, void* host_dst, uint64_t nbytes) {
  if (!c) return FQG_ERR_ARG;
  return text_copy(c, c->b2f_text, stream_id, host_dst, nbytes, "fqg_bam2fastq_output: more than the last call produced");
}
