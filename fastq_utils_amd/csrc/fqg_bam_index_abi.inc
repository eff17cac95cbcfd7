// fqg_bam_index_abi.inc - fqg_bam_header_end, fqg_bam_index_device, fqg_bam_index_offsets, fqg_bam_index_output
// (include/fqg.h), included by fqg_abi.hip

extern "C++" {
namespace {

// FQGPU_BAMIDX_SEG / _RING / _WINDOW: the geometry, for tests and A/B; results do not depend on it
uint64_t bx_env(const char* name, uint64_t dflt, uint64_t lo, uint64_t hi) {
  const char* e = getenv(name);
  const uint64_t v = e && *e ? strtoull(e, nullptr, 10) : dflt;
  return std::max(lo, std::min(hi, v));
}
constexpr uint64_t kBxSegDefault = 256u << 10, kBxWindowDefault = 128u << 20;
constexpr uint32_t kBxRingDefault = 8192;

}  // namespace
}  // extern "C++"

// The header walk of fqg_bam_index_records (fqg_umi_abi.inc), over a prefix: the same tests in the same order, each
// against the total length first (the verdict) and against what is there second (the question for more).
int fqg_bam_header_end(const void* prefix, uint64_t have, uint64_t nbytes_total, uint64_t* first_record, uint64_t* need) {
  if (!first_record || !need || (!prefix && have) || have > nbytes_total) return FQG_ERR_ARG;
  const uint8_t* b = (const uint8_t*)prefix;
  *first_record = *need = 0;
  if (nbytes_total < 12) return FQG_ERR_ARG;
  if (have < 12) {
    *need = 12;
    return FQG_NEED_MORE;
  }
  if (memcmp(b, "BAM\1", 4) != 0) return FQG_ERR_ARG;
  uint64_t p = 8 + (uint64_t)(uint32_t)fqg::bx::bx_rd32(b + 4);
  if (p + 4 > nbytes_total) return FQG_ERR_ARG;
  if (p + 4 > have) {
    *need = p + 4;
    return FQG_NEED_MORE;
  }
  const int32_t n_ref = fqg::bx::bx_rd32(b + p);
  p += 4;
  if (n_ref < 0) return FQG_ERR_ARG;
  for (int32_t i = 0; i < n_ref; ++i) {
    if (p + 4 > nbytes_total) return FQG_ERR_ARG;
    if (p + 4 > have) {
      *need = p + 4;
      return FQG_NEED_MORE;
    }
    p += 4 + (uint64_t)(uint32_t)fqg::bx::bx_rd32(b + p) + 4;
  }
  if (p > nbytes_total) return FQG_ERR_ARG;
  *first_record = p;
  return 0;
}

int fqg_bam_index_device(fqg_ctx* c, const void* stream_dev, uint64_t nbytes, uint64_t first_record, fqg_bam_index_result* out) {
  if (!c || !out || (!stream_dev && nbytes) || first_record > nbytes) return FQG_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  c->bx_valid = false;
  c->bx_n = 0;
  memset(out, 0, sizeof(*out));
  const uint64_t span = nbytes - first_record;
  const uint64_t seg = bx_env("FQGPU_BAMIDX_SEG", kBxSegDefault, 64, bx::kBxMaxSeg);
  uint32_t ring = bx::kBxMinRing;  // a power of two
  while (ring < bx_env("FQGPU_BAMIDX_RING", kBxRingDefault, bx::kBxMinRing, bx::kBxMaxRing)) ring <<= 1;
  uint64_t window = bx_env("FQGPU_BAMIDX_WINDOW", kBxWindowDefault, seg, 1ull << 40);
  window = (window + seg - 1) / seg * seg;  // whole segments
  const uint64_t win = std::max<uint64_t>(1, std::min(window, span));
  const uint64_t cap = span / bx::kBxMinStep + 1, stretch_cap = bx::bx_max_stretches(win, seg, ring);
  NEED(ensure(c, c->bx_offsets, cap * 8));
  NEED(ensure(c, c->bx_entries, win * 4));
  NEED(ensure(c, c->bx_counts, win * 2));
  NEED(ensure(c, c->bx_stretch, stretch_cap * sizeof(bx::BxStretch)));
  NEED(ensure(c, c->bx_state, sizeof(bx::BxState)));
  NEED(raise_dynamic_lds(c, (const void*)k_bamidx_tables, bx_lds_bytes(ring)));
  bx::BxState h_state;
  memset(&h_state, 0, sizeof(h_state));
  h_state.p = first_record;
  HIP_TRY(c, hipMemcpyAsync(c->bx_state.p, &h_state, sizeof(h_state), hipMemcpyHostToDevice, c->stream));
  BxArgs A;
  memset(&A, 0, sizeof(A));
  A.stream = (const uint8_t*)stream_dev;
  A.nbytes = nbytes;
  A.seg = seg;
  A.ring = ring;
  A.entries = (uint32_t*)c->bx_entries.p;
  A.counts = (uint16_t*)c->bx_counts.p;
  A.stretch = (bx::BxStretch*)c->bx_stretch.p;
  A.stretch_cap = stretch_cap;
  A.state = (bx::BxState*)c->bx_state.p;
  A.offsets = (unsigned long long*)c->bx_offsets.p;
  A.offsets_cap = cap;
  for (uint64_t w_lo = first_record; w_lo < nbytes; w_lo += window) {
    A.w_lo = w_lo;
    A.w_hi = std::min(nbytes, w_lo + window);
    {
      ProfScope ps(c, "k_bamidx_tables");
      hipLaunchKernelGGL(k_bamidx_tables, dim3((unsigned)((A.w_hi - w_lo + seg - 1) / seg)), dim3(kBxBlock), bx_lds_bytes(ring), c->stream, A);
    }
    {
      ProfScope ps(c, "k_bamidx_follow");
      hipLaunchKernelGGL(k_bamidx_follow, dim3(1), dim3(kBxBlock), 0, c->stream, A);
    }
    {
      ProfScope ps(c, "k_bamidx_offsets");
      hipLaunchKernelGGL(k_bamidx_offsets, dim3((unsigned)((stretch_cap + kBxBlock - 1) / kBxBlock)), dim3(kBxBlock), 0, c->stream, A);
    }
  }
  HIP_TRY(c, hipMemcpyAsync(&h_state, c->bx_state.p, sizeof(h_state), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  if (h_state.overflow) return fail(c, FQG_ERR_STATE, "fqg_bam_index_device: more stretches in a window than its bound");
  if (h_state.k > cap) return fail(c, FQG_ERR_STATE, "fqg_bam_index_device: more records than the stream has room for");
  out->n_records = h_state.k;
  out->used = h_state.p;  // (where the rule said stop, or the end of the stream)
  c->bx_n = h_state.k;
  c->bx_valid = true;
  return 0;
}

const uint64_t* fqg_bam_index_offsets(const fqg_ctx* c) { return c && c->bx_valid ? (const uint64_t*)c->bx_offsets.p : nullptr; }

int fqg_bam_index_output(fqg_ctx* c, uint64_t first, uint64_t* host_dst, uint64_t n) {
  if (!c || (!host_dst && n)) return FQG_ERR_ARG;
  if (!c->bx_valid) return fail(c, FQG_ERR_STATE, "fqg_bam_index_output: no index");
  if (first > c->bx_n || n > c->bx_n - first) return fail(c, FQG_ERR_ARG, "fqg_bam_index_output: more than was produced");
  if (!n) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(host_dst, (const uint64_t*)c->bx_offsets.p + first, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}
