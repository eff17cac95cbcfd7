// fqg_text_out.inc - the output text of a call that stays on the device until an `_output` call copies it (OutText,
// fqg_abi.hip), and the 64-bit scan that lays it out.  What fqg_barcodes_transform, fqg_records_filter / _gather /
// _split, fqg_bam_add_tags and fqg_bam2fastq share; included by fqg_abi.hip behind `ensure` and ProfScope.
//
// A producer:  text_begin ... plan, scan64, totals to the host ... text_reserve ... emit ... text_publish.
// A call that fails or returns early in between leaves the counts at 0: nothing of it can be copied.

// ---- the scan: k_scan64_a / _b (fqg_tile.h) on c->stream ------------------------------------------
// spans of n lengths: the span sums a scan needs room for (an empty array has one: its total is still written)
inline uint64_t scan64_spans(uint64_t n) { return (std::max<uint64_t>(n, 1) + kScan64Span - 1) / kScan64Span; }

// `ns` scans of n lengths each in one launch pair
void scan64(fqg_ctx* c, const Scan64& t, int ns, uint64_t n) {
  const uint64_t nb = scan64_spans(n);
  hipLaunchKernelGGL(k_scan64_a, dim3((unsigned)nb, (unsigned)ns), dim3(kBlock), 0, c->stream, t, n);
  hipLaunchKernelGGL(k_scan64_b, dim3(1, (unsigned)ns), dim3(kBlock), 0, c->stream, t, nb);
}
// ... and a single one
void scan64(fqg_ctx* c, const void* in, void* local, void* sums, unsigned long long* total, uint64_t n) {
  Scan64 t{};
  t.in[0] = (const uint32_t*)in;
  t.local[0] = (unsigned long long*)local;
  t.sums[0] = (unsigned long long*)sums;
  t.total = total;
  scan64(c, t, 1, n);
}

// ---- the store -----------------------------------------------------------------------------------
int text_wait(fqg_ctx* c, OutText& o) {
  if (!o.pending) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(o.copy_stream));
  o.pending = false;
  return 0;
}

// what every producer opens with
int text_begin(fqg_ctx* c, OutText& o) {
  NEED(text_wait(c, o));  // (a copy of the previous output is still on its way: this call writes the same buffers)
  for (uint64_t& b : o.bytes) b = 0;
  return 0;
}

// Room for streams [0, ns) of totals[s] bytes, out[s]: where stream s starts.  Every stream starts on a 256-byte
// boundary and has 64 bytes behind its text: the tile kernels write whole 16-byte words (emit_flush).
int text_reserve(fqg_ctx* c, OutText& o, const uint64_t* totals, int ns, uint8_t** out) {
  size_t at = 0;
  for (int s = 0; s < ns; ++s) {
    o.at[s] = at;
    at += ((size_t)totals[s] + 64 + 255) & ~(size_t)255;
  }
  NEED(ensure(c, o.buf, at + 64));
  for (int s = 0; s < ns; ++s) out[s] = (uint8_t*)o.buf.p + o.at[s];
  return 0;
}

void text_publish(OutText& o, const uint64_t* totals, int ns) {
  for (int s = 0; s < ns; ++s) o.bytes[s] = totals[s];
}

void text_release(OutText& o) {
  release(o.buf);
  for (uint64_t& b : o.bytes) b = 0;
}

// the first nbytes of stream s to the host; `too_much`: the caller's message for more than was produced
int text_copy(fqg_ctx* c, OutText& o, int s, void* host_dst, uint64_t nbytes, const char* too_much) {
  if (s < 0 || s >= FQG_B2F_STREAMS || (!host_dst && nbytes)) return FQG_ERR_ARG;
  if (nbytes > o.bytes[s]) return fail(c, FQG_ERR_ARG, too_much);
  if (!nbytes) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(host_dst, (const uint8_t*)o.buf.p + o.at[s], nbytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ... the same on a stream of the store's own, beside what the caller does next; text_wait (or the next producer's
// text_begin) waits for it
int text_copy_begin(fqg_ctx* c, OutText& o, int s, void* host_dst, uint64_t nbytes, const char* too_much) {
  if (s < 0 || s >= FQG_B2F_STREAMS || (!host_dst && nbytes)) return FQG_ERR_ARG;
  if (nbytes > o.bytes[s]) return fail(c, FQG_ERR_ARG, too_much);
  if (!nbytes) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!o.copy_stream) {
    HIP_TRY(c, hipStreamCreateWithFlags(&o.copy_stream, hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreateWithFlags(&o.ready, hipEventDisableTiming));
  }
  HIP_TRY(c, hipEventRecord(o.ready, c->stream));  // (what produced the text has been launched on `stream`)
  HIP_TRY(c, hipStreamWaitEvent(o.copy_stream, o.ready, 0));
  HIP_TRY(c, hipMemcpyAsync(host_dst, (const uint8_t*)o.buf.p + o.at[s], nbytes, hipMemcpyDeviceToHost, o.copy_stream));
  o.pending = true;
  return 0;
}

// ---- the small pieces beside them -----------------------------------------------------------------
// A persistent grid of one-wavefront workgroups: exactly the wavefronts that are resident at once (tiles are dealt
// round-robin, so a wavefront that starts late would do its whole share after the others have finished).
// FQGPU_TILE_WAVES=n (n >= 1) caps the grid: a wavefront then walks many tiles of a small image (measurement and tests
// only - results do not depend on it).
unsigned resident_waves(fqg_ctx* c, const void* kernel, unsigned lds) {
  static const unsigned env_cap = [] {
    const char* e = getenv("FQGPU_TILE_WAVES");
    const long v = e ? atol(e) : 0;
    return (unsigned)(v >= 1 && v <= 0x7FFFFFFFl ? v : 0);
  }();
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kWave, lds) != hipSuccess || per_cu < 1) per_cu = 1;
  const unsigned waves = (unsigned)per_cu * (unsigned)c->cu_count;
  return env_cap ? std::min(env_cap, waves) : waves;
}
// The launch pair of a tile emitter, both kernels on the same arguments: `tile` on the resident grid for the tiles that fit
// LDS, `direct` (direct_per_cu workgroups per CU) record by record for those that do not.  -> the tile kernel's grid or 0
template <class KT, class KD, class... A>
unsigned launch_tile_pair(fqg_ctx* c, KT tile, bool tiles, uint64_t n_tiles, unsigned lds, KD direct, bool big, uint64_t n_rec,
                          unsigned direct_per_cu, const A&... args) {
  const unsigned grid_t = tiles ? (unsigned)std::min<uint64_t>(n_tiles, resident_waves(c, (const void*)tile, lds)) : 0u;
  const unsigned grid_e = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_rec + 3) / 4, (uint64_t)c->cu_count * direct_per_cu));
  if (tiles) hipLaunchKernelGGL(tile, dim3(grid_t), dim3(kWave), lds, c->stream, args...);
  if (big) hipLaunchKernelGGL(direct, dim3(grid_e), dim3(kBlock), 0, c->stream, args...);
  return grid_t;
}

// the call's counters zeroed on the device; `none`: what first_finding and first_discard start from
int bcall_reset(fqg_ctx* c, unsigned long long none) {
  BcCall z;
  memset(&z, 0, sizeof(z));
  z.first_finding = z.first_discard = none;
  *c->h_bcall = z;
  HIP_TRY(c, hipMemcpyAsync(c->d_bcall, c->h_bcall, sizeof(BcCall), hipMemcpyHostToDevice, c->stream));
  return 0;
}
// the scan totals of a call live in the 64 bytes behind its BcCall, on the device and in the pinned copy
unsigned long long* bcall_totals(BcCall* call) {
  return reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(call) + sizeof(BcCall));
}
