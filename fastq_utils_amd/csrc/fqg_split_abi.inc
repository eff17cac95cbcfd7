// fqg_split_abi.inc - fqg_records_split / fqg_records_split_output / fqg_records_split_info (include/fqg.h), included by
// fqg_abi.hip

extern "C++" {
namespace {
// FQGPU_SPLIT_T: records per tile (even, 2..64; measurement and tests only - results do not depend on it)
unsigned split_env_T() {
  static const unsigned v = [] {
    const char* e = getenv("FQGPU_SPLIT_T");
    const long t = e ? atol(e) : 0;
    return (unsigned)(t >= 2 && t <= 64 ? t & ~1l : 0);
  }();
  return v;
}
}  // namespace
}  // extern "C++"

int fqg_records_split(fqg_ctx* c, const fqg_frame* frame, uint64_t first_record, uint64_t n_rec, uint64_t out_bytes[2]) {
  if (!c || !frame || !out_bytes) return FQG_ERR_ARG;
  NEED(text_begin(c, c->bc_text));
  out_bytes[0] = out_bytes[1] = 0;
  c->split_info[0] = c->split_info[1] = c->split_info[2] = c->split_info[3] = 0;
  if (n_rec & 1) return fail(c, FQG_ERR_ARG, "fqg_records_split: an odd number of records");
  if (first_record > frame->fv.n_records || n_rec > frame->fv.n_records - first_record)
    return fail(c, FQG_ERR_ARG, "fqg_records_split: records beyond the frame");
  if (!n_rec) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t np = n_rec / 2, nb = scan64_spans(np);
  SplitArgs A;
  memset(&A, 0, sizeof(A));
  A.fv = frame->fv;
  A.first = first_record;
  A.n_rec = n_rec;
  A.has_nul = (frame->flags & kFlagNul) ? 1 : 0;  // lines are C strings then (bc_clip_nul)
  {
    // the LDS budget of a wavefront is the record filters' (bc_tile_one, FQGPU_BC_LDS); it holds the tile's span and,
    // behind it, the two images - together the span's bytes again
    const BcTile tc = bc_tile_one(frame->fv, 24576u);
    const unsigned budget = tc.in_cap + tc.out_cap;
    const double rec = (double)frame->fv.nbytes / (double)frame->fv.n_records;
    unsigned T = (unsigned)std::max(2.0, std::min(((double)budget - 160.0) / (2.12 * rec + 2.0), 64.0)) & ~1u;
    if (split_env_T()) T = split_env_T();
    A.T = T;
    A.in_cap = ((unsigned)(1.06 * rec * T + 96.0) + 15u) & ~15u;
    if (2u * A.in_cap + kSplitOutSlack > budget) A.in_cap = ((budget - kSplitOutSlack) / 2) & ~15u;
    A.out_cap = std::min(A.in_cap + kSplitOutSlack, budget - A.in_cap) & ~15u;
  }
  const uint64_t n_tiles = (n_rec + A.T - 1) / A.T;
  Scan64 S{};
  for (int s = 0; s < 2; ++s) {
    NEED(ensure(c, c->bc_len[1 + s], np * 4));
    NEED(ensure(c, c->bc_off[1 + s], np * 8));
    NEED(ensure(c, c->bc_sum[1 + s], nb * 8 + 32));
    S.in[s] = A.len[s] = (uint32_t*)c->bc_len[1 + s].p;
    S.local[s] = A.local[s] = (unsigned long long*)c->bc_off[1 + s].p;
    S.sums[s] = A.sums[s] = (unsigned long long*)c->bc_sum[1 + s].p;
  }
  NEED(ensure(c, c->bc_tile_big, n_tiles));
  S.total = (unsigned long long*)c->bc_sum[1].p + nb;  // (two words behind stream 0's span sums)
  A.tile_big = (uint8_t*)c->bc_tile_big.p;
  A.n_big = &c->d_bcall->big;
  NEED(bcall_reset(c, 0));
  {
    ProfScope ps(c, "k_split_plan");
    const unsigned grid = (unsigned)std::min<uint64_t>((n_rec + kBlock - 1) / kBlock, (uint64_t)c->cu_count * 32);
    hipLaunchKernelGGL(k_split_lens, dim3(grid), dim3(kBlock), 0, c->stream, A);
    scan64(c, S, 2, np);
    hipLaunchKernelGGL(k_split_tile_flags, dim3((unsigned)((n_tiles + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, A);
  }
  HIP_TRY(c, hipMemcpyAsync(c->h_bcall, c->d_bcall, sizeof(BcCall), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&c->h_scalar[2], S.total, 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  const uint64_t totals[3] = {0, c->h_scalar[2], c->h_scalar[3]};  // (streams 1 and 2, as the transform's two reads)
  const uint64_t n_big = c->h_bcall->big;
  uint8_t* text[3];
  NEED(text_reserve(c, c->bc_text, totals, 3, text));
  A.out[0] = text[1], A.out[1] = text[2];
  unsigned grid_t = 0;
  {
    ProfScope ps(c, "k_split_emit");
    // (16 workgroups per CU where the transform's and the filter's direct paths take 8: kept, the kernel sees the grid)
    grid_t = launch_tile_pair(c, k_split_emit_tile, n_big < n_tiles, n_tiles, A.in_cap + A.out_cap, k_split_emit_direct, n_big != 0,
                              n_rec, 16, A);
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  text_publish(c->bc_text, totals, 3);
  out_bytes[0] = totals[1], out_bytes[1] = totals[2];
  c->split_info[0] = n_tiles;
  c->split_info[1] = n_big;
  c->split_info[2] = grid_t;
  c->split_info[3] = A.T;
  return 0;
}

int fqg_records_split_output(fqg_ctx* c, int which, void* host_dst, uint64_t nbytes) {
  if (!c || which < 0 || which > 1) return FQG_ERR_ARG;
  return fqg_barcodes_output(c, 1 + which, host_dst, nbytes);
}

int fqg_records_split_info(const fqg_ctx* c, uint64_t info[4]) {
  if (!c || !info) return FQG_ERR_ARG;
  for (int i = 0; i < 4; ++i) info[i] = c->split_info[i];
  return 0;
}
