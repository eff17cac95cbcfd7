// fqg_barcode_abi.inc - host side of the barcode kernels: fqg_barcodes_transform, the census of what it kept
// (fqg_census_*, fqg_barcodes_census) and the whitelist (fqg_whitelist_*, fqg_barcodes_whitelist[_correct]).  Included by
// fqg_abi.hip inside extern "C", in front of the per-record filters: bc_tile_one is theirs and fqg_split_abi.inc's.
// fqg_barcodes_transform is its phases in order (bc_prepare, bc_plan, bc_lay_out, bc_emit, bc_cut_at_finding) on one
// BcBatch; the order of launches, memsets, copies and synchronisations on the stream is the order of the text.
// ---- barcode extraction ----------------------------------------------------------------------
// Tile geometry: T iterations whose records (`in` bytes an iteration, of `files` files) and output text (`out` bytes) fit
// the LDS budget of a wavefront, from mean sizes (a tile that does not fit takes the direct path).  FQGPU_BC_LDS: the budget.
static BcTile bc_tile_budget(double in, double out, int files, unsigned lanes_per_iter, unsigned default_budget) {
  static const unsigned env_budget = [] {
    const char* e = getenv("FQGPU_BC_LDS");
    const long v = e ? atol(e) : 0;
    return (unsigned)(v >= 4096 && v <= 65536 ? v : 0);
  }();
  const unsigned budget = env_budget ? env_budget : default_budget;
  const double fixed = 48.0 * files + 96.0;
  double t = ((double)budget - fixed) / (1.06 * (in + out) + 1.0);
  unsigned T = (unsigned)std::max(1.0, std::min(t, 64.0 / lanes_per_iter));
  BcTile tc;
  tc.T = T;
  tc.in_cap = ((unsigned)(1.06 * in * T + 48.0 * files + 48.0) + 15u) & ~15u;
  if (tc.in_cap + 1024u > budget) tc.in_cap = (budget / 2) & ~15u;
  tc.out_cap = (budget - tc.in_cap) & ~15u;
  tc.plan_m = 1;
  tc.plan_cap = 64;
  return tc;
}
// ... of the kernels that read one file and write its records as FASTQ text (the record filters, the split)
static BcTile bc_tile_one(const FrameView& fv, unsigned default_budget) {
  const double rec = fv.n_records ? (double)fv.nbytes / (double)fv.n_records : 0.0;
  return bc_tile_budget(rec, rec + 100, 1, 1, default_budget);
}
// ... of the transform
static BcTile bc_tile_for(const BcParams& P, unsigned default_budget = 20480u) {
  double in = 0, out_sam = 0, out_fq = 0;
  int files = 0;
  for (int x = 1; x < kBcFiles; ++x) {
    if (!P.f[x].present) continue;
    const double rec = P.f[x].fv.n_records ? (double)P.f[x].fv.nbytes / (double)P.f[x].fv.n_records : 0.0;
    in += rec * P.f[x].step;
    ++files;
    if (x <= 2) {
      out_sam += 1.35 * rec + 130;
      if (P.emit[x]) out_fq = std::max(out_fq, rec + 100);
    }
  }
  BcTile tc = bc_tile_budget(in, P.out_sam ? out_sam : out_fq, files, P.out_sam && P.f[2].present ? 2 : 1, default_budget);
  // the plan kernel: several tiles at once while one lane per iteration allows it.  It stages only the files a
  // barcode is cut from, and only when a minimum quality makes it read their bytes (bc_staged<PLAN>)
  tc.plan_m = std::max(1u, std::min(64u / tc.T, 4u));
  double plan_in = 0;
  int plan_files = 0;
  for (int x = 1; x < kBcFiles; ++x)
    if (P.f[x].present && P.min_qual > 0 && (P.umi_read == x || P.cell_read == x || P.sample_read == x)) {
      plan_in += (P.f[x].fv.n_records ? (double)P.f[x].fv.nbytes / (double)P.f[x].fv.n_records : 0.0) * P.f[x].step;
      ++plan_files;
    }
  tc.plan_cap = ((unsigned)(1.06 * plan_in * tc.T * tc.plan_m + 48.0 * plan_files + 64.0) + 15u) & ~15u;
  while (tc.plan_m > 1 && tc.plan_cap > 32768u) {  // (long reads in a barcode file)
    tc.plan_cap = (tc.plan_cap / tc.plan_m * (tc.plan_m - 1) + 15u) & ~15u;
    --tc.plan_m;
  }
  tc.plan_cap = std::min(tc.plan_cap, 65536u - 256u);
  return tc;
}

// the kernels' view of one batch (shared by the transform and the census of what it kept)
static int bc_make_params(fqg_ctx* c, const fqg_frame* const frames[6], const fqg_file_state states[6],
                          const uint64_t first_record[6], const fqg_barcode_params* bp, uint64_t n_iter,
                          uint64_t first_read_number, BcParams& P, bool& inter) {
  memset(&P, 0, sizeof(P));
  inter = bp->interleaved[0] != 0 || bp->interleaved[1] != 0;
  for (int x = 1; x < kBcFiles; ++x) {
    if (!bp->present[x]) continue;
    if (!frames[x]) return fail(c, FQG_ERR_ARG, "fqg_barcodes_transform: missing frame");
    BcFile& f = P.f[x];
    f.fv = frames[x]->fv;
    // NUL bytes (and the "\0\n" behind a piece of a line cut at the gzgets limits): lines are C strings (bc_clip_nul)
    f.has_nul = (frames[x]->flags & kFlagNul) ? 1 : 0;
    P.has_nul |= f.has_nul;
    f.first = first_record[x];
    f.present = 1;
    f.fmt = states[x].readname_format;
    f.step = 1;
    f.add = 0;
    if (inter && (x == bp->interleaved[0] || x == bp->interleaved[1])) {
      f.step = 2;
      f.add = x == bp->interleaved[1] ? 1 : 0;
    }
    // every record the batch touches must exist
    if (n_iter && f.first + (n_iter - 1) * f.step + f.add >= f.fv.n_records)
      return fail(c, FQG_ERR_ARG, "fqg_barcodes_transform: iterations beyond a frame");
    P.n_inputs++;
  }
  if (!P.f[1].present) return fail(c, FQG_ERR_ARG, "fqg_barcodes_transform: read1 is required");
  for (int x = 1; x <= 2; ++x)
    if (((bp->out_sam && x == 1) || (!bp->out_sam && bp->emit[x])) && !P.f[x].present)
      return fail(c, FQG_ERR_ARG, "fqg_barcodes_transform: output requested for an absent input");
  if (bp->out_sam < 0 || bp->out_sam > FQG_OUT_BAM) return fail(c, FQG_ERR_ARG, "fqg_barcodes_transform: out_sam is 0, 1 or 2");
  const int64_t sizes[3] = {bp->umi_size, bp->cell_size, bp->sample_size};
  for (int i = 0; i < 3; ++i)
    if (sizes[i] < 0 || sizes[i] >= 50) return fail(c, FQG_ERR_ARG, "barcode sizes must be 0..49 (MAX_BARCODE_LENGTH)");
  P.umi_read = bp->umi_read;
  P.cell_read = bp->cell_read;
  P.sample_read = bp->sample_read;
  P.phred = bp->phred_encoding;
  P.min_qual = bp->min_qual;
  P.out_sam = bp->out_sam;
  P.tenx = bp->tenx;
  {
    static const int abl = measure_int("FQGPU_BC_ABL");
    P.ablate = abl;
  }
  P.umi_off = bp->umi_offset;
  P.umi_size = bp->umi_size;
  P.cell_off = bp->cell_offset;
  P.cell_size = bp->cell_size;
  P.sample_off = bp->sample_offset;
  P.sample_size = bp->sample_size;
  for (int x = 0; x < 3; ++x) {
    P.emit[x] = bp->emit[x];
    P.read_off[x] = bp->read_offset[x];
    P.read_size[x] = bp->read_size[x];
  }
  P.first_read_number = first_read_number;
  return 0;
}

extern "C++" {
namespace {

// one batch of fqg_barcodes_transform on its way through the phases
struct BcBatch {
  BcParams P;
  BcTile tc;
  int file_mask = 0;  // bit x: input x is present
  bool inter = false;
  uint64_t n_iter = 0;
  uint64_t n_done = 0;  // iterations the batch reaches: all, or up to the first discard of interleaved input
};

// the usual sets of inputs have kernels of their own (bc_has): f(std::integral_constant<int, MASK>)
template <class F>
void bc_with_mask(int file_mask, F f) {
  switch (file_mask) {
    case 0x02: f(std::integral_constant<int, 0x02>{}); break;
    case 0x06: f(std::integral_constant<int, 0x06>{}); break;
    case 0x0A: f(std::integral_constant<int, 0x0A>{}); break;
    case 0x0E: f(std::integral_constant<int, 0x0E>{}); break;
    default: f(std::integral_constant<int, 0>{}); break;
  }
}
// ... and the three kinds of output: f(std::integral_constant<int, kEmit*>)
template <class F>
void bc_with_kind(int out_sam, F f) {
  if (out_sam == FQG_OUT_BAM) f(std::integral_constant<int, kEmitBam>{});
  else if (out_sam) f(std::integral_constant<int, kEmitSam>{});
  else f(std::integral_constant<int, kEmitFastq>{});
}

// output i is produced (the others have no lengths and no text)
bool bc_produced(const BcParams& P, int i) { return P.out_sam ? i == 0 : P.emit[i] != 0; }

// the call's counters as the device has them now, `more` bytes behind them too (bcall_totals)
int bcall_fetch(fqg_ctx* c, size_t more = 0) {
  HIP_TRY(c, hipMemcpyAsync(c->h_bcall, c->d_bcall, sizeof(BcCall) + more, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

// the discards among the first n iterations counted again (the plan counted those of all n_iter)
int bc_recount(fqg_ctx* c, uint64_t n) {
  HIP_TRY(c, hipMemsetAsync(&c->d_bcall->discarded, 0, 2 * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(k_bc_count, dim3((unsigned)std::min<uint64_t>((n + kBlock - 1) / kBlock, 2048)), dim3(kBlock), 0, c->stream,
                     (const uint8_t*)c->bc_status.p, n, c->d_bcall);
  return 0;
}

// arguments, parameters, buffers, counters, tile.  Nothing behind it runs for an empty batch.
int bc_prepare(fqg_ctx* c, const fqg_frame* const frames[6], const fqg_file_state states[6], const uint64_t first_record[6],
               const fqg_barcode_params* bp, uint64_t n_iter, uint64_t first_read_number, BcBatch& B) {
  c->bc_status_valid = 0;
  HIP_TRY(c, hipSetDevice(c->device));
  NEED(bc_make_params(c, frames, states, first_record, bp, n_iter, first_read_number, B.P, B.inter));
  B.n_iter = B.n_done = n_iter;
  if (!n_iter) return 0;
  NEED(ensure(c, c->bc_status, n_iter));
  for (int i = 0; i < 3; ++i) {
    NEED(ensure(c, c->bc_len[i], n_iter * 4));
    NEED(ensure(c, c->bc_off[i], n_iter * 8));
    NEED(ensure(c, c->bc_sum[i], scan64_spans(n_iter) * 8));
  }
  NEED(bcall_reset(c, ~0ull));
  B.tc = bc_tile_for(B.P);
  for (int x = 1; x < kBcFiles; ++x)
    if (B.P.f[x].present) B.file_mask |= 1 << x;
  return ensure(c, c->bc_tile_big, (n_iter + B.tc.T - 1) / B.tc.T);
}

// status and output lengths of every iteration, the tiles that do not fit LDS; where interleaved input ends the batch
int bc_plan(fqg_ctx* c, BcBatch& B) {
  const BcTile& tc = B.tc;
  const uint64_t n_tiles = (B.n_iter + tc.T - 1) / tc.T;
  {
    ProfScope ps(c, "k_bc_plan");
    bc_with_mask(B.file_mask, [&](auto mask) {
      bc_with_kind(B.P.out_sam, [&](auto kind) {
        const auto kernel = k_bc_plan_tile<decltype(mask)::value, decltype(kind)::value == kEmitBam>;
        const uint64_t plan_tiles = (n_tiles + tc.plan_m - 1) / tc.plan_m;
        const unsigned grid = (unsigned)std::min<uint64_t>(plan_tiles, resident_waves(c, (const void*)kernel, tc.plan_cap));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kWave), tc.plan_cap, c->stream, B.P, tc, B.n_iter, (uint8_t*)c->bc_status.p,
                           (uint32_t*)c->bc_len[0].p, (uint32_t*)c->bc_len[1].p, (uint32_t*)c->bc_len[2].p,
                           (uint8_t*)c->bc_tile_big.p, c->d_bcall);
      });
    });
  }
  NEED(bcall_fetch(c));
  // interleaved input re-synchronises behind the first discard: nothing beyond it is reached in this batch (a name
  // finding - the emit kernels look for those - can only lie in what is emitted)
  if (B.inter && c->h_bcall->first_discard < B.n_done) B.n_done = c->h_bcall->first_discard + 1;
  return 0;
}

// where every record of every output goes (scan64), the outputs' sizes, the discards of what the batch reaches
int bc_lay_out(fqg_ctx* c, const BcBatch& B, fqg_barcode_result* out, uint64_t totals[3]) {
  unsigned long long* d_tot = bcall_totals(c->d_bcall);
  out->n_done = B.n_done;
  {
    ProfScope ps(c, "k_bc_scan");
    if (B.n_done != B.n_iter) NEED(bc_recount(c, B.n_done));
    HIP_TRY(c, hipMemsetAsync(d_tot, 0, 3 * sizeof(unsigned long long), c->stream));
    for (int i = 0; i < 3; ++i)
      if (bc_produced(B.P, i)) scan64(c, c->bc_len[i].p, c->bc_off[i].p, c->bc_sum[i].p, d_tot + i, B.n_done);
  }
  NEED(bcall_fetch(c, 64));
  out->n_discarded = c->h_bcall->discarded;
  out->n_short = c->h_bcall->short_warnings;
  for (int i = 0; i < 3; ++i) out->out_bytes[i] = totals[i] = bcall_totals(c->h_bcall)[i];
  return 0;
}

// the text: tile by tile, and record by record for the tiles that do not fit LDS
int bc_emit(fqg_ctx* c, const BcBatch& B, const uint64_t totals[3]) {
  const BcTile& tc = B.tc;
  const uint64_t n_big = c->h_bcall->big;  // (the plan's count: nothing behind the plan writes it)
  uint8_t* text[3];
  NEED(text_reserve(c, c->bc_text, totals, 3, text));
  text_publish(c->bc_text, totals, 3);
  {
    ProfScope ps(c, "k_bc_emit");
    EmitOut eo[3];
    for (int i = 0; i < 3; ++i)
      eo[i] = EmitOut{(const uint32_t*)c->bc_len[i].p, (const unsigned long long*)c->bc_off[i].p,
                      (const unsigned long long*)c->bc_sum[i].p, text[i]};
    const uint64_t n_tiles_done = (B.n_done + tc.T - 1) / tc.T;
    const unsigned lds = tc.in_cap + tc.out_cap;
    const auto status = (const uint8_t*)c->bc_status.p, big = (const uint8_t*)c->bc_tile_big.p;
    bc_with_kind(B.P.out_sam, [&](auto kind) {
      unsigned grid_t = 1;
      bc_with_mask(B.file_mask, [&](auto mask) {
        grid_t = launch_tile_pair(c, k_bc_emit_tile<decltype(kind)::value, decltype(mask)::value>, true, n_tiles_done, lds,
                                  k_bc_emit_direct<decltype(kind)::value == kEmitBam>, n_big != 0, B.n_done, 8, B.P, tc, B.n_done,
                                  status, big, eo[0], eo[1], eo[2], c->d_bcall);
      });
      if (getenv("FQGPU_BC_DEBUG"))
        fprintf(stderr, "fqgpu barcodes: T=%u in_cap=%u out_cap=%u emit grid=%u (%u/CU) big tiles=%llu\n", tc.T, tc.in_cap,
                tc.out_cap, grid_t, grid_t / (unsigned)c->cu_count, (unsigned long long)n_big);
    });
  }
  NEED(bcall_fetch(c));
  HIP_TRY(c, hipGetLastError());
  return 0;
}

// Names that do not agree (or a header without '@') at iteration k: the reference stops there, before it looks at the
// iteration's barcodes.  What the batch yields is what lies in front of k: the text up to k's place in every output,
// the discards among the first k iterations.  (A refused BAM record is found by the plan, which looks at all n_iter
// iterations: one behind where interleaved input re-synchronises is none.)
int bc_cut_at_finding(fqg_ctx* c, const BcBatch& B, fqg_barcode_result* out, uint64_t totals[3]) {
  const unsigned long long finding = c->h_bcall->first_finding;
  const uint64_t k = finding >> 8;
  if (finding == ~0ull || k >= B.n_done) return 0;
  out->iteration = k;
  out->code = (int32_t)((finding & 0xFF) >> 3);
  if (out->code == (int32_t)kBcFindBam) out->code = FQG_E_BAM_RECORD;
  out->file = (int32_t)(finding & 7);
  out->n_done = k;
  out->n_discarded = out->n_short = 0;
  for (int i = 0; i < 3; ++i) {
    if (!bc_produced(B.P, i)) continue;
    unsigned long long off = 0, sum = 0;
    if (k) {  // (k < n_done: both entries exist)
      HIP_TRY(c, hipMemcpy(&off, (const unsigned long long*)c->bc_off[i].p + k, 8, hipMemcpyDeviceToHost));
      HIP_TRY(c, hipMemcpy(&sum, (const unsigned long long*)c->bc_sum[i].p + k / kScan64Span, 8, hipMemcpyDeviceToHost));
    }
    out->out_bytes[i] = totals[i] = off + sum;
  }
  text_publish(c->bc_text, totals, 3);
  if (k) {
    NEED(bc_recount(c, k));
    NEED(bcall_fetch(c));
    out->n_discarded = c->h_bcall->discarded;
    out->n_short = c->h_bcall->short_warnings;
  }
  return 0;
}

}  // namespace
}  // extern "C++"

int fqg_barcodes_transform(fqg_ctx* c, const fqg_frame* const frames[6], const fqg_file_state states[6],
                           const uint64_t first_record[6], const fqg_barcode_params* bp, uint64_t n_iter,
                           uint64_t first_read_number, fqg_barcode_result* out) {
  if (!c || !frames || !states || !first_record || !bp || !out) return FQG_ERR_ARG;
  NEED(text_begin(c, c->bc_text));
  memset(out, 0, sizeof(*out));
  BcBatch B;
  uint64_t totals[3];
  NEED(bc_prepare(c, frames, states, first_record, bp, n_iter, first_read_number, B));
  if (!n_iter) return 0;
  NEED(bc_plan(c, B));
  NEED(bc_lay_out(c, B, out, totals));
  NEED(bc_emit(c, B, totals));
  NEED(bc_cut_at_finding(c, B, out, totals));
  c->bc_status_valid = out->n_done;  // (fqg_barcodes_census: the status bytes of the iterations this batch yielded)
  return 0;
}

// the text of the last call that left some (the transform, the record filters, the gather, the split)
int fqg_barcodes_output(fqg_ctx* c, int which, void* host_dst, uint64_t nbytes) {
  if (!c || which < 0 || which > 2) return FQG_ERR_ARG;
  return text_copy(c, c->bc_text, which, host_dst, nbytes, "fqg_barcodes_output: more than was produced");
}

int fqg_barcodes_output_wait(fqg_ctx* c) { return c ? text_wait(c, c->bc_text) : (int)FQG_ERR_ARG; }

int fqg_barcodes_output_begin(fqg_ctx* c, int which, void* host_dst, uint64_t nbytes) {
  if (!c || which < 0 || which > 2) return FQG_ERR_ARG;
  return text_copy_begin(c, c->bc_text, which, host_dst, nbytes, "fqg_barcodes_output_begin: more than was produced");
}

// ---- census of what the transform kept (fqg_census_kernels.hip) -------------------------------------
struct fqg_whitelist {
  fqg_ctx* ctx = nullptr;
  DevBuf set;
  uint64_t capacity = 0;
};

struct fqg_census {
  fqg_ctx* ctx = nullptr;
  DevBuf cells, umis;     // the pairs, in arrival order until fqg_census_finish sorts them
  DevBuf cells2, umis2, tmp, flag, local, sums, lines;
  unsigned long long* d_count = nullptr;
  uint64_t n_pairs = 0, n_cells = 0;
  unsigned umi_bits = 1, cell_bits = 1;  // bits the packed values of the batches so far can need (census_bits)
  bool finished = false;
  const struct fqg_whitelist* wl = nullptr;  // fqg_census_set_whitelist: the caller's, alive while it is attached
  int max_mismatch = 0;
  // fqg_census_collapse_umis (fqg_census_umi_kernels.hip): the table of distinct (cell, UMI) rows and what led to it
  bool umi_wide = false;   // a umi_size outside 1..19 was seen: the values may have twenty digits
  bool collapsed = false;  // the last collapse call's results stand in u_table / u_cell_roots
  uint64_t n_umis = 0;
  DevBuf u_flag, u_local, u_sums, u_tot, u_umi, u_cid, u_head, u_reads, u_first, u_word, u_table, u_cell_roots, u_part;
  DevBuf u_rot[2], u_perm[2], u_key[2], u_pos[2];  // the second order: in / out of its two sorts
};

// char2uint_64 of at most `size` characters is below 10^size: the sorts of fqg_census_finish need not look at more bits
// (a UMI of 10 bases: 34 of 64, a cell barcode of 16: 54).  A size that is not known (< 0), or beyond 19 digits: all 64.
static unsigned census_bits(long size) {
  if (size <= 0) return size == 0 ? 1u : 64u;
  if (size > 19) return 64u;
  unsigned long long lim = 1;
  for (long i = 0; i < size; ++i) lim *= 10ull;
  unsigned bits = 1;
  while (bits < 64 && (1ull << bits) < lim) ++bits;
  return bits;
}

int fqg_census_create(fqg_ctx* c, fqg_census** out) {
  if (!c || !out) return FQG_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  std::unique_ptr<fqg_census> z(new fqg_census());
  z->ctx = c;
  // the count of a call, and behind it the whitelist's four: pairs by status (kWlMiss .. kWlAmbiguous) since the census was created
  if (hipMalloc((void**)&z->d_count, 5 * 8) != hipSuccess) return fail(c, FQG_ERR_NOMEM, "fqg_census_create");
  HIP_TRY(c, hipMemsetAsync(z->d_count, 0, 5 * 8, c->stream));
  *out = z.release();
  return 0;
}

void fqg_census_destroy(fqg_census* z) {
  if (!z) return;
  (void)hipStreamSynchronize(z->ctx->stream);
  for (DevBuf* b : {&z->cells, &z->umis, &z->cells2, &z->umis2, &z->tmp, &z->flag, &z->local, &z->sums, &z->lines}) release(*b);
  for (DevBuf* b : {&z->u_flag, &z->u_local, &z->u_sums, &z->u_tot, &z->u_umi, &z->u_cid, &z->u_head, &z->u_reads, &z->u_first,
                    &z->u_word, &z->u_table, &z->u_cell_roots, &z->u_part, &z->u_rot[0], &z->u_rot[1], &z->u_perm[0], &z->u_perm[1],
                    &z->u_key[0], &z->u_key[1], &z->u_pos[0], &z->u_pos[1]})
    release(*b);
  if (z->d_count) (void)hipFree(z->d_count);
  delete z;
}

// room for `need` pairs in a pair of arrays that keep their contents
static int census_reserve(fqg_ctx* c, fqg_census* z, uint64_t need) {
  if (need * 8 <= z->cells.cap) return 0;
  const uint64_t cap = std::max<uint64_t>(need + need / 2, 1u << 16);
  DevBuf a, b;
  if (hipMalloc(&a.p, cap * 8) != hipSuccess) return fail(c, FQG_ERR_NOMEM, "fqg_barcodes_census");
  if (hipMalloc(&b.p, cap * 8) != hipSuccess) {
    (void)hipFree(a.p);
    return fail(c, FQG_ERR_NOMEM, "fqg_barcodes_census");
  }
  a.cap = b.cap = cap * 8;
  if (z->n_pairs) {
    (void)hipMemcpyAsync(a.p, z->cells.p, z->n_pairs * 8, hipMemcpyDeviceToDevice, c->stream);
    (void)hipMemcpyAsync(b.p, z->umis.p, z->n_pairs * 8, hipMemcpyDeviceToDevice, c->stream);
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  release(z->cells);
  release(z->umis);
  z->cells = a;
  z->umis = b;
  return 0;
}

int fqg_barcodes_census(fqg_ctx* c, fqg_census* z, const fqg_frame* const frames[6], const fqg_file_state states[6],
                        const uint64_t first_record[6], const fqg_barcode_params* bp, uint64_t n_done, uint64_t* n_added) {
  if (!c || !z || z->ctx != c || !frames || !states || !first_record || !bp) return FQG_ERR_ARG;
  if (z->finished) return fail(c, FQG_ERR_STATE, "fqg_barcodes_census: the census is finished");
  if (n_done > c->bc_status_valid)
    return fail(c, FQG_ERR_STATE, "fqg_barcodes_census: call it behind the fqg_barcodes_transform of the same batch, with that call's n_done");
  if (n_added) *n_added = 0;
  if (!n_done) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  BcParams P;
  bool inter;
  int rc;
  if ((rc = bc_make_params(c, frames, states, first_record, bp, n_done, 0, P, inter))) return rc;
  if (z->wl && z->max_mismatch && P.cell_read > 0 && (P.cell_size < 1 || P.cell_size > kWlMaxRescueSize))
    return fail(c, FQG_ERR_ARG, "fqg_barcodes_census: a whitelist with max_mismatch 1 takes a cell_size of 1..19");
  if ((rc = census_reserve(c, z, z->n_pairs + n_done))) return rc;
  z->umi_bits = std::max(z->umi_bits, census_bits((long)P.umi_size));
  z->cell_bits = std::max(z->cell_bits, P.cell_read > 0 ? census_bits((long)P.cell_size) : 1u);
  if (P.umi_read > 0 && (P.umi_size < 1 || P.umi_size > kWlMaxRescueSize)) z->umi_wide = true;
  HIP_TRY(c, hipMemsetAsync(z->d_count, 0, 8, c->stream));
  {
    ProfScope ps(c, "k_bc_census");
    const uint64_t tile = (uint64_t)kBlock * kCensusPer;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_done + tile - 1) / tile, (uint64_t)c->cu_count * 16));
    CensusWl W{nullptr, 0, z->d_count + 1, 0};
    if (z->wl) W = CensusWl{(const WlSlot*)z->wl->set.p, z->wl->capacity - 1, z->d_count + 1, (uint32_t)z->max_mismatch};
#define FQG_CENSUS(WL)                                                                                                          \
  hipLaunchKernelGGL(k_bc_census<WL>, dim3(grid), dim3(kBlock), 0, c->stream, P, n_done, (const uint8_t*)c->bc_status.p,        \
                     (unsigned long long*)z->cells.p, (unsigned long long*)z->umis.p, (unsigned long long)z->n_pairs,          \
                     (unsigned long long)(z->cells.cap / 8), z->d_count, W)
    if (z->wl) FQG_CENSUS(true);
    else FQG_CENSUS(false);
#undef FQG_CENSUS
  }
  unsigned long long added = 0;
  HIP_TRY(c, hipMemcpyAsync(&added, z->d_count, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  z->n_pairs += added;
  if (n_added) *n_added = added;
  return 0;
}

int fqg_census_finish(fqg_ctx* c, fqg_census* z, uint64_t* n_pairs, uint64_t* n_cells) {
  if (!c || !z || z->ctx != c) return FQG_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t n = z->n_pairs;
  if (!z->finished && n) {
    int rc;
    if ((rc = ensure(c, z->cells2, n * 8)) || (rc = ensure(c, z->umis2, n * 8))) return rc;
    if (n >= (1ull << 31)) return fail(c, FQG_ERR_ARG, "fqg_census_finish: more than 2^31 pairs");
    // by UMI, then (stable) by cell: sorted by (cell, UMI)
    unsigned long long *ce = (unsigned long long*)z->cells.p, *um = (unsigned long long*)z->umis.p;
    unsigned long long *ce2 = (unsigned long long*)z->cells2.p, *um2 = (unsigned long long*)z->umis2.p;
    size_t tmp_bytes = 0;
    const unsigned ub = z->umi_bits, cb = z->cell_bits;
    if (rocprim::radix_sort_pairs(nullptr, tmp_bytes, um, um2, ce, ce2, n, 0, 64, c->stream) != hipSuccess)
      return fail(c, FQG_ERR_HIP, "fqg_census_finish: sort");
    if ((rc = ensure(c, z->tmp, tmp_bytes + 16))) return rc;
    ProfScope ps(c, "k_census_finish");
    if (rocprim::radix_sort_pairs(z->tmp.p, tmp_bytes, um, um2, ce, ce2, n, 0, ub, c->stream) != hipSuccess ||
        rocprim::radix_sort_pairs(z->tmp.p, tmp_bytes, ce2, ce, um2, um, n, 0, cb, c->stream) != hipSuccess)
      return fail(c, FQG_ERR_HIP, "fqg_census_finish: sort");
    const uint64_t nb = scan64_spans(n);
    if ((rc = ensure(c, z->flag, n * 4)) || (rc = ensure(c, z->local, n * 8)) || (rc = ensure(c, z->sums, nb * 8 + 8))) return rc;
    unsigned long long* d_total = (unsigned long long*)z->sums.p + nb;
    HIP_TRY(c, hipMemsetAsync(d_total, 0, 8, c->stream));
    const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_census_flags, dim3(grid), dim3(kBlock), 0, c->stream, (const unsigned long long*)ce, n, (uint32_t*)z->flag.p);
    scan64(c, z->flag.p, z->local.p, z->sums.p, d_total, n);
    unsigned long long cells = 0;
    HIP_TRY(c, hipMemcpyAsync(&cells, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    z->n_cells = cells;
    if ((rc = ensure(c, z->lines, cells * sizeof(CensusCell)))) return rc;
    HIP_TRY(c, hipMemsetAsync(z->lines.p, 0, cells * sizeof(CensusCell), c->stream));
    hipLaunchKernelGGL(k_census_count, dim3(grid), dim3(kBlock), 0, c->stream, (const unsigned long long*)ce,
                       (const unsigned long long*)um, n, (const uint32_t*)z->flag.p, (const unsigned long long*)z->local.p,
                       (const unsigned long long*)z->sums.p, (CensusCell*)z->lines.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
  }
  z->finished = true;
  if (n_pairs) *n_pairs = z->n_pairs;
  if (n_cells) *n_cells = z->n_cells;
  return 0;
}

int fqg_census_cells(fqg_ctx* c, fqg_census* z, fqg_census_cell* out, uint64_t cap) {
  if (!c || !z || z->ctx != c || (!out && cap)) return FQG_ERR_ARG;
  if (!z->finished) return fail(c, FQG_ERR_STATE, "fqg_census_cells: fqg_census_finish first");
  static_assert(sizeof(fqg_census_cell) == sizeof(CensusCell), "the C-ABI line is the device line");
  const uint64_t n = std::min<uint64_t>(cap, z->n_cells);
  if (n) HIP_TRY(c, hipMemcpy(out, z->lines.p, n * sizeof(CensusCell), hipMemcpyDeviceToHost));
  return 0;
}

int fqg_census_pairs(fqg_ctx* c, fqg_census* z, uint64_t* cells, uint64_t* umis, uint64_t cap) {
  if (!c || !z || z->ctx != c || ((!cells || !umis) && cap)) return FQG_ERR_ARG;
  const uint64_t n = std::min<uint64_t>(cap, z->n_pairs);
  if (n) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(cells, z->cells.p, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(umis, z->umis.p, n * 8, hipMemcpyDeviceToHost));
  }
  return 0;
}

const void* fqg_census_device_pairs(const fqg_census* z, int which) {
  return z ? (which ? z->umis.p : z->cells.p) : nullptr;
}

// pairs from host memory, taken as given (no whitelist look-up)
int fqg_census_append(fqg_ctx* c, fqg_census* z, const uint64_t* cells, const uint64_t* umis, uint64_t n, int cell_size,
                      int umi_size) {
  if (!c || !z || z->ctx != c || ((!cells || !umis) && n)) return FQG_ERR_ARG;
  if (z->finished) return fail(c, FQG_ERR_STATE, "fqg_census_append: the census is finished");
  if (!n) return 0;
  const int sizes[2] = {cell_size, umi_size};
  const uint64_t* vals[2] = {cells, umis};
  for (int k = 0; k < 2; ++k) {
    if (sizes[k] < 1 || sizes[k] > kWlMaxRescueSize) continue;  // (unknown, or twenty digits and more: any value)
    unsigned long long lim = 1;
    for (int i = 0; i < sizes[k]; ++i) lim *= 10ull;
    for (uint64_t i = 0; i < n; ++i)
      if (vals[k][i] >= lim) return fail(c, FQG_ERR_ARG, "fqg_census_append: a value of more digits than its size");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  if ((rc = census_reserve(c, z, z->n_pairs + n))) return rc;
  HIP_TRY(c, hipMemcpyAsync((unsigned long long*)z->cells.p + z->n_pairs, cells, n * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync((unsigned long long*)z->umis.p + z->n_pairs, umis, n * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  z->umi_bits = std::max(z->umi_bits, census_bits(umi_size > 0 ? (long)umi_size : -1l));
  z->cell_bits = std::max(z->cell_bits, census_bits(cell_size > 0 ? (long)cell_size : -1l));
  if (umi_size < 1 || umi_size > kWlMaxRescueSize) z->umi_wide = true;
  z->n_pairs += n;
  return 0;
}

// ---- the census with UMI collapse (fqg_census_umi_kernels.hip) ---------------------------------------
// bits a radix sort has to look at for keys below `count`
static unsigned bits_below(uint64_t count) {
  unsigned bits = 1;
  while (bits < 64 && (1ull << bits) < count) ++bits;
  return bits;
}

int fqg_census_collapse_umis(fqg_ctx* c, fqg_census* z, int max_mismatch, fqg_census_collapse_result* out) {
  if (!c || !z || z->ctx != c || !out) return FQG_ERR_ARG;
  *out = fqg_census_collapse_result{};
  if (!z->finished) return fail(c, FQG_ERR_STATE, "fqg_census_collapse_umis: fqg_census_finish first");
  if (max_mismatch != 0 && max_mismatch != 1) return fail(c, FQG_ERR_ARG, "fqg_census_collapse_umis: max_mismatch is 0 or 1");
  if (max_mismatch && z->umi_wide) return fail(c, FQG_ERR_ARG, "fqg_census_collapse_umis: max_mismatch 1 takes a umi_size of 1..19");
  HIP_TRY(c, hipSetDevice(c->device));
  z->collapsed = false;
  z->n_umis = 0;
  const uint64_t n = z->n_pairs, n_cells = z->n_cells;
  if (!n) {
    z->collapsed = true;
    return 0;
  }
  typedef unsigned long long u64;
  int rc;
  const uint64_t nb = scan64_spans(n);
  if ((rc = ensure(c, z->u_flag, n * 4)) || (rc = ensure(c, z->u_local, n * 8)) || (rc = ensure(c, z->u_sums, nb * 8 + 8)) ||
      (rc = ensure(c, z->u_tot, 3 * 8)))
    return rc;
  u64* d_tot = (u64*)z->u_tot.p;  // distinct pairs; rows with a parent, the longest chain (k_cu_roots)
  HIP_TRY(c, hipMemsetAsync(d_tot, 0, 3 * 8, c->stream));
  const unsigned grid_n = (unsigned)((n + kBlock - 1) / kBlock);
  {
    ProfScope ps(c, "k_cu_flags");
    hipLaunchKernelGGL(k_cu_flags, dim3(grid_n), dim3(kBlock), 0, c->stream, (const u64*)z->cells.p, (const u64*)z->umis.p, n,
                       (uint32_t*)z->u_flag.p);
    scan64(c, z->u_flag.p, z->u_local.p, z->u_sums.p, d_tot, n);
  }
  u64 m64 = 0;
  HIP_TRY(c, hipMemcpyAsync(&m64, d_tot, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  const uint64_t m = m64;
  if (!m || m > n || !n_cells) return fail(c, FQG_ERR_HIP, "fqg_census_collapse_umis: the count of distinct pairs");
  if ((rc = ensure(c, z->u_umi, m * 8)) || (rc = ensure(c, z->u_cid, m * 4)) || (rc = ensure(c, z->u_head, (m + 1) * 4)) ||
      (rc = ensure(c, z->u_reads, m * 4)) || (rc = ensure(c, z->u_first, (n_cells + 1) * 4)) || (rc = ensure(c, z->u_word, m * 8)) ||
      (rc = ensure(c, z->u_table, m * sizeof(CensusUmi))) || (rc = ensure(c, z->u_cell_roots, n_cells * 8)) ||
      (rc = ensure(c, z->u_part, ((m + kBlock - 1) / kBlock) * 16)))
    return rc;
  const unsigned ub = std::min(64u, z->umi_bits), cb = bits_below(n_cells);
  size_t tmp_bytes = 0;
  if (max_mismatch) {
    for (int k = 0; k < 2; ++k)
      if ((rc = ensure(c, z->u_rot[k], m * 8)) || (rc = ensure(c, z->u_perm[k], m * 4)) || (rc = ensure(c, z->u_key[k], m * 4)) ||
          (rc = ensure(c, z->u_pos[k], m * 4)))
        return rc;
    size_t t1 = 0, t2 = 0;
    if (rocprim::radix_sort_pairs(nullptr, t1, (u64*)z->u_rot[0].p, (u64*)z->u_rot[1].p, (uint32_t*)z->u_perm[0].p,
                                  (uint32_t*)z->u_perm[1].p, m, 0, ub, c->stream) != hipSuccess ||
        rocprim::radix_sort_pairs(nullptr, t2, (uint32_t*)z->u_key[0].p, (uint32_t*)z->u_key[1].p, (uint32_t*)z->u_pos[0].p,
                                  (uint32_t*)z->u_pos[1].p, m, 0, cb, c->stream) != hipSuccess)
      return fail(c, FQG_ERR_HIP, "fqg_census_collapse_umis: sort");
    tmp_bytes = std::max(t1, t2);
    if ((rc = ensure(c, z->tmp, tmp_bytes + 16))) return rc;
  }
  const unsigned grid_m = (unsigned)((m + kBlock - 1) / kBlock);
  const u64* r_umi = (const u64*)z->u_umi.p;
  const uint32_t *r_cid = (const uint32_t*)z->u_cid.p, *r_reads = (const uint32_t*)z->u_reads.p, *first = (const uint32_t*)z->u_first.p;
  {
    ProfScope ps(c, "k_cu_rows");
    hipLaunchKernelGGL(k_cu_rows, dim3(grid_n), dim3(kBlock), 0, c->stream, (const u64*)z->umis.p, n, (const uint32_t*)z->u_flag.p,
                       (const u64*)z->u_local.p, (const u64*)z->u_sums.p, (const uint32_t*)z->flag.p, (const u64*)z->local.p,
                       (const u64*)z->sums.p, m, n_cells, (u64*)z->u_umi.p, (uint32_t*)z->u_cid.p, (uint32_t*)z->u_head.p,
                       (uint32_t*)z->u_first.p);
    hipLaunchKernelGGL(k_cu_prep, dim3(grid_m), dim3(kBlock), 0, c->stream, r_umi, (const uint32_t*)z->u_head.p, m,
                       (uint32_t*)z->u_reads.p, max_mismatch ? (u64*)z->u_rot[0].p : nullptr, (uint32_t*)z->u_perm[0].p);
  }
  if (max_mismatch) {
    {
      ProfScope ps(c, "k_cu_run_a");
      hipLaunchKernelGGL(k_cu_run<false>, dim3(grid_m), dim3(kBlock), 0, c->stream, r_umi, (const uint32_t*)nullptr, r_cid, first,
                         r_reads, m, (u64*)z->u_word.p);
    }
    {
      // the second order: by the rotated value, then (stable) by cell id; keys and rows gathered into that order
      ProfScope ps(c, "k_cu_order");
      if (rocprim::radix_sort_pairs(z->tmp.p, tmp_bytes, (u64*)z->u_rot[0].p, (u64*)z->u_rot[1].p, (uint32_t*)z->u_perm[0].p,
                                    (uint32_t*)z->u_perm[1].p, m, 0, ub, c->stream) != hipSuccess)
        return fail(c, FQG_ERR_HIP, "fqg_census_collapse_umis: sort");
      hipLaunchKernelGGL(k_cu_gather_cid, dim3(grid_m), dim3(kBlock), 0, c->stream, (const uint32_t*)z->u_perm[1].p, r_cid, m,
                         (uint32_t*)z->u_key[0].p, (uint32_t*)z->u_pos[0].p);
      if (rocprim::radix_sort_pairs(z->tmp.p, tmp_bytes, (uint32_t*)z->u_key[0].p, (uint32_t*)z->u_key[1].p, (uint32_t*)z->u_pos[0].p,
                                    (uint32_t*)z->u_pos[1].p, m, 0, cb, c->stream) != hipSuccess)
        return fail(c, FQG_ERR_HIP, "fqg_census_collapse_umis: sort");
      hipLaunchKernelGGL(k_cu_gather_rot, dim3(grid_m), dim3(kBlock), 0, c->stream, (const uint32_t*)z->u_pos[1].p,
                         (const u64*)z->u_rot[1].p, (const uint32_t*)z->u_perm[1].p, m, (u64*)z->u_rot[0].p, (uint32_t*)z->u_perm[0].p);
    }
    {
      ProfScope ps(c, "k_cu_run_b");
      hipLaunchKernelGGL(k_cu_run<true>, dim3(grid_m), dim3(kBlock), 0, c->stream, (const u64*)z->u_rot[0].p,
                         (const uint32_t*)z->u_perm[0].p, r_cid, first, r_reads, m, (u64*)z->u_word.p);
    }
  } else {
    HIP_TRY(c, hipMemsetAsync(z->u_word.p, 0, m * 8, c->stream));
  }
  HIP_TRY(c, hipMemsetAsync(z->u_cell_roots.p, 0, n_cells * 8, c->stream));
  {
    ProfScope ps(c, "k_cu_roots");
    hipLaunchKernelGGL(k_cu_roots, dim3(grid_m), dim3(kBlock), 0, c->stream, (const u64*)z->u_word.p, r_umi, r_cid, r_reads,
                       (const CensusCell*)z->lines.p, m, (CensusUmi*)z->u_table.p, (u64*)z->u_cell_roots.p, (u64*)z->u_part.p);
    hipLaunchKernelGGL(k_cu_totals, dim3(1), dim3(kBlock), 0, c->stream, (const u64*)z->u_part.p, (uint64_t)grid_m, d_tot + 1);
  }
  u64 tot[3] = {0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  z->n_umis = m;
  z->collapsed = true;
  out->n_umis = m;
  out->n_absorbed = tot[1];
  out->n_roots = m - tot[1];
  out->longest_chain = tot[2];
  return 0;
}

int fqg_census_umis(fqg_ctx* c, fqg_census* z, fqg_census_umi* out, uint64_t cap) {
  if (!c || !z || z->ctx != c || (!out && cap)) return FQG_ERR_ARG;
  if (!z->collapsed) return fail(c, FQG_ERR_STATE, "fqg_census_umis: fqg_census_collapse_umis first");
  static_assert(sizeof(fqg_census_umi) == sizeof(CensusUmi), "the C-ABI row is the device row");
  const uint64_t n = std::min<uint64_t>(cap, z->n_umis);
  if (n) HIP_TRY(c, hipMemcpy(out, z->u_table.p, n * sizeof(CensusUmi), hipMemcpyDeviceToHost));
  return 0;
}

int fqg_census_cells_collapsed(fqg_ctx* c, fqg_census* z, uint64_t* umis, uint64_t cap) {
  if (!c || !z || z->ctx != c || (!umis && cap)) return FQG_ERR_ARG;
  if (!z->collapsed) return fail(c, FQG_ERR_STATE, "fqg_census_cells_collapsed: fqg_census_collapse_umis first");
  const uint64_t n = std::min<uint64_t>(cap, z->n_cells);
  if (n) HIP_TRY(c, hipMemcpy(umis, z->u_cell_roots.p, n * 8, hipMemcpyDeviceToHost));
  return 0;
}

int fqg_census_set_whitelist(fqg_ctx* c, fqg_census* z, const fqg_whitelist* wl, int max_mismatch) {
  if (!c || !z || z->ctx != c) return FQG_ERR_ARG;
  if (wl && wl->ctx != c) return fail(c, FQG_ERR_ARG, "fqg_census_set_whitelist: a whitelist of another context");
  if (max_mismatch != 0 && max_mismatch != 1) return fail(c, FQG_ERR_ARG, "fqg_census_set_whitelist: max_mismatch is 0 or 1");
  if (z->n_pairs || z->finished)
    return fail(c, FQG_ERR_ARG, "fqg_census_set_whitelist: the census holds pairs already");
  z->wl = wl;
  z->max_mismatch = wl ? max_mismatch : 0;
  return 0;
}

int fqg_census_whitelist_info(const fqg_census* z, uint64_t info[4]) {
  if (!z || !info) return FQG_ERR_ARG;
  unsigned long long v[4] = {0, 0, 0, 0};
  if (hipSetDevice(z->ctx->device) != hipSuccess || hipStreamSynchronize(z->ctx->stream) != hipSuccess ||
      hipMemcpy(v, z->d_count + 1, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
    return FQG_ERR_HIP;
  info[0] = v[kWlExact], info[1] = v[kWlRescued], info[2] = v[kWlAmbiguous];
  info[3] = v[kWlAmbiguous] + v[kWlMiss];  // dropped: what the look-up took away, the ambiguous ones among them
  return 0;
}

// ---- whitelist membership (struct fqg_whitelist: above, in front of the census that may hold one) ----
int fqg_whitelist_create(fqg_ctx* c, const uint64_t* packed, uint64_t n, fqg_whitelist** out) {
  if (!c || !out || (!packed && n)) return FQG_ERR_ARG;
  *out = nullptr;
  HIP_TRY(c, hipSetDevice(c->device));
  uint64_t cap = 1024;
  while (cap < 4 * n) cap <<= 1;
  std::vector<WlSlot> host(cap, WlSlot{0, 0});
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t at = wl_hash(packed[i]) & (cap - 1);
    while (host[at].used && host[at].key != packed[i]) at = (at + 1) & (cap - 1);
    host[at] = WlSlot{packed[i], 1};
  }
  std::unique_ptr<fqg_whitelist> w(new fqg_whitelist());
  w->ctx = c;
  w->capacity = cap;
  int rc;
  if ((rc = ensure(c, w->set, cap * sizeof(WlSlot)))) return rc;
  HIP_TRY(c, hipMemcpy(w->set.p, host.data(), cap * sizeof(WlSlot), hipMemcpyHostToDevice));
  *out = w.release();
  return 0;
}

void fqg_whitelist_destroy(fqg_whitelist* w) {
  if (!w) return;
  (void)hipStreamSynchronize(w->ctx->stream);
  release(w->set);
  delete w;
}

// fqg_barcodes_whitelist and fqg_barcodes_whitelist_correct are wl_call_begin, their kernel, wl_call_end, their counters.
extern "C++" {
namespace {

// The checks (`who`: the caller, for the messages), `out` cleared; for records to look at, room for the per-record arrays
// the caller wants - bytes in c->bc_status, cells in c->wl_cells - and the call's counters, `call_bytes` at the head of the
// context's BcCall, zeroed.
int wl_call_begin(fqg_ctx* c, const char* who, const fqg_frame* frame, uint64_t first, uint64_t step, uint64_t n, int64_t offset,
                  int64_t size, const fqg_whitelist* wl, int max_mismatch, void* out, size_t out_bytes, bool want_bytes,
                  bool want_cells, size_t call_bytes) {
  if (!c || !frame || !wl || !out || wl->ctx != c || frame->ctx != c) return FQG_ERR_ARG;
  memset(out, 0, out_bytes);
  const auto refuse = [&](const char* what) {
    fail(c, FQG_ERR_ARG, who);
    c->err += what;
    return FQG_ERR_ARG;
  };
  if (offset < 0 || size < 1 || size > kWlMaxSize) return refuse(": offset >= 0 and 1 <= size <= 56");
  if (max_mismatch != 0 && max_mismatch != 1) return refuse(": max_mismatch is 0 or 1");
  if (max_mismatch && size > kWlMaxRescueSize) return refuse(": max_mismatch 1 takes a size of 1..19");
  if (frame->flags & kFlagNul) return refuse(": input holds NUL bytes");
  if (step < 1 || (n && first + (n - 1) * step >= frame->fv.n_records)) return refuse(": records beyond the frame");
  if (!n) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  if (want_bytes) {
    NEED(ensure(c, c->bc_status, n));
    c->bc_status_valid = 0;  // (the status bytes of the last transform are gone: fqg_barcodes_census refuses them)
  }
  if (want_cells) NEED(ensure(c, c->wl_cells, n * 8));
  static_assert(sizeof(WlCall) <= sizeof(BcCall) && sizeof(WlCorrectCall) <= sizeof(BcCall),
                "the call's counters live in the context's BcCall");
  HIP_TRY(c, hipMemsetAsync(c->d_bcall, 0, call_bytes, c->stream));
  return 0;
}

// the kernel for the barcode's size: f(std::integral_constant<int, WORDS>), WORDS 8-byte words hold it
template <class F>
void wl_with_words(int64_t size, F f) {
  if (size <= 16) f(std::integral_constant<int, 2>{});
  else if (size <= 32) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 7>{});
}

// the counters read back into the pinned BcCall, the per-record arrays into the caller's memory
int wl_call_end(fqg_ctx* c, uint64_t n, size_t call_bytes, uint8_t* bytes, uint64_t* cells) {
  HIP_TRY(c, hipMemcpyAsync(c->h_bcall, c->d_bcall, call_bytes, hipMemcpyDeviceToHost, c->stream));
  if (bytes) HIP_TRY(c, hipMemcpyAsync(bytes, c->bc_status.p, n, hipMemcpyDeviceToHost, c->stream));
  if (cells) HIP_TRY(c, hipMemcpyAsync(cells, c->wl_cells.p, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipGetLastError());
  return 0;
}

}  // namespace
}  // extern "C++"

int fqg_barcodes_whitelist(fqg_ctx* c, const fqg_frame* frame, uint64_t first, uint64_t step, uint64_t n, int64_t offset,
                           int64_t size, const fqg_whitelist* wl, uint8_t* valid, fqg_whitelist_result* out) {
  NEED(wl_call_begin(c, "fqg_barcodes_whitelist", frame, first, step, n, offset, size, wl, 0, out, sizeof(*out), valid != nullptr,
                     false, sizeof(WlCall)));
  out->n_records = n;
  if (!n) return 0;
  {
    ProfScope ps(c, "k_bc_whitelist");
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)c->cu_count * 32));
    wl_with_words(size, [&](auto words) {
      hipLaunchKernelGGL(k_bc_whitelist<decltype(words)::value>, dim3(grid), dim3(kBlock), 0, c->stream, frame->fv, first, step, n,
                         (uint32_t)offset, (uint32_t)size, (const WlSlot*)wl->set.p, wl->capacity - 1, valid ? (uint8_t*)c->bc_status.p : nullptr,
                         reinterpret_cast<WlCall*>(c->d_bcall));
    });
  }
  NEED(wl_call_end(c, n, sizeof(WlCall), valid, nullptr));
  const WlCall* h_call = reinterpret_cast<const WlCall*>(c->h_bcall);
  out->n_valid = h_call->n_valid;
  out->n_short = h_call->n_short;
  return 0;
}

int fqg_barcodes_whitelist_correct(fqg_ctx* c, const fqg_frame* frame, uint64_t first, uint64_t step, uint64_t n, int64_t offset,
                                   int64_t size, const fqg_whitelist* wl, int max_mismatch, uint8_t* status, uint64_t* cells,
                                   fqg_whitelist_correct_result* out) {
  static_assert(kWlMiss == FQG_WL_MISS && kWlExact == FQG_WL_EXACT && kWlRescued == FQG_WL_RESCUED &&
                    kWlAmbiguous == FQG_WL_AMBIGUOUS && kWlShort == FQG_WL_SHORT,
                "the kernels' status bytes are the header's");
  NEED(wl_call_begin(c, "fqg_barcodes_whitelist_correct", frame, first, step, n, offset, size, wl, max_mismatch, out, sizeof(*out),
                     status != nullptr, cells != nullptr, sizeof(WlCorrectCall)));
  out->n_records = n;
  if (!n) return 0;
  {
    ProfScope ps(c, "k_bc_whitelist_correct");
    // (8 workgroups of 4 wavefronts fill a CU; more of them only add to the counters more often)
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)c->cu_count * 8));
    wl_with_words(size, [&](auto words) {
      hipLaunchKernelGGL(k_bc_whitelist_correct<decltype(words)::value>, dim3(grid), dim3(kBlock), 0, c->stream, frame->fv, first,
                         step, n, (uint32_t)offset, (uint32_t)size, (const WlSlot*)wl->set.p, wl->capacity - 1,
                         (uint32_t)max_mismatch, status ? (uint8_t*)c->bc_status.p : nullptr,
                         cells ? (unsigned long long*)c->wl_cells.p : nullptr, reinterpret_cast<WlCorrectCall*>(c->d_bcall));
    });
  }
  NEED(wl_call_end(c, n, sizeof(WlCorrectCall), status, cells));
  const WlCorrectCall* h_call = reinterpret_cast<const WlCorrectCall*>(c->h_bcall);
  out->n_exact = h_call->by_status[kWlExact];
  out->n_rescued = h_call->by_status[kWlRescued];
  out->n_ambiguous = h_call->by_status[kWlAmbiguous];
  out->n_short = h_call->by_status[kWlShort];
  return 0;
}
