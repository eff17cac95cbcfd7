// fqg_umi_abi.inc - host side of fqg_umi_count (included by fqg_abi.hip inside extern "C")

uint64_t fqg_pack_barcode(const char* s) {  // char2uint_64, src/bam_umi_count.c:364-382
  if (!s || !*s) return 0;
  int pos = 0;
  while (s[pos] != '\0' && s[pos] != '\n') ++pos;
  uint64_t v = 0;
  while (pos > 0) {
    int b;
    switch (s[pos - 1]) {
      case 'A': case 'a': b = 1; break;
      case 'C': case 'c': b = 2; break;
      case 'G': case 'g': b = 3; break;
      case 'T': case 't': b = 4; break;
      case 'N': case 'n': b = 5; break;
      default: b = 0;
    }
    if (!b) break;
    v = v * 10 + (uint64_t)b;
    --pos;
  }
  return v;
}

void fqg_unpack_barcode(uint64_t v, char* out) {  // uint_642char, :342-360
  static const char nt[] = {' ', 'A', 'C', 'G', 'T', 'N', '.', '?', '?', '?'};
  int x = 0;
  while (v > 0 && x < 19) {
    out[x++] = nt[v % 10];
    v /= 10;
  }
  out[x] = '\0';
}

int fqg_bam_index_records(const void* stream, uint64_t nbytes, uint64_t* offsets, uint64_t cap, uint64_t* n,
                          uint64_t* used) {
  if (!stream || !n) return FQG_ERR_ARG;
  const uint8_t* b = (const uint8_t*)stream;
  auto rd32 = [&](uint64_t o) { return (int32_t)((uint32_t)b[o] | ((uint32_t)b[o + 1] << 8) | ((uint32_t)b[o + 2] << 16) | ((uint32_t)b[o + 3] << 24)); };
  if (nbytes < 12 || memcmp(b, "BAM\1", 4) != 0) return FQG_ERR_ARG;
  uint64_t p = 8 + (uint64_t)(uint32_t)rd32(4);
  if (p + 4 > nbytes) return FQG_ERR_ARG;
  const int32_t n_ref = rd32(p);
  p += 4;
  if (n_ref < 0) return FQG_ERR_ARG;
  for (int32_t i = 0; i < n_ref; ++i) {
    if (p + 4 > nbytes) return FQG_ERR_ARG;
    p += 4 + (uint64_t)(uint32_t)rd32(p) + 4;
  }
  if (p > nbytes) return FQG_ERR_ARG;  // the last reference's name / length lie beyond the stream (a truncated header)
  uint64_t k = 0;
  while (p + 4 <= nbytes) {
    const int32_t block = rd32(p);
    if (block < 32 || p + 4 + (uint64_t)block > nbytes) break;  // truncated tail: bam_read1 fails there
    if (offsets && k < cap) offsets[k] = p;
    ++k;
    p += 4 + (uint64_t)block;
  }
  *n = k;
  if (used) *used = p;
  return (offsets && k > cap) ? FQG_ERR_ARG : 0;
}

extern "C++" {
namespace {
// Device memory of one call.  A call makes about fifty allocations; hipMalloc / hipFree for each of
// them cost more than all kernels of configs[3] together.  They are carved out of one arena that the
// context keeps between calls instead (sized by what the previous call asked for); what does not fit
// - the first call, a larger input - falls back to hipMalloc for this call only.
struct Scratch {
  fqg_ctx* c;
  std::vector<void*> ptrs;
  size_t used = 0, wanted = 0;
  explicit Scratch(fqg_ctx* ctx) : c(ctx) {}
  ~Scratch() {
    for (void* p : ptrs) (void)hipFree(p);
    if (wanted > c->umi_arena_wanted) c->umi_arena_wanted = wanted;
  }
  template <class T>
  T* get(uint64_t count, int fill = -1) {
    void* p = nullptr;
    const size_t bytes = (std::max<uint64_t>(count, 1) * sizeof(T) + 255u) & ~(size_t)255u;
    wanted += bytes;
    if (c->umi_arena.p && used + bytes <= c->umi_arena.cap) {
      p = (char*)c->umi_arena.p + used;
      used += bytes;
    } else {
      if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
      ptrs.push_back(p);
    }
    if (fill >= 0 && hipMemsetAsync(p, fill, bytes, c->stream) != hipSuccess) return nullptr;
    return (T*)p;
  }
};
// Grows the arena to what the call that just ended asked for - at the END of that call (declared before the
// call's Scratch, so destroyed after it), unless a deferred state still lives in the arena.  The next call then
// starts with its memory in place.
struct ArenaGrow {
  fqg_ctx* c;
  ~ArenaGrow() {
    if (c->umi_state || c->umi_arena_wanted <= c->umi_arena.cap) return;
    (void)hipStreamSynchronize(c->stream);
    release(c->umi_arena);
    (void)ensure(c, c->umi_arena, c->umi_arena_wanted + (c->umi_arena_wanted >> 3));  // (on failure: hipMalloc per buffer)
  }
};
struct UmiState {  // what fqg_umi_emit needs from the counting step
  Scratch* scratch = nullptr;
  EmitArgs A;
  UmiCall* d_call = nullptr;
  unsigned long long* d_tot = nullptr;
  uint64_t n_pairs = 0;
  // for runs over several GPUs (fqg_umi_record_features / fqg_umi_replayed_features)
  const uint32_t* rec_feat = nullptr;   // per alignment: its feature id (0: the alignment was not counted)
  const uint8_t* feat_replayed = nullptr;  // per feature id: one of its (cell, feature) sets was replayed (null: none was)
  uint64_t n_records = 0, n_features = 0;
};
void umi_drop_state(fqg_ctx* c) {
  UmiState* us = (UmiState*)c->umi_state;
  if (!us) return;
  delete us->scratch;
  delete us;
  c->umi_state = nullptr;
}
uint64_t pow2_at_least(uint64_t v) {
  uint64_t p = 1024;
  while (p < v) p <<= 1;
  return p;
}
unsigned blocks_for(uint64_t n) { return (unsigned)std::max<uint64_t>(1, (n + kBlock - 1) / kBlock); }
}  // namespace
}  // extern "C++"

#define UMI_NEED(ptr) \
  if (!(ptr)) return fail(c, FQG_ERR_NOMEM, "fqg_umi_count: device allocation failed")

int fqg_umi_count(fqg_ctx* c, const void* stream, uint64_t nbytes, int mem, const uint64_t* offsets,
                  uint64_t n_records, const fqg_umi_params* prm, fqg_umi_result* out) {
  if (!c || !out || !prm || (n_records && (!stream || !offsets))) return FQG_ERR_ARG;
  if (mem != FQG_MEM_HOST && mem != FQG_MEM_DEVICE && mem != FQG_MEM_DEVICE_INDEXED) return FQG_ERR_ARG;
  if (n_records >= 0x7FFFFFFFull) return fail(c, FQG_ERR_ARG, "fqg_umi_count: more than 2^31 alignments in one call");
  memset(out, 0, sizeof(*out));
  c->umi_n_features = c->umi_n_cells = c->umi_n_entries[0] = c->umi_n_entries[1] = 0;
  c->umi_n_umis = 0;
  out->n_alignments = n_records;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!n_records) return 0;
  const uint32_t n = (uint32_t)n_records;
  umi_drop_state(c);
  if (c->umi_arena_wanted > c->umi_arena.cap) {  // nothing of an earlier call is alive here: the arena may move
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    release(c->umi_arena);
    (void)ensure(c, c->umi_arena, c->umi_arena_wanted + (c->umi_arena_wanted >> 3));  // (on failure: hipMalloc per buffer)
  }
  ArenaGrow grow_afterwards{c};
  Scratch* Sp = new Scratch(c);
  std::unique_ptr<Scratch> S_owner(Sp);
  Scratch& S = *Sp;
  hipStream_t st = c->stream;

  // ---- inputs ----
  const uint8_t* d_buf;
  if (mem == FQG_MEM_HOST) {
    uint8_t* p = S.get<uint8_t>(nbytes + 16);
    UMI_NEED(p);
    HIP_TRY(c, hipMemcpyAsync(p, stream, nbytes, hipMemcpyHostToDevice, st));
    d_buf = p;
  } else d_buf = (const uint8_t*)stream;
  const unsigned long long* d_off;
  if (mem == FQG_MEM_DEVICE_INDEXED) d_off = reinterpret_cast<const unsigned long long*>(offsets);  // (the caller's, in HBM)
  else {
    unsigned long long* p = S.get<unsigned long long>(n);
    UMI_NEED(p);
    HIP_TRY(c, hipMemcpyAsync(p, offsets, (size_t)n * 8, hipMemcpyHostToDevice, st));
    d_off = p;
  }

  UmiParams P;
  memset(&P, 0, sizeof(P));
  memcpy(P.feat_tag, prm->feat_tag, 2);
  memcpy(P.cell_tag, prm->cell_tag, 2);
  memcpy(P.umi_tag, prm->umi_tag, 2);
  P.sorted_by_cell = prm->sorted_by_cell;
  P.uniq_mapped_only = prm->uniq_mapped_only;
  P.max_cells = prm->max_cells;
  P.max_features = prm->max_features;
  P.min_reads = prm->min_reads;
  P.min_umis = prm->min_umis;
  // whitelists: the UMI list numbers its distinct entries 1..K in file order (load_whitelist :543-579 with
  // map = umis_map); the cell list is a plain set
  std::vector<unsigned long long> ku_sorted, kc_sorted;
  std::vector<uint32_t> ku_order;
  if (prm->known_umis) {
    P.have_known_umis = 1;
    std::vector<std::pair<unsigned long long, uint32_t>> v;
    std::vector<unsigned long long> seen;
    for (uint64_t i = 0; i < prm->n_known_umis; ++i) {
      const unsigned long long x = prm->known_umis[i];
      bool dup = false;
      for (auto& e : v) dup |= e.first == x;  // (whitelists are small; keep file order exact)
      if (!dup) v.push_back({x, (uint32_t)v.size()});
    }
    std::sort(v.begin(), v.end());
    for (auto& e : v) {
      ku_sorted.push_back(e.first);
      ku_order.push_back(e.second);
    }
    P.n_known_umis = (uint32_t)v.size();
    unsigned long long* a = S.get<unsigned long long>(v.size());
    uint32_t* b = S.get<uint32_t>(v.size());
    UMI_NEED(a && b);
    if (!v.empty()) {
      HIP_TRY(c, hipMemcpyAsync(a, ku_sorted.data(), v.size() * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(b, ku_order.data(), v.size() * 4, hipMemcpyHostToDevice, st));
    }
    P.known_umis_sorted = a;
    P.known_umis_order = b;
  }
  if (prm->known_cells) {
    P.have_known_cells = 1;
    kc_sorted.assign(prm->known_cells, prm->known_cells + prm->n_known_cells);
    std::sort(kc_sorted.begin(), kc_sorted.end());
    kc_sorted.erase(std::unique(kc_sorted.begin(), kc_sorted.end()), kc_sorted.end());
    P.n_known_cells = (uint32_t)kc_sorted.size();
    unsigned long long* a = S.get<unsigned long long>(kc_sorted.size());
    UMI_NEED(a);
    if (!kc_sorted.empty())
      HIP_TRY(c, hipMemcpyAsync(a, kc_sorted.data(), kc_sorted.size() * 8, hipMemcpyHostToDevice, st));
    P.known_cells_sorted = a;
  }

  if (prm->umi_table_keys) {
    if (!prm->umi_table_ids || prm->n_umi_table >= 0xFFFFFFFFull) return fail(c, FQG_ERR_ARG, "fqg_umi_count: umi_table_ids / n_umi_table");
    unsigned long long* a = S.get<unsigned long long>(prm->n_umi_table);
    uint32_t* b = S.get<uint32_t>(prm->n_umi_table);
    UMI_NEED(a && b);
    if (prm->n_umi_table) {
      HIP_TRY(c, hipMemcpyAsync(a, prm->umi_table_keys, (size_t)prm->n_umi_table * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(b, prm->umi_table_ids, (size_t)prm->n_umi_table * 4, hipMemcpyHostToDevice, st));
    }
    P.umi_table_keys = a;
    P.umi_table_ids = b;
    P.n_umi_table = (uint32_t)prm->n_umi_table;
  }

  UmiCall* d_call = S.get<UmiCall>(1);
  UMI_NEED(d_call);
  UmiCall h_call;
  memset(&h_call, 0, sizeof(h_call));
  h_call.first_key = ~0ull;
  h_call.all_unit = 1;
  HIP_TRY(c, hipMemcpyAsync(d_call, &h_call, sizeof(h_call), hipMemcpyHostToDevice, st));

  // ---- parse ----
  UmiRec* d_rec = S.get<UmiRec>(n);
  uint8_t* d_stage = S.get<uint8_t>(n);
  UMI_NEED(d_rec && d_stage);
  {
    ProfScope ps(c, "k_umi_parse");
    // records per tile and the LDS area: what the mean record needs
    // (the index on the device: the header in front of the first record is small beside the records, and this call
    // always gets the whole stream - no first offset is fetched.  fqg_bam_add_tags / fqg_bam2fastq do fetch it, eight
    // bytes and a synchronisation: bam2fastq hands a later PIECE over from byte 0, where nbytes / n is far off)
    const double mean = mem == FQG_MEM_DEVICE_INDEXED ? (double)nbytes / (double)n : (double)(nbytes - offsets[0]) / (double)n;
    const uint32_t T = (uint32_t)std::max(1.0, std::min(64.0, std::floor(((double)kParseStage - 64.0) / (1.1 * mean + 1.0))));
    const uint32_t cap = std::min<uint32_t>((uint32_t)kParseStage, ((uint32_t)(1.15 * mean * T) + 256u + 15u) & ~15u);
    hipLaunchKernelGGL(k_umi_parse, dim3((n + T - 1) / T), dim3(kWave), cap + 32, st, d_buf, nbytes, d_off, n, T, cap, P, d_rec,
                       d_stage, d_call);
  }

  // ---- key tables ----
  const uint64_t cap = pow2_at_least(2ull * n);
  KeyTable U, C;
  NameTable F;
  {  // the seven arrays of the three tables start out all ones: one block, one fill
    unsigned long long* blk = S.get<unsigned long long>(6 * cap + (3 * cap + 1) / 2 + 8, 0xFF);
    UMI_NEED(blk);
    U.keys = blk;
    C.keys = blk + cap;
    F.slots = blk + 2 * cap;
    F.words = blk + 3 * cap;
    uint32_t* firsts32 = reinterpret_cast<uint32_t*>(blk + 6 * cap);
    U.first = firsts32;
    C.first = firsts32 + cap;
    F.first = firsts32 + 2 * cap;
  }
  U.mask = C.mask = F.mask = cap - 1;
  uint32_t* d_uslot = S.get<uint32_t>(n);
  uint32_t* d_cslot = S.get<uint32_t>(n);
  uint32_t* d_fslot = S.get<uint32_t>(n);
  UMI_NEED(d_uslot && d_cslot && d_fslot);
  {
    ProfScope ps(c, "k_umi_insert");
    hipLaunchKernelGGL(k_umi_insert, dim3(blocks_for(n)), dim3(kBlock), 0, st, d_buf, nbytes, n, P, (const UmiRec*)d_rec, d_stage,
                       U, C, F, d_uslot, d_cslot, d_fslot, d_call, measure_int("FQGPU_UMI_INSERT_ABL"));
  }

  // ---- dense ids: flags on the record axis + exclusive prefix ----
  const uint64_t nb = scan64_spans(n);
  uint32_t* d_flag[3];
  unsigned long long *d_loc[3], *d_span[3], *d_tot = S.get<unsigned long long>(8);
  UMI_NEED(d_tot);
  const uint32_t* firsts[3] = {U.first, C.first, F.first};
  {
    ProfScope ps(c, "k_umi_ids");
    // the three flag arrays are one block (one fill), the three scans one launch each
    uint32_t* flags3 = S.get<uint32_t>(3ull * n + 64, 0);
    UMI_NEED(flags3);
    Scan3 t3;
    Scan64 s3{};
    for (int k = 0; k < 3; ++k) {
      d_flag[k] = flags3 + (uint64_t)k * n;
      d_loc[k] = S.get<unsigned long long>(n);
      d_span[k] = S.get<unsigned long long>(nb);
      UMI_NEED(d_loc[k] && d_span[k]);
      t3.first[k] = firsts[k];
      s3.in[k] = t3.flag[k] = d_flag[k];
      s3.local[k] = d_loc[k];
      s3.sums[k] = d_span[k];
    }
    s3.total = d_tot;
    hipLaunchKernelGGL(k_umi_flag3, dim3(blocks_for(cap), 3), dim3(kBlock), 0, st, t3, cap);
    scan64(c, s3, 3, n);
  }
  Prefix pu{d_loc[0], d_span[0]}, pc{d_loc[1], d_span[1]}, pf{d_loc[2], d_span[2]};
  UmiIds ids;
  ids.umi = S.get<uint32_t>(n);
  ids.cell = S.get<uint32_t>(n);
  ids.feat = S.get<uint32_t>(n);
  UMI_NEED(ids.umi && ids.cell && ids.feat);
  {
    ProfScope ps(c, "k_umi_assign");
    hipLaunchKernelGGL(k_umi_assign, dim3(blocks_for(n)), dim3(kBlock), 0, st, n, P, (const UmiRec*)d_rec,
                       (const uint8_t*)d_stage, U, C, F, (const uint32_t*)d_uslot, (const uint32_t*)d_cslot,
                       (const uint32_t*)d_fslot, pu, pc, pf, (const uint32_t*)d_flag[1], ids, d_call);
  }
  // sorted mode: first record and size of every cell (the per-cell counting path works on record ranges) - launched
  // before the host has seen the number of cells (at most n: the arrays are sized for that, the kernels read the
  // count from the device), so that ONE synchronisation brings back everything the host decides on
  uint32_t* d_cell_first = nullptr;
  if (prm->sorted_by_cell) {
    d_cell_first = S.get<uint32_t>((uint64_t)n + 2);
    UMI_NEED(d_cell_first);
    ProfScope ps(c, "k_umi_cell_first");
    hipLaunchKernelGGL(k_umi_cell_first, dim3(blocks_for(cap)), dim3(kBlock), 0, st, cap, C, pc, n, d_cell_first);
    hipLaunchKernelGGL(k_umi_cell_sizes, dim3(blocks_for((uint64_t)n + 1)), dim3(kBlock), 0, st,
                       (const unsigned long long*)d_tot, n, d_cell_first, d_call);
  }
  unsigned long long h_tot[8];
  HIP_TRY(c, hipMemcpyAsync(&h_call, d_call, sizeof(h_call), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h_tot, d_tot, sizeof(h_tot), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_call.table_full & 2u) return fail(c, FQG_ERR_ARG, "fqg_umi_count: a UMI of the call is missing from umi_table_keys");
  if (h_call.table_full) return fail(c, FQG_ERR_STATE, "fqg_umi_count: hash table full");
  for (int k = 0; k < 64; ++k) h_call.n_tags += h_call.spread[0][k];
  out->n_tags_found = h_call.n_tags;
  if (prm->defer_output) {  // the UMIs of the call that are not whitelisted, in order of first appearance (fqg_umi_umis: shards)
    int rc;
    c->umi_n_umis = h_tot[0];
    if ((rc = ensure(c, c->umi_umis, (size_t)std::max<uint64_t>(h_tot[0], 1) * 8))) return rc;
    hipLaunchKernelGGL(k_umi_export_cells, dim3(blocks_for(cap)), dim3(kBlock), 0, st, cap, U, pu,
                       (unsigned long long*)c->umi_umis.p);
  }
  out->n_umis_discarded = h_call.n_umis_disc;
  out->n_cells_discarded = h_call.n_cells_disc;
  const uint64_t n_cells = h_tot[1], n_feat = h_tot[2];
  out->n_cells = n_cells;
  out->n_features = n_feat;
  if (h_call.first_key != ~0ull) {
    out->code = (int32_t)(h_call.first_key & 0xFF);
    out->record = h_call.first_key >> 8;
    const uint32_t* src = out->code == FQG_E_UMI_TOO_MANY_UMIS ? ids.umi
                          : out->code == FQG_E_UMI_TOO_MANY_FEATURES ? ids.feat : ids.cell;
    uint32_t v = 0;
    HIP_TRY(c, hipMemcpy(&v, src + out->record, 4, hipMemcpyDeviceToHost));
    out->aux = v;
    // counters as they stood when the reference stopped are not reproduced: it prints none of them
    return 0;
  }

  // ---- counting: (cell, feature) pairs, new UMIs, the reference's tree where it is not a set, pairs by cell ----
  PairTable Pt;
  memset(&Pt, 0, sizeof(Pt));
  uint8_t* d_new = nullptr;
  uint32_t *d_cell_reads = nullptr, *d_cell_umis = nullptr, *d_cell_pairs = nullptr, *d_pair_of = nullptr;
  float *d_pair_reads = nullptr, *d_pair_umis = nullptr, *d_cellf_reads = nullptr, *d_cellf_umis = nullptr;
  unsigned long long *d_cloc = nullptr, *d_cspan = nullptr;
  uint64_t n_pairs = 0;
  const uint8_t* d_feat_replayed = nullptr;  // (set by the per-cell path when it replays sets)
  const bool unit = h_call.all_unit != 0;
  const uint64_t nbc = scan64_spans(n_cells + 2);
  // CR-sorted input with unit increments: one workgroup per cell, LDS (fqg_umi_cell_kernels.hip).  Anything else -
  // unsorted mode, fractional increments, features or cells beyond the key's bit fields - takes the hash tables.
  static const bool force_hash = getenv("FQGPU_UMI_HASH_PATH") != nullptr;
  const bool use_cells = prm->sorted_by_cell && unit && !force_hash && n_feat < (1ull << kCellFeatBits) &&
                         h_call.max_cell_records < (1u << kCellIdxBits) && n_cells > 0;
  auto hash_path = [&]() -> int {
  // ---- (cell, feature) pairs, (pair, UMI) set ----
  Pt.t.s = S.get<KeySlot>(cap, 0xFF);
  Pt.t.mask = cap - 1;
  Pt.reads = S.get<uint32_t>(cap, 0);
  Pt.umis = S.get<uint32_t>(cap, 0);
  SlotTable T;
  T.s = S.get<KeySlot>(cap, 0xFF);
  T.mask = cap - 1;
  uint32_t* d_pslot = S.get<uint32_t>(n);
  uint32_t* d_tslot = S.get<uint32_t>(n);
  d_new = S.get<uint8_t>(n);
  d_cell_reads = S.get<uint32_t>(n_cells + 2, 0);
  d_cell_umis = S.get<uint32_t>(n_cells + 2, 0);
  UMI_NEED(Pt.t.s && Pt.reads && Pt.umis && T.s && d_pslot && d_tslot && d_new &&
           d_cell_reads && d_cell_umis);
  {
    ProfScope ps(c, "k_umi_count");
    hipLaunchKernelGGL(k_umi_count, dim3(blocks_for(n)), dim3(kBlock), 0, st, n, n, ids, T, Pt, d_pslot, d_tslot, d_call);
    hipLaunchKernelGGL(k_umi_new, dim3(blocks_for(n)), dim3(kBlock), 0, st, n, (const uint32_t*)d_tslot,
                       (const uint32_t*)d_pslot, T, Pt, ids, d_new, d_cell_reads, d_cell_umis, d_call);
  }

  // ---- the reference's UMI container where it is not a set (fqg_umi_rl_kernels.hip, fqg_rl_sim.h) ----
  // records sorted by (pair slot, record index): needed by this stage and by the ordered float sums below
  uint32_t* kp = S.get<uint32_t>(n);
  uint32_t* kc = S.get<uint32_t>(n);
  uint32_t* ix = S.get<uint32_t>(n);
  uint32_t* ko = S.get<uint32_t>(n);
  uint32_t* io = S.get<uint32_t>(n);
  UMI_NEED(kp && kc && ix && ko && io);
  size_t sort_tmp_bytes = 0;
  HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, sort_tmp_bytes, kp, ko, ix, io, (size_t)n, 0, 32, st));
  void* sort_tmp = S.get<uint8_t>(sort_tmp_bytes + 16);
  UMI_NEED(sort_tmp);
  bool sorted_by_pair = false;
  RlCall h_rl;
  memset(&h_rl, 0, sizeof(h_rl));
  if (!prm->strict_set || !unit) {
    ProfScope ps(c, "k_umi_sort_pairs");
    hipLaunchKernelGGL(k_umi_sort_keys, dim3(blocks_for(n)), dim3(kBlock), 0, st, n, (const uint32_t*)d_tslot,
                       (const uint32_t*)d_pslot, (const uint32_t*)ids.cell, kp, kc, ix);
    HIP_TRY(c, rocprim::radix_sort_pairs(sort_tmp, sort_tmp_bytes, kp, ko, ix, io, (size_t)n, 0, 32, st));
    sorted_by_pair = true;
  }
  if (!prm->strict_set) {
    RlCall* d_rl = S.get<RlCall>(1, 0);
    uint32_t* d_sflag = S.get<uint32_t>(n);
    unsigned long long* d_rloc = S.get<unsigned long long>(n);
    unsigned long long* d_rspan = S.get<unsigned long long>(nb);
    RlRuns runs;
    runs.start = S.get<uint32_t>(n);
    runs.len = S.get<uint32_t>(n);
    runs.pslot = S.get<uint32_t>(n);
    runs.flag = S.get<uint32_t>(n, 0xFF);
    uint32_t* d_flagged = S.get<uint32_t>(n);
    uint32_t* d_fk0 = S.get<uint32_t>(n);
    UMI_NEED(d_rl && d_sflag && d_rloc && d_rspan && runs.start && runs.len && runs.pslot && runs.flag && d_flagged && d_fk0);
    {
      ProfScope ps(c, "k_rl_detect");
      hipLaunchKernelGGL(k_rl_starts, dim3(blocks_for(n)), dim3(kBlock), 0, st, n, (const uint32_t*)ko, d_sflag);
      scan64(c, d_sflag, d_rloc, d_rspan, d_tot + 6, n);
      hipLaunchKernelGGL(k_rl_detect, dim3(blocks_for(n)), dim3(kBlock), 0, st, n, (const uint32_t*)ko, (const uint32_t*)io,
                         (const uint32_t*)d_sflag, Prefix{d_rloc, d_rspan}, (const uint32_t*)ids.umi,
                         (const uint8_t*)d_new, runs, d_flagged, d_fk0, d_rl);
    }
    HIP_TRY(c, hipMemcpyAsync(&h_rl, d_rl, sizeof(h_rl), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h_tot, d_tot, sizeof(h_tot), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const uint32_t n_runs = (uint32_t)h_tot[6], n_flagged = h_rl.n_flagged;
    if (n_flagged) {
      {  // which features these sets belong to (fqg_umi_replayed_features)
        uint8_t* d_feat_flag = S.get<uint8_t>((uint64_t)n_feat + 2, 0);
        UMI_NEED(d_feat_flag);
        hipLaunchKernelGGL(k_umi_mark_replayed, dim3(blocks_for(n_flagged)), dim3(kBlock), 0, st, n_flagged,
                           (const uint32_t*)d_flagged, (const uint32_t*)runs.pslot, Pt, d_feat_flag);
        d_feat_replayed = d_feat_flag;
      }
      // where every flagged run keeps its final array: at most 1 + 8 nodes per record of the run, 128-byte aligned
      std::vector<uint32_t> h_len(n_flagged), h_off(n_flagged);
      uint32_t* d_flen = S.get<uint32_t>(n_flagged);
      uint32_t* d_foff = S.get<uint32_t>(n_flagged);
      uint32_t* d_fext = S.get<uint32_t>(n_flagged, 0);
      UMI_NEED(d_flen && d_foff && d_fext);
      hipLaunchKernelGGL(k_rl_flag_lens, dim3(blocks_for(n_flagged)), dim3(kBlock), 0, st, n_flagged,
                         (const uint32_t*)d_flagged, (const uint32_t*)runs.len, d_flen);
      HIP_TRY(c, hipMemcpyAsync(h_len.data(), d_flen, (size_t)n_flagged * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      uint32_t cap_nodes = 1u + 8u * h_rl.max_flagged_len + 2048u;
      cap_nodes = (cap_nodes + 63u) & ~63u;
      uint32_t mcap = 64;
      while (mcap < h_rl.max_len) mcap <<= 1;  // (a power of two: the member sort pads to one)
      uint64_t arena_nodes = 0;
      for (uint32_t f = 0; f < n_flagged; ++f) {
        h_off[f] = (uint32_t)arena_nodes;
        arena_nodes += ((uint64_t)std::min<uint64_t>(cap_nodes, 1ull + 8ull * h_len[f]) + 63u) & ~63ull;
        if (arena_nodes >= 0xFFFFFFFFull) return fail(c, FQG_ERR_STATE, "fqg_umi_count: too many replayed UMI sets");
      }
      uint16_t* d_arena = S.get<uint16_t>(arena_nodes + 64);
      UMI_NEED(d_arena);
      HIP_TRY(c, hipMemcpyAsync(d_foff, h_off.data(), (size_t)n_flagged * 4, hipMemcpyHostToDevice, st));
      RlReplayArgs A;
      memset(&A, 0, sizeof(A));
      if (prm->sorted_by_cell) {
        ProfScope ps(c, "k_rl_chains");
        unsigned long long* ck = S.get<unsigned long long>(n_runs);
        unsigned long long* cko = S.get<unsigned long long>(n_runs);
        uint32_t* cv = S.get<uint32_t>(n_runs);
        uint32_t* cvo = S.get<uint32_t>(n_runs);
        uint32_t* pos = S.get<uint32_t>(n_runs);
        uint32_t* ik = S.get<uint32_t>(n_flagged);
        uint32_t* iko = S.get<uint32_t>(n_flagged);
        uint32_t* iv = S.get<uint32_t>(n_flagged);
        uint32_t* ivo = S.get<uint32_t>(n_flagged);
        UMI_NEED(ck && cko && cv && cvo && pos && ik && iko && iv && ivo);
        hipLaunchKernelGGL(k_rl_chain_keys, dim3(blocks_for(n_runs)), dim3(kBlock), 0, st, n_runs,
                           (const uint32_t*)runs.pslot, Pt, ck, cv);
        size_t tb = 0, tb2 = 0;
        HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, tb, ck, cko, cv, cvo, (size_t)n_runs, 0, 64, st));
        HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, tb2, ik, iko, iv, ivo, (size_t)n_flagged, 0, 32, st));
        void* tmp2 = S.get<uint8_t>(std::max(tb, tb2) + 16);
        UMI_NEED(tmp2);
        HIP_TRY(c, rocprim::radix_sort_pairs(tmp2, tb, ck, cko, cv, cvo, (size_t)n_runs, 0, 64, st));
        hipLaunchKernelGGL(k_rl_positions, dim3(blocks_for(n_runs)), dim3(kBlock), 0, st, n_runs, (const uint32_t*)cvo, pos);
        hipLaunchKernelGGL(k_rl_item_keys, dim3(blocks_for(n_flagged)), dim3(kBlock), 0, st, n_flagged,
                           (const uint32_t*)d_flagged, (const uint32_t*)pos, ik, iv);
        HIP_TRY(c, rocprim::radix_sort_pairs(tmp2, tb2, ik, iko, iv, ivo, (size_t)n_flagged, 0, 32, st));
        A.chain_runs = cvo;
        A.chain_key = cko;
        A.pos_of_run = pos;
        A.items = ivo;
      }  // else: every (cell, feature) has a tree of its own (src/bam_umi_count.c:468-479), no history
      A.flagged = d_flagged;
      A.n_items = n_flagged;
      A.runs = runs;
      A.order = io;
      A.umi_id = ids.umi;
      A.cell_id = ids.cell;
      A.is_new = d_new;
      A.flag_k0 = d_fk0;
      A.flag_off = d_foff;
      A.flag_ext = d_fext;
      A.arena = d_arena;
      A.cap = cap_nodes;
      A.mcap = mcap;
      A.pair_umis = Pt.umis;
      A.cell_umis = d_cell_umis;
      A.n_new_spread = &d_call->spread[2][0];
      A.call = d_rl;
      const uint64_t work_bytes = rl_work_bytes(cap_nodes, mcap);
      const unsigned grid = (unsigned)std::min<uint32_t>(A.n_items, 1024u);
      A.in_lds = work_bytes <= 150u * 1024u;
      if (!A.in_lds) {
        A.scratch_stride = (work_bytes + 255) & ~255ull;
        A.scratch = S.get<uint8_t>(A.scratch_stride * grid);
        UMI_NEED(A.scratch);
      }
      if (A.in_lds && work_bytes > 48u * 1024u) {  // (raised per device and kernel, for the whole process: raise_dynamic_lds)
        const int rcl = raise_dynamic_lds(c, reinterpret_cast<const void*>(k_rl_replay), (size_t)work_bytes);
        if (rcl) return rcl;
      }
      {
        ProfScope ps(c, "k_rl_replay");
        hipLaunchKernelGGL(k_rl_replay, dim3(grid), dim3(kWave), A.in_lds ? (size_t)work_bytes : 0, st, A);
      }
      HIP_TRY(c, hipMemcpyAsync(&h_rl, d_rl, sizeof(h_rl), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      HIP_TRY(c, hipGetLastError());
    }
    if (getenv("FQGPU_RL_DEBUG"))
      fprintf(stderr, "[rl] runs %u flagged %u max_len %u max_flagged_len %u overwrites %u lookback_runs %u changed %u undefined %u "
              "ticks(100MHz): replay %llu (build %llu loop %llu) lookback %llu store %llu\n", n_runs, n_flagged, h_rl.max_len, h_rl.max_flagged_len,
              h_rl.overwrites, h_rl.lookback_runs, h_rl.changed, (unsigned)h_rl.undefined, h_rl.clk_replay, h_rl.clk_build, h_rl.clk_loop, h_rl.clk_lookback, h_rl.clk_store);
    out->rl_replayed = n_flagged;
    out->rl_changed = h_rl.changed;
    out->rl_undefined = h_rl.undefined;
    out->rl_unresolved = h_rl.overflow ? 1 : 0;
  }

  // ---- float32 counters ----
  d_pair_reads = S.get<float>(cap, 0);
  d_pair_umis = S.get<float>(cap, 0);
  d_cellf_reads = S.get<float>(n_cells + 2, 0);
  d_cellf_umis = S.get<float>(n_cells + 2, 0);
  UMI_NEED(d_pair_reads && d_pair_umis && d_cellf_reads && d_cellf_umis);
  if (unit) {
    ProfScope ps(c, "k_umi_sums");
    hipLaunchKernelGGL(k_umi_unit_sums, dim3(blocks_for(cap)), dim3(kBlock), 0, st, cap, (const uint32_t*)Pt.reads,
                       (const uint32_t*)Pt.umis, d_pair_reads, d_pair_umis);
    hipLaunchKernelGGL(k_umi_unit_sums, dim3(blocks_for(n_cells + 1)), dim3(kBlock), 0, st, n_cells + 1,
                       (const uint32_t*)d_cell_reads, (const uint32_t*)d_cell_umis, d_cellf_reads, d_cellf_umis);
  } else {
    // fractional increments (NH > 1, several genes): replay the additions in record order
    ProfScope ps(c, "k_umi_sums_ordered");
    for (int pass = 0; pass < 2; ++pass) {
      if (pass || !sorted_by_pair)
        HIP_TRY(c, rocprim::radix_sort_pairs(sort_tmp, sort_tmp_bytes, pass ? kc : kp, ko, ix, io, (size_t)n, 0, 32, st));
      hipLaunchKernelGGL(k_umi_sums_sorted, dim3(blocks_for(n)), dim3(kBlock), 0, st, n, (const uint32_t*)ko,
                         (const uint32_t*)io, (const UmiRec*)d_rec, (const uint8_t*)d_new,
                         pass ? d_cellf_reads : d_pair_reads, pass ? d_cellf_umis : d_pair_umis);
    }
    hipLaunchKernelGGL(k_umi_db_totals, dim3(1), dim3(64), 0, st, n, n, (const UmiRec*)d_rec, (const uint32_t*)d_tslot,
                       (const uint8_t*)d_new, d_call, prm->db_start_reads, prm->db_start_umi,
                       (uint32_t)std::min<uint64_t>(prm->db_skip, n));
  }

  // ---- pairs grouped by cell, output ----
  d_cell_pairs = S.get<uint32_t>(n_cells + 2, 0);
  uint32_t* d_cursor = S.get<uint32_t>(n_cells + 2, 0);
  d_cloc = S.get<unsigned long long>(n_cells + 2);
  d_cspan = S.get<unsigned long long>(nbc);
  UMI_NEED(d_cell_pairs && d_cursor && d_cloc && d_cspan);
  {
    ProfScope ps(c, "k_umi_pairs");
    hipLaunchKernelGGL(k_umi_pairs_count, dim3(blocks_for(cap)), dim3(kBlock), 0, st, cap, Pt, d_cell_pairs);
    scan64(c, d_cell_pairs, d_cloc, d_cspan, d_tot + 3, n_cells + 2);
  }
  HIP_TRY(c, hipMemcpyAsync(h_tot, d_tot, sizeof(h_tot), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  n_pairs = h_tot[3];
  const Prefix cstart{d_cloc, d_cspan};
  d_pair_of = S.get<uint32_t>(n_pairs);
  UMI_NEED(d_pair_of);
  if (n_pairs) {
    ProfScope ps(c, "k_umi_pairs");
    hipLaunchKernelGGL(k_umi_pairs_fill, dim3(blocks_for(cap)), dim3(kBlock), 0, st, cap, Pt, cstart, d_cursor, d_pair_of);
  }
    return 0;
  };
  auto cell_path = [&]() -> int {
#include "fqg_umi_cell_path.inc"
    return 0;
  };
  {
    const int rc_count = use_cells ? cell_path() : hash_path();
    if (rc_count) return rc_count;
  }
  const Prefix cstart{d_cloc, d_cspan};
  // what the output step needs, kept with the scratch memory it points into
  UmiState* us = new UmiState();
  us->scratch = S_owner.release();
  us->A.Pt = Pt;
  us->A.start = cstart;
  us->A.cell_pairs = d_cell_pairs;
  us->A.pair_of = d_pair_of;
  us->A.pair_reads = d_pair_reads;
  us->A.pair_umis = d_pair_umis;
  us->A.cell_umis = d_cellf_umis;
  us->A.P = P;
  us->A.n_cells = (uint32_t)n_cells;
  us->A.remap = nullptr;
  us->A.pairs_by_feature = use_cells ? 1 : 0;
  us->A.cell_offset = 0;
  us->d_call = d_call;
  us->d_tot = d_tot;
  us->n_pairs = n_pairs;
  us->rec_feat = ids.feat;
  us->feat_replayed = d_feat_replayed;
  us->n_records = n;
  us->n_features = n_feat;
  c->umi_state = us;
  // names and cells in id order
  {
    int rc;
    if ((rc = ensure(c, c->umi_names, (size_t)std::max<uint64_t>(n_feat, 1) * kFeatIdMaxLen))) return rc;
    if ((rc = ensure(c, c->umi_cells, (size_t)std::max<uint64_t>(n_cells, 1) * 8))) return rc;
    ProfScope ps(c, "k_umi_export");
    hipLaunchKernelGGL(k_umi_export_features, dim3(blocks_for(cap)), dim3(kBlock), 0, st, d_buf, cap, F, pf,
                       (const UmiRec*)d_rec, (char*)c->umi_names.p);
    hipLaunchKernelGGL(k_umi_export_cells, dim3(blocks_for(cap)), dim3(kBlock), 0, st, cap, C, pc,
                       (unsigned long long*)c->umi_cells.p);
  }
  HIP_TRY(c, hipMemcpyAsync(&h_call, d_call, sizeof(h_call), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  HIP_TRY(c, hipGetLastError());
  if (h_call.table_full) return fail(c, FQG_ERR_STATE, "fqg_umi_count: hash table full");
  for (int k = 0; k < 64; ++k) {
    h_call.n_counted += h_call.spread[1][k];
    h_call.n_new += h_call.spread[2][k];
  }
  out->n_counted = h_call.n_counted;
  out->n_new = h_call.n_new;
  out->unit_increments = unit ? 1 : 0;
  if (unit) {
    out->tot_reads = h_call.n_counted > 16777216ull ? 16777216.0f : (float)h_call.n_counted;
    out->tot_umi = h_call.n_new > 16777216ull ? 16777216.0f : (float)h_call.n_new;
  } else {
    out->tot_reads = h_call.db_reads;
    out->tot_umi = h_call.db_umi;
  }
  c->umi_n_features = n_feat;
  c->umi_n_cells = n_cells;
  if (prm->defer_output) return 0;
  const int rc_emit = fqg_umi_emit(c, nullptr, 0, 0, out);
  umi_drop_state(c);
  return rc_emit;
}

int fqg_umi_emit(fqg_ctx* c, const uint32_t* feat_remap, uint64_t n_remap, uint32_t cell_offset, fqg_umi_result* out) {
  if (!c || !out || (n_remap && !feat_remap)) return FQG_ERR_ARG;
  UmiState* us = (UmiState*)c->umi_state;
  if (!us) return fail(c, FQG_ERR_STATE, "fqg_umi_emit: no counted state (fqg_umi_count with defer_output first)");
  HIP_TRY(c, hipSetDevice(c->device));
  Scratch& S = *us->scratch;
  hipStream_t st = c->stream;
  const uint64_t n_pairs = us->n_pairs;
  c->umi_n_entries[0] = c->umi_n_entries[1] = 0;
  out->n_entries[0] = out->n_entries[1] = out->total[0] = out->total[1] = 0;
  if (!n_pairs) return 0;
  EmitArgs A = us->A;
  A.cell_offset = cell_offset;
  if (feat_remap) {
    if (n_remap <= c->umi_n_features) return fail(c, FQG_ERR_ARG, "fqg_umi_emit: feat_remap must cover ids 0..n_features");
    uint32_t* d_map = S.get<uint32_t>(n_remap);
    UMI_NEED(d_map);
    HIP_TRY(c, hipMemcpyAsync(d_map, feat_remap, (size_t)n_remap * 4, hipMemcpyHostToDevice, st));
    A.remap = d_map;
  }
  UmiEntry* d_su = S.get<UmiEntry>(n_pairs, 0xFF);
  UmiEntry* d_sr = S.get<UmiEntry>(n_pairs, 0xFF);
  UMI_NEED(d_su && d_sr);
  A.out_u = d_su;
  A.out_r = d_sr;
  HIP_TRY(c, hipMemsetAsync(&us->d_call->tot[0], 0, 16, st));
  HIP_TRY(c, hipMemsetAsync(&us->d_call->tot_spread[0][0], 0, sizeof(us->d_call->tot_spread), st));
  {
    ProfScope ps(c, "k_umi_emit");
    hipLaunchKernelGGL(k_umi_emit, dim3(A.n_cells), dim3(kBlock), 0, st, A, us->d_call);
  }
  // close the gaps
  const uint64_t nbp = scan64_spans(n_pairs);
  for (int w = 0; w < 2; ++w) {
    ProfScope ps(c, "k_umi_compact");
    uint32_t* fl = S.get<uint32_t>(n_pairs);
    unsigned long long* lo = S.get<unsigned long long>(n_pairs);
    unsigned long long* sp = S.get<unsigned long long>(nbp);
    UMI_NEED(fl && lo && sp);
    const UmiEntry* src = w ? d_sr : d_su;
    hipLaunchKernelGGL(k_umi_entry_flags, dim3(blocks_for(n_pairs)), dim3(kBlock), 0, st, (uint32_t)n_pairs, src, fl);
    scan64(c, fl, lo, sp, us->d_tot + 4 + w, n_pairs);
    int rc;
    if ((rc = ensure(c, c->umi_entries[w], (size_t)n_pairs * sizeof(UmiEntry)))) return rc;
    hipLaunchKernelGGL(k_umi_compact, dim3(blocks_for(n_pairs)), dim3(kBlock), 0, st, (uint32_t)n_pairs, src,
                       (const uint32_t*)fl, Prefix{lo, sp}, (UmiEntry*)c->umi_entries[w].p);
  }
  UmiCall h_call;
  unsigned long long h_tot[8];
  HIP_TRY(c, hipMemcpyAsync(&h_call, us->d_call, sizeof(h_call), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h_tot, us->d_tot, sizeof(h_tot), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  HIP_TRY(c, hipGetLastError());
  out->n_entries[0] = h_tot[4];
  out->n_entries[1] = h_tot[5];
  out->total[0] = h_call.tot[0];
  out->total[1] = h_call.tot[1];
  for (int k = 0; k < 64; ++k) {
    out->total[0] += h_call.tot_spread[0][k];
    out->total[1] += h_call.tot_spread[1][k];
  }
  c->umi_n_entries[0] = out->n_entries[0];
  c->umi_n_entries[1] = out->n_entries[1];
  return 0;
}

// After fqg_umi_count(defer_output = 1), for runs over several GPUs (fastq_utils_amd/dist.py: umi_count_sharded): the
// feature id of every alignment (0 where it was not counted), and per feature id (1..n_features; [0] unused) whether one
// of its (cell, feature) sets went through the RL_Tree replay - the trees of exactly those features carry state from
// cell to cell (src/range_list.c:187-198), so a later shard needs their earlier alignments.
int fqg_umi_record_features(fqg_ctx* c, uint32_t* feat, uint64_t cap) {
  if (!c || (!feat && cap)) return FQG_ERR_ARG;
  UmiState* us = (UmiState*)c->umi_state;
  if (!us) return fail(c, FQG_ERR_STATE, "fqg_umi_record_features: no counted state (fqg_umi_count with defer_output first)");
  if (cap < us->n_records) return fail(c, FQG_ERR_ARG, "fqg_umi_record_features: buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  if (us->n_records) HIP_TRY(c, hipMemcpy(feat, us->rec_feat, (size_t)us->n_records * 4, hipMemcpyDeviceToHost));
  return 0;
}
int fqg_umi_replayed_features(fqg_ctx* c, uint8_t* flags, uint64_t cap) {
  if (!c || (!flags && cap)) return FQG_ERR_ARG;
  UmiState* us = (UmiState*)c->umi_state;
  if (!us) return fail(c, FQG_ERR_STATE, "fqg_umi_replayed_features: no counted state (fqg_umi_count with defer_output first)");
  if (cap < us->n_features + 1) return fail(c, FQG_ERR_ARG, "fqg_umi_replayed_features: buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  memset(flags, 0, (size_t)us->n_features + 1);
  if (us->feat_replayed) HIP_TRY(c, hipMemcpy(flags, us->feat_replayed, (size_t)us->n_features + 1, hipMemcpyDeviceToHost));
  return 0;
}

int fqg_umi_features(fqg_ctx* c, char* names, uint64_t cap) {
  if (!c || (!names && cap)) return FQG_ERR_ARG;
  if (cap < c->umi_n_features) return fail(c, FQG_ERR_ARG, "fqg_umi_features: buffer too small");
  if (c->umi_n_features)
    HIP_TRY(c, hipMemcpy(names, c->umi_names.p, (size_t)c->umi_n_features * kFeatIdMaxLen, hipMemcpyDeviceToHost));
  return 0;
}

int fqg_umi_umis(fqg_ctx* c, uint64_t* packed, uint64_t cap, uint64_t* n) {
  if (!c || !n || (!packed && cap)) return FQG_ERR_ARG;
  *n = c->umi_n_umis;
  if (!packed) return 0;
  if (cap < c->umi_n_umis) return fail(c, FQG_ERR_ARG, "fqg_umi_umis: buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->umi_n_umis) HIP_TRY(c, hipMemcpy(packed, c->umi_umis.p, (size_t)c->umi_n_umis * 8, hipMemcpyDeviceToHost));
  return 0;
}

int fqg_umi_cells(fqg_ctx* c, uint64_t* packed, uint64_t cap) {
  if (!c || (!packed && cap)) return FQG_ERR_ARG;
  if (cap < c->umi_n_cells) return fail(c, FQG_ERR_ARG, "fqg_umi_cells: buffer too small");
  if (c->umi_n_cells) HIP_TRY(c, hipMemcpy(packed, c->umi_cells.p, (size_t)c->umi_n_cells * 8, hipMemcpyDeviceToHost));
  return 0;
}

int fqg_umi_entries(fqg_ctx* c, int which, fqg_umi_entry* out, uint64_t cap) {
  if (!c || which < 0 || which > 1 || (!out && cap)) return FQG_ERR_ARG;
  const uint64_t m = c->umi_n_entries[which];
  if (cap < m) return fail(c, FQG_ERR_ARG, "fqg_umi_entries: buffer too small");
  static_assert(sizeof(fqg_umi_entry) == sizeof(UmiEntry), "entry layout");
  if (m) HIP_TRY(c, hipMemcpy(out, c->umi_entries[which].p, (size_t)m * sizeof(UmiEntry), hipMemcpyDeviceToHost));
  return 0;
}
