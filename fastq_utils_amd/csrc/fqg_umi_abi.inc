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

#define UMI_NEED(ptr) \
  if (!(ptr)) return fail(c, FQG_ERR_NOMEM, "fqg_umi_count: device allocation failed")

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
// Moves the arena to what the calls so far asked for - only while nothing lives in it: no Scratch of a running
// call, no deferred state.  (When the allocation fails the arena stays empty: hipMalloc per buffer.)  ArenaGrow does so
// at the END of the call that asked for more (declared before what holds the call's Scratch, so destroyed after it):
// the next call then starts with its memory in place.
int arena_regrow(fqg_ctx* c) {
  if (c->umi_state || c->umi_arena_wanted <= c->umi_arena.cap) return 0;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  release(c->umi_arena);
  (void)ensure(c, c->umi_arena, c->umi_arena_wanted + (c->umi_arena_wanted >> 3));
  return 0;
}
struct ArenaGrow {
  fqg_ctx* c;
  ~ArenaGrow() { (void)arena_regrow(c); }
};
struct UmiState {  // what fqg_umi_emit needs from the counting step, with the scratch memory it points into
  std::unique_ptr<Scratch> scratch;
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
  delete (UmiState*)c->umi_state;
  c->umi_state = nullptr;
}
uint64_t pow2_at_least(uint64_t v) {
  uint64_t p = 1024;
  while (p < v) p <<= 1;
  return p;
}
unsigned blocks_for(uint64_t n) { return (unsigned)std::max<uint64_t>(1, (n + kBlock - 1) / kBlock); }

// What the phases of one fqg_umi_count call share: what the caller passed, then what each phase settles for the
// ones behind it.  Lives for the call; the Scratch moves on to the UmiState (umi_keep_state).
struct UmiCount {
  uint64_t nbytes;
  uint32_t n;
  const fqg_umi_params* prm;
  fqg_umi_result* out;
  std::unique_ptr<Scratch> S;
  hipStream_t st;
  // inputs and parameters on the device (the host copies of the whitelists live until the uploads have run)
  const uint8_t* d_buf = nullptr;
  const unsigned long long* d_off = nullptr;
  double mean_record = 0;
  std::vector<unsigned long long> ku_sorted, kc_sorted;
  std::vector<uint32_t> ku_order;
  UmiParams P{};
  UmiCall *d_call = nullptr, h_call{};
  UmiRec* d_rec = nullptr;
  uint8_t* d_stage = nullptr;
  // the tables of UMIs, cells and feature names (cap slots each), the slot of every record in them, the dense ids
  uint64_t cap = 0;
  KeyTable U{}, C{};
  NameTable F{};
  uint32_t *d_uslot = nullptr, *d_cslot = nullptr, *d_fslot = nullptr;
  Prefix pu{}, pc{}, pf{};
  UmiIds ids{};
  unsigned long long *d_tot = nullptr, h_tot[8] = {};
  uint32_t* d_cell_first = nullptr;  // sorted mode: first record of every cell
  // known after the first synchronisation
  bool stopped = false;  // the reference ends at a record of this call: `out` says which, nothing is counted
  uint64_t n_cells = 0, n_feat = 0;
  bool unit = false, by_cells = false;
  // what counting leaves for the output step (either path)
  PairTable Pt{};
  uint8_t* d_new = nullptr;
  uint32_t *d_cell_reads = nullptr, *d_cell_umis = nullptr, *d_cell_pairs = nullptr, *d_pair_of = nullptr;
  float *d_pair_reads = nullptr, *d_pair_umis = nullptr, *d_cellf_reads = nullptr, *d_cellf_umis = nullptr;
  unsigned long long *d_cloc = nullptr, *d_cspan = nullptr;
  uint64_t n_pairs = 0;
  const uint8_t* d_feat_replayed = nullptr;  // (null: no set was replayed)
  template <class T>
  T* get(uint64_t count, int fill = -1) { return S->get<T>(count, fill); }
};

// phase 1: the stream and the record offsets where the kernels read them, for the three kinds of `mem`; the mean record
// (the index on the device: the header in front of the first record is small beside the records, and this call
// always gets the whole stream - no first offset is fetched.  fqg_bam_add_tags / fqg_bam2fastq do fetch it, eight
// bytes and a synchronisation: bam2fastq hands a later PIECE over from byte 0, where nbytes / n is far off)
int umi_inputs(fqg_ctx* c, UmiCount& u, const void* stream, int mem, const uint64_t* offsets) {
  u.mean_record = mem == FQG_MEM_DEVICE_INDEXED ? (double)u.nbytes / (double)u.n : (double)(u.nbytes - offsets[0]) / (double)u.n;
  if (mem == FQG_MEM_HOST) {
    uint8_t* p = u.get<uint8_t>(u.nbytes + 16);
    UMI_NEED(p);
    HIP_TRY(c, hipMemcpyAsync(p, stream, u.nbytes, hipMemcpyHostToDevice, u.st));
    u.d_buf = p;
  } else u.d_buf = (const uint8_t*)stream;
  if (mem == FQG_MEM_DEVICE_INDEXED) u.d_off = reinterpret_cast<const unsigned long long*>(offsets);  // (the caller's, in HBM)
  else {
    unsigned long long* p = u.get<unsigned long long>(u.n);
    UMI_NEED(p);
    HIP_TRY(c, hipMemcpyAsync(p, offsets, (size_t)u.n * 8, hipMemcpyHostToDevice, u.st));
    u.d_off = p;
  }
  return 0;
}

// phase 2: the parameters as the kernels take them, the whitelists and the UMI table uploaded, the call's counters
int umi_parameters(fqg_ctx* c, UmiCount& u) {
  const fqg_umi_params* prm = u.prm;
  UmiParams& P = u.P;
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
  if (prm->known_umis) {
    P.have_known_umis = 1;
    std::vector<std::pair<unsigned long long, uint32_t>> v;
    for (uint64_t i = 0; i < prm->n_known_umis; ++i) {
      const unsigned long long x = prm->known_umis[i];
      bool dup = false;
      for (auto& e : v) dup |= e.first == x;  // (whitelists are small; keep file order exact)
      if (!dup) v.push_back({x, (uint32_t)v.size()});
    }
    std::sort(v.begin(), v.end());
    for (auto& e : v) {
      u.ku_sorted.push_back(e.first);
      u.ku_order.push_back(e.second);
    }
    P.n_known_umis = (uint32_t)v.size();
    unsigned long long* a = u.get<unsigned long long>(v.size());
    uint32_t* b = u.get<uint32_t>(v.size());
    UMI_NEED(a && b);
    if (!v.empty()) {
      HIP_TRY(c, hipMemcpyAsync(a, u.ku_sorted.data(), v.size() * 8, hipMemcpyHostToDevice, u.st));
      HIP_TRY(c, hipMemcpyAsync(b, u.ku_order.data(), v.size() * 4, hipMemcpyHostToDevice, u.st));
    }
    P.known_umis_sorted = a;
    P.known_umis_order = b;
  }
  if (prm->known_cells) {
    P.have_known_cells = 1;
    u.kc_sorted.assign(prm->known_cells, prm->known_cells + prm->n_known_cells);
    std::sort(u.kc_sorted.begin(), u.kc_sorted.end());
    u.kc_sorted.erase(std::unique(u.kc_sorted.begin(), u.kc_sorted.end()), u.kc_sorted.end());
    P.n_known_cells = (uint32_t)u.kc_sorted.size();
    unsigned long long* a = u.get<unsigned long long>(u.kc_sorted.size());
    UMI_NEED(a);
    if (!u.kc_sorted.empty())
      HIP_TRY(c, hipMemcpyAsync(a, u.kc_sorted.data(), u.kc_sorted.size() * 8, hipMemcpyHostToDevice, u.st));
    P.known_cells_sorted = a;
  }
  if (prm->umi_table_keys) {
    if (!prm->umi_table_ids || prm->n_umi_table >= 0xFFFFFFFFull) return fail(c, FQG_ERR_ARG, "fqg_umi_count: umi_table_ids / n_umi_table");
    unsigned long long* a = u.get<unsigned long long>(prm->n_umi_table);
    uint32_t* b = u.get<uint32_t>(prm->n_umi_table);
    UMI_NEED(a && b);
    if (prm->n_umi_table) {
      HIP_TRY(c, hipMemcpyAsync(a, prm->umi_table_keys, (size_t)prm->n_umi_table * 8, hipMemcpyHostToDevice, u.st));
      HIP_TRY(c, hipMemcpyAsync(b, prm->umi_table_ids, (size_t)prm->n_umi_table * 4, hipMemcpyHostToDevice, u.st));
    }
    P.umi_table_keys = a;
    P.umi_table_ids = b;
    P.n_umi_table = (uint32_t)prm->n_umi_table;
  }
  u.d_call = u.get<UmiCall>(1);
  UMI_NEED(u.d_call);
  memset(&u.h_call, 0, sizeof(u.h_call));
  u.h_call.first_key = ~0ull;
  u.h_call.all_unit = 1;
  HIP_TRY(c, hipMemcpyAsync(u.d_call, &u.h_call, sizeof(u.h_call), hipMemcpyHostToDevice, u.st));
  return 0;
}

// phase 3: the fields of every record (records per tile and the LDS area: what the mean record needs), then the key
// tables with every record's UMI, cell and feature name inserted
int umi_parse_and_insert(fqg_ctx* c, UmiCount& u) {
  u.d_rec = u.get<UmiRec>(u.n);
  u.d_stage = u.get<uint8_t>(u.n);
  UMI_NEED(u.d_rec && u.d_stage);
  {
    ProfScope ps(c, "k_umi_parse");
    const double mean = u.mean_record;
    const uint32_t T = (uint32_t)std::max(1.0, std::min(64.0, std::floor(((double)kParseStage - 64.0) / (1.1 * mean + 1.0))));
    const uint32_t lds = std::min<uint32_t>((uint32_t)kParseStage, ((uint32_t)(1.15 * mean * T) + 256u + 15u) & ~15u);
    hipLaunchKernelGGL(k_umi_parse, dim3((u.n + T - 1) / T), dim3(kWave), lds + 32, u.st, u.d_buf, u.nbytes, u.d_off, u.n, T, lds, u.P,
                       u.d_rec, u.d_stage, u.d_call);
  }
  const uint64_t cap = u.cap = pow2_at_least(2ull * u.n);
  {  // the seven arrays of the three tables start out all ones: one block, one fill
    unsigned long long* blk = u.get<unsigned long long>(6 * cap + (3 * cap + 1) / 2 + 8, 0xFF);
    UMI_NEED(blk);
    u.U.keys = blk;
    u.C.keys = blk + cap;
    u.F.slots = blk + 2 * cap;
    u.F.words = blk + 3 * cap;
    uint32_t* firsts32 = reinterpret_cast<uint32_t*>(blk + 6 * cap);
    u.U.first = firsts32;
    u.C.first = firsts32 + cap;
    u.F.first = firsts32 + 2 * cap;
  }
  u.U.mask = u.C.mask = u.F.mask = cap - 1;
  u.d_uslot = u.get<uint32_t>(u.n);
  u.d_cslot = u.get<uint32_t>(u.n);
  u.d_fslot = u.get<uint32_t>(u.n);
  UMI_NEED(u.d_uslot && u.d_cslot && u.d_fslot);
  ProfScope ps(c, "k_umi_insert");
  hipLaunchKernelGGL(k_umi_insert, dim3(blocks_for(u.n)), dim3(kBlock), 0, u.st, u.d_buf, u.nbytes, u.n, u.P, (const UmiRec*)u.d_rec,
                     u.d_stage, u.U, u.C, u.F, u.d_uslot, u.d_cslot, u.d_fslot, u.d_call, measure_int("FQGPU_UMI_INSERT_ABL"));
  return 0;
}

// phase 4: dense ids in order of first appearance: flags on the record axis + exclusive prefix, for the three tables
int umi_dense_ids(fqg_ctx* c, UmiCount& u) {
  const uint64_t cap = u.cap, nb = scan64_spans(u.n);
  uint32_t* d_flag[3];
  unsigned long long *d_loc[3], *d_span[3];
  u.d_tot = u.get<unsigned long long>(8);
  UMI_NEED(u.d_tot);
  const uint32_t* firsts[3] = {u.U.first, u.C.first, u.F.first};
  {
    ProfScope ps(c, "k_umi_ids");
    // the three flag arrays are one block (one fill), the three scans one launch each
    uint32_t* flags3 = u.get<uint32_t>(3ull * u.n + 64, 0);
    UMI_NEED(flags3);
    Scan3 t3;
    Scan64 s3{};
    for (int k = 0; k < 3; ++k) {
      d_flag[k] = flags3 + (uint64_t)k * u.n;
      d_loc[k] = u.get<unsigned long long>(u.n);
      d_span[k] = u.get<unsigned long long>(nb);
      UMI_NEED(d_loc[k] && d_span[k]);
      t3.first[k] = firsts[k];
      s3.in[k] = t3.flag[k] = d_flag[k];
      s3.local[k] = d_loc[k];
      s3.sums[k] = d_span[k];
    }
    s3.total = u.d_tot;
    hipLaunchKernelGGL(k_umi_flag3, dim3(blocks_for(cap), 3), dim3(kBlock), 0, u.st, t3, cap);
    scan64(c, s3, 3, u.n);
  }
  u.pu = Prefix{d_loc[0], d_span[0]};
  u.pc = Prefix{d_loc[1], d_span[1]};
  u.pf = Prefix{d_loc[2], d_span[2]};
  u.ids.umi = u.get<uint32_t>(u.n);
  u.ids.cell = u.get<uint32_t>(u.n);
  u.ids.feat = u.get<uint32_t>(u.n);
  UMI_NEED(u.ids.umi && u.ids.cell && u.ids.feat);
  {
    ProfScope ps(c, "k_umi_assign");
    hipLaunchKernelGGL(k_umi_assign, dim3(blocks_for(u.n)), dim3(kBlock), 0, u.st, u.n, u.P, (const UmiRec*)u.d_rec,
                       (const uint8_t*)u.d_stage, u.U, u.C, u.F, (const uint32_t*)u.d_uslot, (const uint32_t*)u.d_cslot,
                       (const uint32_t*)u.d_fslot, u.pu, u.pc, u.pf, (const uint32_t*)d_flag[1], u.ids, u.d_call);
  }
  // sorted mode: first record and size of every cell (the per-cell counting path works on record ranges) - launched
  // before the host has seen the number of cells (at most n: the arrays are sized for that, the kernels read the
  // count from the device), so that ONE synchronisation brings back everything the host decides on
  if (u.prm->sorted_by_cell) {
    u.d_cell_first = u.get<uint32_t>((uint64_t)u.n + 2);
    UMI_NEED(u.d_cell_first);
    ProfScope ps(c, "k_umi_cell_first");
    hipLaunchKernelGGL(k_umi_cell_first, dim3(blocks_for(cap)), dim3(kBlock), 0, u.st, cap, u.C, u.pc, u.n, u.d_cell_first);
    hipLaunchKernelGGL(k_umi_cell_sizes, dim3(blocks_for((uint64_t)u.n + 1)), dim3(kBlock), 0, u.st,
                       (const unsigned long long*)u.d_tot, u.n, u.d_cell_first, u.d_call);
  }
  return 0;
}

// phase 5: the one synchronisation in front of counting, and what the host decides with it: the tables held
// everything, the numbers of cells and features, the first finding (u.stopped), which counting path
int umi_first_results(fqg_ctx* c, UmiCount& u) {
  fqg_umi_result* out = u.out;
  UmiCall& h_call = u.h_call;
  HIP_TRY(c, hipMemcpyAsync(&h_call, u.d_call, sizeof(h_call), hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipMemcpyAsync(u.h_tot, u.d_tot, sizeof(u.h_tot), hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipStreamSynchronize(u.st));
  if (h_call.table_full & 2u) return fail(c, FQG_ERR_ARG, "fqg_umi_count: a UMI of the call is missing from umi_table_keys");
  if (h_call.table_full) return fail(c, FQG_ERR_STATE, "fqg_umi_count: hash table full");
  for (int k = 0; k < 64; ++k) h_call.n_tags += h_call.spread[0][k];
  out->n_tags_found = h_call.n_tags;
  if (u.prm->defer_output) {  // the UMIs of the call that are not whitelisted, in order of first appearance (fqg_umi_umis: shards)
    int rc;
    c->umi_n_umis = u.h_tot[0];
    if ((rc = ensure(c, c->umi_umis, (size_t)std::max<uint64_t>(u.h_tot[0], 1) * 8))) return rc;
    hipLaunchKernelGGL(k_umi_export_cells, dim3(blocks_for(u.cap)), dim3(kBlock), 0, u.st, u.cap, u.U, u.pu, (unsigned long long*)c->umi_umis.p);
  }
  out->n_umis_discarded = h_call.n_umis_disc;
  out->n_cells_discarded = h_call.n_cells_disc;
  out->n_cells = u.n_cells = u.h_tot[1];
  out->n_features = u.n_feat = u.h_tot[2];
  if (h_call.first_key != ~0ull) {
    out->code = (int32_t)(h_call.first_key & 0xFF);
    out->record = h_call.first_key >> 8;
    const uint32_t* src = out->code == FQG_E_UMI_TOO_MANY_UMIS ? u.ids.umi
                          : out->code == FQG_E_UMI_TOO_MANY_FEATURES ? u.ids.feat : u.ids.cell;
    uint32_t v = 0;
    HIP_TRY(c, hipMemcpy(&v, src + out->record, 4, hipMemcpyDeviceToHost));
    out->aux = v;
    // counters as they stood when the reference stopped are not reproduced: it prints none of them
    u.stopped = true;
    return 0;
  }
  u.unit = h_call.all_unit != 0;
  // CR-sorted input with unit increments: one workgroup per cell, LDS (fqg_umi_cell_kernels.hip).  Anything else -
  // unsorted mode, fractional increments, features or cells beyond the key's bit fields - takes the hash tables.
  static const bool force_hash = getenv("FQGPU_UMI_HASH_PATH") != nullptr;
  u.by_cells = u.prm->sorted_by_cell && u.unit && !force_hash && u.n_feat < (1ull << kCellFeatBits) &&
               h_call.max_cell_records < (1u << kCellIdxBits) && u.n_cells > 0;
  return 0;
}

// ---- the RL_Tree replay: the reference's UMI container where it is not a set (fqg_umi_rl_kernels.hip, fqg_rl_sim.h) ----
// Both counting paths come to it with the runs and the list of flagged ones on the device, RlCall fetched and the
// flagged runs' lengths on the host.  What the paths differ in they write into A themselves: `order`, the by_cell fields.
struct RlReplay {
  uint32_t n_flagged = 0, n_chain = 0;
  RlRuns runs{};
  // the chain - the runs a replayed set may look back into, by (feature, cell): keys and runs, unsorted and sorted
  unsigned long long *ck = nullptr, *cko = nullptr;
  uint32_t *cv = nullptr, *cvo = nullptr, *pos = nullptr;
  uint32_t *d_flagged = nullptr, *d_fk0 = nullptr, *d_flen = nullptr, *d_foff = nullptr, *d_fext = nullptr;
  RlCall *d_rl = nullptr, h_rl{};
  std::vector<uint32_t> h_len, h_off;  // per flagged run: records, first node in the arena (alive until the fetch)
  RlReplayArgs A{};
};
int rl_chain_get(fqg_ctx* c, UmiCount& u, RlReplay& r, uint32_t n_runs) {
  r.ck = u.get<unsigned long long>(n_runs);
  r.cko = u.get<unsigned long long>(n_runs);
  r.cv = u.get<uint32_t>(n_runs);
  r.cvo = u.get<uint32_t>(n_runs);
  r.pos = u.get<uint32_t>(n_runs);
  UMI_NEED(r.ck && r.cko && r.cv && r.cvo && r.pos);
  r.n_chain = n_runs;
  return 0;
}

// where every flagged run keeps its final array: at most 1 + 8 nodes per record of the run, 128-byte aligned
int rl_lay_out(fqg_ctx* c, UmiCount& u, RlReplay& r) {
  const uint32_t cap_nodes = r.A.cap = (1u + 8u * r.h_rl.max_flagged_len + 2048u + 63u) & ~63u;
  r.A.mcap = 64;
  while (r.A.mcap < r.h_rl.max_len) r.A.mcap <<= 1;  // (a power of two: the member sort pads to one)
  uint64_t arena_nodes = 0;
  r.h_off.resize(r.n_flagged);
  for (uint32_t f = 0; f < r.n_flagged; ++f) {
    r.h_off[f] = (uint32_t)arena_nodes;
    arena_nodes += ((uint64_t)std::min<uint64_t>(cap_nodes, 1ull + 8ull * r.h_len[f]) + 63u) & ~63ull;
    if (arena_nodes >= 0xFFFFFFFFull) return fail(c, FQG_ERR_STATE, "fqg_umi_count: too many replayed UMI sets");
  }
  r.A.arena = u.get<uint16_t>(arena_nodes + 64);
  UMI_NEED(r.A.arena);
  HIP_TRY(c, hipMemcpyAsync(r.d_foff, r.h_off.data(), (size_t)r.n_flagged * 4, hipMemcpyHostToDevice, u.st));
  return 0;
}

// the order of the replay: the chain sorted by (feature, cell), the flagged runs by their place in it (inside the caller's "k_rl_chains")
int rl_sort_chains(fqg_ctx* c, UmiCount& u, RlReplay& r) {
  const uint32_t nf = r.n_flagged;
  uint32_t* ik = u.get<uint32_t>(nf);
  uint32_t* iko = u.get<uint32_t>(nf);
  uint32_t* iv = u.get<uint32_t>(nf);
  uint32_t* ivo = u.get<uint32_t>(nf);
  UMI_NEED(ik && iko && iv && ivo);
  size_t tb = 0, tb2 = 0;
  HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, tb, r.ck, r.cko, r.cv, r.cvo, (size_t)r.n_chain, 0, 64, u.st));
  HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, tb2, ik, iko, iv, ivo, (size_t)nf, 0, 32, u.st));
  void* tmp2 = u.get<uint8_t>(std::max(tb, tb2) + 16);
  UMI_NEED(tmp2);
  HIP_TRY(c, rocprim::radix_sort_pairs(tmp2, tb, r.ck, r.cko, r.cv, r.cvo, (size_t)r.n_chain, 0, 64, u.st));
  hipLaunchKernelGGL(k_rl_positions, dim3(blocks_for(r.n_chain)), dim3(kBlock), 0, u.st, r.n_chain, (const uint32_t*)r.cvo, r.pos);
  hipLaunchKernelGGL(k_rl_item_keys, dim3(blocks_for(nf)), dim3(kBlock), 0, u.st, nf, (const uint32_t*)r.d_flagged, (const uint32_t*)r.pos, ik, iv);
  HIP_TRY(c, rocprim::radix_sort_pairs(tmp2, tb2, ik, iko, iv, ivo, (size_t)nf, 0, 32, u.st));
  r.A.chain_runs = r.cvo;
  r.A.chain_key = r.cko;
  r.A.pos_of_run = r.pos;
  r.A.items = ivo;
  return 0;
}

// the arguments both paths share, the worker's arrays in LDS where they fit, the launch, RlCall and what `out` takes from it
int rl_run(fqg_ctx* c, UmiCount& u, RlReplay& r) {
  RlReplayArgs& A = r.A;
  A.flagged = r.d_flagged;
  A.n_items = r.n_flagged;
  A.runs = r.runs;
  A.umi_id = u.ids.umi;
  A.cell_id = u.ids.cell;
  A.is_new = u.d_new;
  A.flag_k0 = r.d_fk0;
  A.flag_off = r.d_foff;
  A.flag_ext = r.d_fext;
  A.pair_umis = u.Pt.umis;
  A.cell_umis = u.d_cell_umis;
  A.n_new_spread = &u.d_call->spread[2][0];
  A.call = r.d_rl;
  const uint64_t work_bytes = rl_work_bytes(A.cap, A.mcap);
  const unsigned grid = (unsigned)std::min<uint32_t>(A.n_items, 1024u);
  A.in_lds = work_bytes <= 150u * 1024u;
  if (!A.in_lds) {
    A.scratch_stride = (work_bytes + 255) & ~255ull;
    A.scratch = u.get<uint8_t>(A.scratch_stride * grid);
    UMI_NEED(A.scratch);
  }
  if (A.in_lds && work_bytes > 48u * 1024u)  // (raised per device and kernel, for the whole process: raise_dynamic_lds)
    NEED(raise_dynamic_lds(c, reinterpret_cast<const void*>(k_rl_replay), (size_t)work_bytes));
  {
    ProfScope ps(c, "k_rl_replay");
    hipLaunchKernelGGL(k_rl_replay, dim3(grid), dim3(kWave), A.in_lds ? (size_t)work_bytes : 0, u.st, A);
  }
  HIP_TRY(c, hipMemcpyAsync(&r.h_rl, r.d_rl, sizeof(r.h_rl), hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipStreamSynchronize(u.st));
  HIP_TRY(c, hipGetLastError());
  u.out->rl_changed = r.h_rl.changed;
  u.out->rl_undefined = r.h_rl.undefined;
  u.out->rl_unresolved = r.h_rl.overflow ? 1 : 0;
  return 0;
}

// ---- counting through hash tables: unsorted mode, fractional increments, ids beyond the per-cell key's bit fields ----
// the runs of the pair order (one per pair), the ones whose UMIs the reference's tree does not keep as a set, their replay
int table_replay(fqg_ctx* c, UmiCount& u, const uint32_t* ko, const uint32_t* io) {
  RlReplay r;
  r.d_rl = u.get<RlCall>(1, 0);
  uint32_t* d_sflag = u.get<uint32_t>(u.n);
  unsigned long long* d_rloc = u.get<unsigned long long>(u.n);
  unsigned long long* d_rspan = u.get<unsigned long long>(scan64_spans(u.n));
  r.runs.start = u.get<uint32_t>(u.n);
  r.runs.len = u.get<uint32_t>(u.n);
  r.runs.pslot = u.get<uint32_t>(u.n);
  r.runs.flag = u.get<uint32_t>(u.n, 0xFF);
  r.d_flagged = u.get<uint32_t>(u.n);
  r.d_fk0 = u.get<uint32_t>(u.n);
  UMI_NEED(r.d_rl && d_sflag && d_rloc && d_rspan && r.runs.start && r.runs.len && r.runs.pslot && r.runs.flag && r.d_flagged && r.d_fk0);
  {
    ProfScope ps(c, "k_rl_detect");
    hipLaunchKernelGGL(k_rl_starts, dim3(blocks_for(u.n)), dim3(kBlock), 0, u.st, u.n, ko, d_sflag);
    scan64(c, d_sflag, d_rloc, d_rspan, u.d_tot + 6, u.n);
    hipLaunchKernelGGL(k_rl_detect, dim3(blocks_for(u.n)), dim3(kBlock), 0, u.st, u.n, ko, io, (const uint32_t*)d_sflag, Prefix{d_rloc, d_rspan},
                       (const uint32_t*)u.ids.umi, (const uint8_t*)u.d_new, r.runs, r.d_flagged, r.d_fk0, r.d_rl);
  }
  HIP_TRY(c, hipMemcpyAsync(&r.h_rl, r.d_rl, sizeof(r.h_rl), hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipMemcpyAsync(u.h_tot, u.d_tot, sizeof(u.h_tot), hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipStreamSynchronize(u.st));
  const uint32_t n_runs = (uint32_t)u.h_tot[6], n_flagged = r.n_flagged = r.h_rl.n_flagged;
  if (n_flagged) {
    uint8_t* d_feat_flag = u.get<uint8_t>((uint64_t)u.n_feat + 2, 0);  // which features these sets belong to (fqg_umi_replayed_features)
    UMI_NEED(d_feat_flag);
    hipLaunchKernelGGL(k_umi_mark_replayed, dim3(blocks_for(n_flagged)), dim3(kBlock), 0, u.st, n_flagged,
                       (const uint32_t*)r.d_flagged, (const uint32_t*)r.runs.pslot, u.Pt, d_feat_flag);
    u.d_feat_replayed = d_feat_flag;
    r.h_len.resize(n_flagged);
    r.d_flen = u.get<uint32_t>(n_flagged);
    r.d_foff = u.get<uint32_t>(n_flagged);
    r.d_fext = u.get<uint32_t>(n_flagged, 0);
    UMI_NEED(r.d_flen && r.d_foff && r.d_fext);
    hipLaunchKernelGGL(k_rl_flag_lens, dim3(blocks_for(n_flagged)), dim3(kBlock), 0, u.st, n_flagged,
                       (const uint32_t*)r.d_flagged, (const uint32_t*)r.runs.len, r.d_flen);
    HIP_TRY(c, hipMemcpyAsync(r.h_len.data(), r.d_flen, (size_t)n_flagged * 4, hipMemcpyDeviceToHost, u.st));
    HIP_TRY(c, hipStreamSynchronize(u.st));
    NEED(rl_lay_out(c, u, r));
    if (u.prm->sorted_by_cell) {
      ProfScope ps(c, "k_rl_chains");
      NEED(rl_chain_get(c, u, r, n_runs));
      hipLaunchKernelGGL(k_rl_chain_keys, dim3(blocks_for(n_runs)), dim3(kBlock), 0, u.st, n_runs,
                         (const uint32_t*)r.runs.pslot, u.Pt, r.ck, r.cv);
      NEED(rl_sort_chains(c, u, r));
    }  // else: every (cell, feature) has a tree of its own (src/bam_umi_count.c:468-479), no history
    r.A.order = io;
    NEED(rl_run(c, u, r));
  }
  if (getenv("FQGPU_RL_DEBUG"))
    fprintf(stderr, "[rl] runs %u flagged %u max_len %u max_flagged_len %u overwrites %u lookback_runs %u changed %u undefined %u "
            "ticks(100MHz): replay %llu (build %llu loop %llu) lookback %llu store %llu\n", n_runs, n_flagged, r.h_rl.max_len, r.h_rl.max_flagged_len,
            r.h_rl.overwrites, r.h_rl.lookback_runs, r.h_rl.changed, (unsigned)r.h_rl.undefined, r.h_rl.clk_replay, r.h_rl.clk_build, r.h_rl.clk_loop, r.h_rl.clk_lookback, r.h_rl.clk_store);
  u.out->rl_replayed = n_flagged;
  return 0;
}

// phase 6, table path: (cell, feature) pairs and the (pair, UMI) set - reads and new UMIs per pair and cell; the records sorted
// by (pair slot, record index) for the replay and the ordered float sums; the float32 counters; the pairs grouped by cell
int umi_count_tables(fqg_ctx* c, UmiCount& u) {
  const uint64_t cap = u.cap, n_cells = u.n_cells;
  u.Pt.t.s = u.get<KeySlot>(u.cap, 0xFF);
  u.Pt.t.mask = u.cap - 1;
  u.Pt.reads = u.get<uint32_t>(u.cap, 0);
  u.Pt.umis = u.get<uint32_t>(u.cap, 0);
  SlotTable T;
  T.s = u.get<KeySlot>(u.cap, 0xFF);
  T.mask = u.cap - 1;
  uint32_t* d_pslot = u.get<uint32_t>(u.n);
  uint32_t* d_tslot = u.get<uint32_t>(u.n);
  u.d_new = u.get<uint8_t>(u.n);
  u.d_cell_reads = u.get<uint32_t>(u.n_cells + 2, 0);
  u.d_cell_umis = u.get<uint32_t>(u.n_cells + 2, 0);
  UMI_NEED(u.Pt.t.s && u.Pt.reads && u.Pt.umis && T.s && d_pslot && d_tslot && u.d_new && u.d_cell_reads && u.d_cell_umis);
  {
    ProfScope ps(c, "k_umi_count");
    hipLaunchKernelGGL(k_umi_count, dim3(blocks_for(u.n)), dim3(kBlock), 0, u.st, u.n, u.n, u.ids, T, u.Pt, d_pslot, d_tslot, u.d_call);
    hipLaunchKernelGGL(k_umi_new, dim3(blocks_for(u.n)), dim3(kBlock), 0, u.st, u.n, (const uint32_t*)d_tslot,
                       (const uint32_t*)d_pslot, T, u.Pt, u.ids, u.d_new, u.d_cell_reads, u.d_cell_umis, u.d_call);
  }
  uint32_t* kp = u.get<uint32_t>(u.n);
  uint32_t* kc = u.get<uint32_t>(u.n);
  uint32_t* ix = u.get<uint32_t>(u.n);
  uint32_t* ko = u.get<uint32_t>(u.n);
  uint32_t* io = u.get<uint32_t>(u.n);
  UMI_NEED(kp && kc && ix && ko && io);
  size_t sort_tmp_bytes = 0;
  HIP_TRY(c, rocprim::radix_sort_pairs(nullptr, sort_tmp_bytes, kp, ko, ix, io, (size_t)u.n, 0, 32, u.st));
  void* sort_tmp = u.get<uint8_t>(sort_tmp_bytes + 16);
  UMI_NEED(sort_tmp);
  bool sorted_by_pair = false;
  if (!u.prm->strict_set || !u.unit) {
    ProfScope ps(c, "k_umi_sort_pairs");
    hipLaunchKernelGGL(k_umi_sort_keys, dim3(blocks_for(u.n)), dim3(kBlock), 0, u.st, u.n, (const uint32_t*)d_tslot,
                       (const uint32_t*)d_pslot, (const uint32_t*)u.ids.cell, kp, kc, ix);
    HIP_TRY(c, rocprim::radix_sort_pairs(sort_tmp, sort_tmp_bytes, kp, ko, ix, io, (size_t)u.n, 0, 32, u.st));
    sorted_by_pair = true;
  }
  if (!u.prm->strict_set) NEED(table_replay(c, u, ko, io));
  // ---- float32 counters ----
  u.d_pair_reads = u.get<float>(cap, 0);
  u.d_pair_umis = u.get<float>(cap, 0);
  u.d_cellf_reads = u.get<float>(n_cells + 2, 0);
  u.d_cellf_umis = u.get<float>(n_cells + 2, 0);
  UMI_NEED(u.d_pair_reads && u.d_pair_umis && u.d_cellf_reads && u.d_cellf_umis);
  if (u.unit) {
    ProfScope ps(c, "k_umi_sums");
    hipLaunchKernelGGL(k_umi_unit_sums, dim3(blocks_for(cap)), dim3(kBlock), 0, u.st, cap, (const uint32_t*)u.Pt.reads,
                       (const uint32_t*)u.Pt.umis, u.d_pair_reads, u.d_pair_umis);
    hipLaunchKernelGGL(k_umi_unit_sums, dim3(blocks_for(n_cells + 1)), dim3(kBlock), 0, u.st, n_cells + 1,
                       (const uint32_t*)u.d_cell_reads, (const uint32_t*)u.d_cell_umis, u.d_cellf_reads, u.d_cellf_umis);
  } else {
    // fractional increments (NH > 1, several genes): replay the additions in record order
    ProfScope ps(c, "k_umi_sums_ordered");
    for (int pass = 0; pass < 2; ++pass) {
      if (pass || !sorted_by_pair)
        HIP_TRY(c, rocprim::radix_sort_pairs(sort_tmp, sort_tmp_bytes, pass ? kc : kp, ko, ix, io, (size_t)u.n, 0, 32, u.st));
      hipLaunchKernelGGL(k_umi_sums_sorted, dim3(blocks_for(u.n)), dim3(kBlock), 0, u.st, u.n, (const uint32_t*)ko,
                         (const uint32_t*)io, (const UmiRec*)u.d_rec, (const uint8_t*)u.d_new,
                         pass ? u.d_cellf_reads : u.d_pair_reads, pass ? u.d_cellf_umis : u.d_pair_umis);
    }
    hipLaunchKernelGGL(k_umi_db_totals, dim3(1), dim3(64), 0, u.st, u.n, u.n, (const UmiRec*)u.d_rec, (const uint32_t*)d_tslot,
                       (const uint8_t*)u.d_new, u.d_call, u.prm->db_start_reads, u.prm->db_start_umi,
                       (uint32_t)std::min<uint64_t>(u.prm->db_skip, u.n));
  }
  u.d_cell_pairs = u.get<uint32_t>(n_cells + 2, 0);
  uint32_t* d_cursor = u.get<uint32_t>(n_cells + 2, 0);
  u.d_cloc = u.get<unsigned long long>(n_cells + 2);
  u.d_cspan = u.get<unsigned long long>(scan64_spans(n_cells + 2));
  UMI_NEED(u.d_cell_pairs && d_cursor && u.d_cloc && u.d_cspan);
  {
    ProfScope ps(c, "k_umi_pairs");
    hipLaunchKernelGGL(k_umi_pairs_count, dim3(blocks_for(cap)), dim3(kBlock), 0, u.st, cap, u.Pt, u.d_cell_pairs);
    scan64(c, u.d_cell_pairs, u.d_cloc, u.d_cspan, u.d_tot + 3, n_cells + 2);
  }
  HIP_TRY(c, hipMemcpyAsync(u.h_tot, u.d_tot, sizeof(u.h_tot), hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipStreamSynchronize(u.st));
  u.n_pairs = u.h_tot[3];
  u.d_pair_of = u.get<uint32_t>(u.n_pairs);
  UMI_NEED(u.d_pair_of);
  if (u.n_pairs) {
    ProfScope ps(c, "k_umi_pairs");
    hipLaunchKernelGGL(k_umi_pairs_fill, dim3(blocks_for(cap)), dim3(kBlock), 0, u.st, cap, u.Pt, Prefix{u.d_cloc, u.d_cspan}, d_cursor, u.d_pair_of);
  }
  return 0;
}

// ---- counting by one workgroup per cell (fqg_umi_cell_kernels.hip): CR-sorted input, unit increments.  The pair
// arrays are laid out per cell: the pairs of a cell start at its first record's index ----
struct CellPairs {  // what the replay on (cell, feature) runs takes over from the counting kernel
  uint32_t *d_pair_mem = nullptr, *d_members = nullptr, *d_slot_hit = nullptr, *d_flagged_slot = nullptr, *d_run_of_slot = nullptr;
  RlCall* d_rl = nullptr;
  uint32_t n_flagged = 0;
};
// the replay on (cell, feature) runs: every pair is a run; the chain holds the runs of the features that have a flagged one
int cells_replay(fqg_ctx* c, UmiCount& u, const CellPairs& p) {
  const uint32_t n_runs = (uint32_t)u.n_pairs, n_flagged = p.n_flagged;
  RlReplay r;
  r.n_flagged = n_flagged;
  r.d_rl = p.d_rl;
  r.runs.start = u.get<uint32_t>(n_runs);
  r.runs.len = u.get<uint32_t>(n_runs);
  r.runs.pslot = u.d_pair_of;
  r.runs.flag = u.get<uint32_t>(n_runs, 0xFF);
  uint32_t* d_run_feat = u.get<uint32_t>(n_runs);
  uint32_t* d_run_mem = u.get<uint32_t>(n_runs);
  uint32_t* d_run_nmem = u.get<uint32_t>(n_runs);
  r.d_flagged = u.get<uint32_t>(n_flagged);
  r.d_fk0 = u.get<uint32_t>(n_flagged);
  r.d_flen = u.get<uint32_t>(n_flagged);
  r.d_foff = u.get<uint32_t>(n_flagged);
  r.d_fext = u.get<uint32_t>(n_flagged, 0);
  UMI_NEED(r.runs.start && r.runs.len && r.runs.flag && d_run_feat && d_run_mem && d_run_nmem && r.d_flagged && r.d_fk0 && r.d_flen &&
           r.d_foff && r.d_fext);
  HIP_TRY(c, hipMemsetAsync(r.d_rl, 0, sizeof(RlCall), u.st));
  uint8_t* d_feat_flag = u.get<uint8_t>((uint64_t)u.n_feat + 2, 0);
  UMI_NEED(d_feat_flag);
  NEED(rl_chain_get(c, u, r, n_runs));
  u.d_feat_replayed = d_feat_flag;
  {
    ProfScope ps(c, "k_rl_detect");
    hipLaunchKernelGGL(k_rl_cell_flags, dim3(blocks_for(n_flagged)), dim3(kBlock), 0, u.st, n_flagged,
                       (const uint32_t*)p.d_flagged_slot, (const uint32_t*)p.d_slot_hit, (const uint32_t*)p.d_run_of_slot,
                       (const KeySlot*)u.Pt.t.s, (const uint32_t*)u.Pt.reads, r.runs, r.d_flagged, r.d_fk0, r.d_flen, d_feat_flag, r.d_rl);
    hipLaunchKernelGGL(k_rl_cell_chain, dim3(blocks_for(n_runs)), dim3(kBlock), 0, u.st, n_runs, (const uint32_t*)u.d_pair_of,
                       (const KeySlot*)u.Pt.t.s, (const uint8_t*)d_feat_flag, (const uint32_t*)u.d_cell_first, (const uint32_t*)p.d_pair_mem,
                       (const uint32_t*)u.Pt.umis, r.runs, d_run_feat, d_run_mem, d_run_nmem, r.ck, r.cv, r.d_rl);
  }
  r.h_len.resize(n_flagged);
  HIP_TRY(c, hipMemcpyAsync(r.h_len.data(), r.d_flen, (size_t)n_flagged * 4, hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipMemcpyAsync(&r.h_rl, r.d_rl, sizeof(r.h_rl), hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipStreamSynchronize(u.st));
  r.n_chain = r.h_rl.n_chain;
  NEED(rl_lay_out(c, u, r));
  {
    ProfScope ps(c, "k_rl_chains");
    NEED(rl_sort_chains(c, u, r));
  }
  r.A.by_cell = 1;
  r.A.rec_feat = u.ids.feat;
  r.A.run_feat = d_run_feat;
  r.A.run_mem = d_run_mem;
  r.A.run_nmem = d_run_nmem;
  r.A.members = p.d_members;
  NEED(rl_run(c, u, r));
  if (getenv("FQGPU_RL_DEBUG"))
    fprintf(stderr, "[rl/cells] runs %u flagged %u max_len %u max_flagged_len %u overwrites %u lookback_runs %u changed %u "
            "ticks(100MHz): replay %llu (build %llu loop %llu) lookback %llu store %llu; slowest run: %llu ticks, %llu records, %llu inserts; most look-back (waiting included) in one run: %llu ticks\n", n_runs, n_flagged, r.h_rl.max_len, r.h_rl.max_flagged_len,
            r.h_rl.overwrites, r.h_rl.lookback_runs, r.h_rl.changed, r.h_rl.clk_replay, r.h_rl.clk_build, r.h_rl.clk_loop, r.h_rl.clk_lookback, r.h_rl.clk_store, r.h_rl.clk_max >> 32, (r.h_rl.clk_max >> 16) & 0xFFFF, r.h_rl.clk_max & 0xFFFF, r.h_rl.clk_max_wait);
  return 0;
}

// phase 6, per-cell path: the counting kernel; the pairs in compact order (they are grouped by cell already: a prefix over the
// cells' pair counts); the replay; the float32 counters (the counts as floats, saturating like repeated += 1.0f)
int umi_count_cells(fqg_ctx* c, UmiCount& u) {
  CellPairs p;
  const uint64_t slots = u.n, n_cells = u.n_cells;
  u.Pt.t.s = u.get<KeySlot>(slots);
  u.Pt.t.mask = 0;
  u.Pt.reads = u.get<uint32_t>(slots);
  u.Pt.umis = u.get<uint32_t>(slots);
  p.d_pair_mem = u.get<uint32_t>(slots);
  uint32_t* d_pair_pos = u.get<uint32_t>(slots);
  p.d_members = u.get<uint32_t>(slots);
  p.d_slot_hit = u.get<uint32_t>(slots, 0xFF);
  p.d_flagged_slot = u.get<uint32_t>(slots);
  p.d_run_of_slot = u.get<uint32_t>(slots);
  u.d_new = u.get<uint8_t>(u.n);
  u.d_cell_reads = u.get<uint32_t>(n_cells + 2, 0);
  u.d_cell_umis = u.get<uint32_t>(n_cells + 2, 0);
  u.d_cell_pairs = u.get<uint32_t>(n_cells + 2, 0);
  u.d_cloc = u.get<unsigned long long>(n_cells + 2);
  u.d_cspan = u.get<unsigned long long>(scan64_spans(n_cells + 2));
  p.d_rl = u.get<RlCall>(1, 0);
  UMI_NEED(u.Pt.t.s && u.Pt.reads && u.Pt.umis && p.d_pair_mem && d_pair_pos && p.d_members && p.d_slot_hit && p.d_flagged_slot &&
           p.d_run_of_slot && u.d_new && u.d_cell_reads && u.d_cell_umis && u.d_cell_pairs && u.d_cloc && u.d_cspan && p.d_rl);
  CellArgs CA;
  memset(&CA, 0, sizeof(CA));
  CA.n = u.n;
  CA.n_cells = (uint32_t)n_cells;
  CA.feat = u.ids.feat;
  CA.umi = u.ids.umi;
  CA.cell_first = u.d_cell_first;
  CA.is_new = u.d_new;
  CA.pair_key = u.Pt.t.s;
  CA.pair_reads = u.Pt.reads;
  CA.pair_umis = u.Pt.umis;
  CA.pair_mem = p.d_pair_mem;
  CA.pair_pos = d_pair_pos;
  CA.members = p.d_members;
  CA.cell_pairs = u.d_cell_pairs;
  CA.cell_reads = u.d_cell_reads;
  CA.cell_umis = u.d_cell_umis;
  CA.slot_hit = p.d_slot_hit;
  CA.flagged_slot = p.d_flagged_slot;
  CA.rl = p.d_rl;
  CA.call = u.d_call;
  // LDS keys: the smallest power of two that holds the largest cell, up to 8192 (64 KiB); larger cells sort in memory
  uint32_t lds_keys = 64;
  while (lds_keys < u.h_call.max_cell_records && lds_keys < 8192u) lds_keys <<= 1;
  CA.lds_keys = lds_keys;
  if (u.h_call.max_cell_records > lds_keys) {
    CA.big_keys = u.get<unsigned long long>(2ull * u.n + 128);
    UMI_NEED(CA.big_keys);
  }
  if (lds_keys * 8u > 48u * 1024u) NEED(raise_dynamic_lds(c, reinterpret_cast<const void*>(k_umi_cells), (size_t)lds_keys * 8u));
  {
    ProfScope ps(c, "k_umi_cells");
    hipLaunchKernelGGL(k_umi_cells, dim3((unsigned)n_cells), dim3(kBlock), (size_t)lds_keys * 8u, u.st, CA);
  }
  {
    ProfScope ps(c, "k_umi_pairs");
    scan64(c, u.d_cell_pairs, u.d_cloc, u.d_cspan, u.d_tot + 3, n_cells + 2);
  }
  RlCall h_rl;
  HIP_TRY(c, hipMemcpyAsync(u.h_tot, u.d_tot, sizeof(u.h_tot), hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipMemcpyAsync(&h_rl, p.d_rl, sizeof(h_rl), hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipStreamSynchronize(u.st));
  u.n_pairs = u.h_tot[3];
  p.n_flagged = u.prm->strict_set ? 0u : h_rl.n_flagged;
  u.d_pair_of = u.get<uint32_t>(u.n_pairs);
  UMI_NEED(u.d_pair_of);
  if (u.n_pairs) {
    ProfScope ps(c, "k_umi_pairs");
    hipLaunchKernelGGL(k_umi_cell_pairs_fill, dim3((unsigned)n_cells), dim3(kBlock), 0, u.st, (uint32_t)n_cells, (const uint32_t*)u.d_cell_first,
                       (const uint32_t*)u.d_cell_pairs, Prefix{u.d_cloc, u.d_cspan}, u.d_pair_of, p.d_run_of_slot);
  }
  if (p.n_flagged) NEED(cells_replay(c, u, p));
  u.out->rl_replayed = p.n_flagged;
  u.d_pair_reads = u.get<float>(slots);
  u.d_pair_umis = u.get<float>(slots);
  u.d_cellf_reads = u.get<float>(n_cells + 2, 0);
  u.d_cellf_umis = u.get<float>(n_cells + 2, 0);
  UMI_NEED(u.d_pair_reads && u.d_pair_umis && u.d_cellf_reads && u.d_cellf_umis);
  ProfScope ps(c, "k_umi_sums");
  hipLaunchKernelGGL(k_umi_cell_unit_sums, dim3((unsigned)n_cells), dim3(kBlock), 0, u.st, (uint32_t)n_cells, (const uint32_t*)u.d_cell_first,
                     (const uint32_t*)u.d_cell_pairs, (const uint32_t*)u.Pt.reads, (const uint32_t*)u.Pt.umis, u.d_pair_reads, u.d_pair_umis);
  hipLaunchKernelGGL(k_umi_unit_sums, dim3(blocks_for(n_cells + 1)), dim3(kBlock), 0, u.st, n_cells + 1,
                     (const uint32_t*)u.d_cell_reads, (const uint32_t*)u.d_cell_umis, u.d_cellf_reads, u.d_cellf_umis);
  return 0;
}

// phase 7: what the output step needs, kept with the scratch memory it points into; names and cells in id order
int umi_keep_state(fqg_ctx* c, UmiCount& u) {
  UmiState* us = new UmiState();
  us->scratch = std::move(u.S);
  us->A.Pt = u.Pt;
  us->A.start = Prefix{u.d_cloc, u.d_cspan};
  us->A.cell_pairs = u.d_cell_pairs;
  us->A.pair_of = u.d_pair_of;
  us->A.pair_reads = u.d_pair_reads;
  us->A.pair_umis = u.d_pair_umis;
  us->A.cell_umis = u.d_cellf_umis;
  us->A.P = u.P;
  us->A.n_cells = (uint32_t)u.n_cells;
  us->A.remap = nullptr;
  us->A.pairs_by_feature = u.by_cells ? 1 : 0;
  us->A.cell_offset = 0;
  us->d_call = u.d_call;
  us->d_tot = u.d_tot;
  us->n_pairs = u.n_pairs;
  us->rec_feat = u.ids.feat;
  us->feat_replayed = u.d_feat_replayed;
  us->n_records = u.n;
  us->n_features = u.n_feat;
  c->umi_state = us;
  NEED(ensure(c, c->umi_names, (size_t)std::max<uint64_t>(u.n_feat, 1) * kFeatIdMaxLen));
  NEED(ensure(c, c->umi_cells, (size_t)std::max<uint64_t>(u.n_cells, 1) * 8));
  ProfScope ps(c, "k_umi_export");
  hipLaunchKernelGGL(k_umi_export_features, dim3(blocks_for(u.cap)), dim3(kBlock), 0, u.st, u.d_buf, u.cap, u.F, u.pf,
                     (const UmiRec*)u.d_rec, (char*)c->umi_names.p);
  hipLaunchKernelGGL(k_umi_export_cells, dim3(blocks_for(u.cap)), dim3(kBlock), 0, u.st, u.cap, u.C, u.pc, (unsigned long long*)c->umi_cells.p);
  return 0;
}

// phase 8: the counters of the call, and the output itself unless the caller asks for it later (fqg_umi_emit)
int umi_finish(fqg_ctx* c, UmiCount& u) {
  fqg_umi_result* out = u.out;
  UmiCall& h_call = u.h_call;
  HIP_TRY(c, hipMemcpyAsync(&h_call, u.d_call, sizeof(h_call), hipMemcpyDeviceToHost, u.st));
  HIP_TRY(c, hipStreamSynchronize(u.st));
  HIP_TRY(c, hipGetLastError());
  if (h_call.table_full) return fail(c, FQG_ERR_STATE, "fqg_umi_count: hash table full");
  for (int k = 0; k < 64; ++k) {
    h_call.n_counted += h_call.spread[1][k];
    h_call.n_new += h_call.spread[2][k];
  }
  out->n_counted = h_call.n_counted;
  out->n_new = h_call.n_new;
  out->unit_increments = u.unit ? 1 : 0;
  if (u.unit) {
    out->tot_reads = h_call.n_counted > 16777216ull ? 16777216.0f : (float)h_call.n_counted;
    out->tot_umi = h_call.n_new > 16777216ull ? 16777216.0f : (float)h_call.n_new;
  } else {
    out->tot_reads = h_call.db_reads;
    out->tot_umi = h_call.db_umi;
  }
  c->umi_n_features = u.n_feat;
  c->umi_n_cells = u.n_cells;
  if (u.prm->defer_output) return 0;
  const int rc_emit = fqg_umi_emit(c, nullptr, 0, 0, out);
  umi_drop_state(c);
  return rc_emit;
}
}  // namespace
}  // extern "C++"

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
  umi_drop_state(c);
  NEED(arena_regrow(c));  // (nothing of an earlier call is alive here)
  ArenaGrow grow_afterwards{c};
  UmiCount u{nbytes, (uint32_t)n_records, prm, out, std::unique_ptr<Scratch>(new Scratch(c)), c->stream};
  NEED(umi_inputs(c, u, stream, mem, offsets));
  NEED(umi_parameters(c, u));
  NEED(umi_parse_and_insert(c, u));
  NEED(umi_dense_ids(c, u));
  NEED(umi_first_results(c, u));
  if (u.stopped) return 0;
  // counting: (cell, feature) pairs, new UMIs, the reference's tree where it is not a set, pairs by cell
  NEED(u.by_cells ? umi_count_cells(c, u) : umi_count_tables(c, u));
  NEED(umi_keep_state(c, u));
  return umi_finish(c, u);
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
