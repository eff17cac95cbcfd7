// fqg_index_abi.inc - host side of the read-name index: fqg_index_*, fqg_names_compare (included by fqg_abi.hip inside
// extern "C").  The three calls that run a pass and report a finding - insert_unique, match / probe_delete, names_compare -
// are argument checks, index_call_begin, what only they do, index_call_arm, their launches, index_call_end, index_finding:
// where they differ, the difference is an argument of those functions.
struct fqg_index {
  fqg_ctx* ctx = nullptr;
  DevBuf slots, names, claims, segs_dev, found, match;
  uint64_t capacity = 0;
  uint64_t rec_cap = 0;          // records names[] / claims[] have room for
  bool keep_names = true;        // false: nobody will look names up in this index (fqg_index_expect_lookups)
  std::vector<fqg_frame*> frames;
  std::vector<IndexSeg> segs;
  uint64_t n_records_total = 0;  // records fed so far = global index of the next frame's first record
  uint64_t n_askers_total = 0;   // records of the asking file(s) matched against the index so far
  uint64_t inserted = 0, matched = 0, name_bytes = 0;
  int fmt = FQG_NAME_UNDEF, is_pe = 0;
  uint32_t flags = 0;
  bool names_once = true;        // no insert has reported a repeated name or a header without '@' (IndexView::n_positional)
};

extern "C++" {
namespace {

int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

int index_alloc_table(fqg_index* ix, uint64_t capacity) {
  fqg_ctx* c = ix->ctx;
  NEED(ensure(c, ix->slots, (size_t)capacity * 8));
  HIP_TRY(c, hipMemsetAsync(ix->slots.p, 0xFF, (size_t)capacity * 8, c->stream));
  ix->capacity = capacity;
  return 0;
}

IndexView index_view(fqg_index* ix) {
  IndexView v;
  v.slots = (unsigned long long*)ix->slots.p;
  v.names = ix->keep_names ? (NameRec*)ix->names.p : nullptr;
  v.claims = (unsigned long long*)ix->claims.p;
  v.mask = ix->capacity - 1;
  static const bool no_positional = getenv("FQGPU_NO_POSITIONAL_MATCH") != nullptr;  // (measurement, tests)
  v.n_positional = ix->keep_names && ix->names.p && ix->names_once && !no_positional ? ix->n_records_total : 0;
  v.segs = (const IndexSeg*)ix->segs_dev.p;
  v.n_segs = (int)ix->segs.size();
  v.fmt = ix->fmt;
  v.is_pe = ix->is_pe;
  v.may_have_nul = (ix->flags & kFlagNul) ? 1 : 0;
  return v;
}

// room in names[] / claims[] for `total` inserted records (kept across growth: record-ordered arrays)
int index_reserve_records(fqg_index* ix, uint64_t total) {
  fqg_ctx* c = ix->ctx;
  if (total <= ix->rec_cap) return 0;
  const uint64_t cap = std::max<uint64_t>(total + total / 8 + 1024, 2 * ix->rec_cap);
  DevBuf names, claims;
  hipError_t e = hipSuccess;
  if (ix->keep_names) e = hipMalloc(&names.p, (size_t)cap * sizeof(NameRec));
  if (e == hipSuccess) e = hipMalloc(&claims.p, (size_t)cap * 8);
  if (e != hipSuccess) {
    if (names.p) (void)hipFree(names.p);
    return fail(c, FQG_ERR_NOMEM, "name index: hipMalloc", e);
  }
  names.cap = (size_t)cap * sizeof(NameRec);
  claims.cap = (size_t)cap * 8;
  const uint64_t used = ix->n_records_total;
  if (used && ix->names.p && names.p)
    (void)hipMemcpyAsync(names.p, ix->names.p, (size_t)used * sizeof(NameRec), hipMemcpyDeviceToDevice, c->stream);
  if (used && ix->claims.p) (void)hipMemcpyAsync(claims.p, ix->claims.p, (size_t)used * 8, hipMemcpyDeviceToDevice, c->stream);
  (void)hipMemsetAsync((char*)claims.p + (size_t)used * 8, 0xFF, (size_t)(cap - used) * 8, c->stream);  // nobody has asked yet
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  release(ix->names);
  release(ix->claims);
  ix->names = names;
  ix->claims = claims;
  ix->rec_cap = cap;
  return 0;
}

int index_upload_segs(fqg_index* ix) {
  fqg_ctx* c = ix->ctx;
  NEED(ensure(c, ix->segs_dev, std::max<size_t>(1, ix->segs.size()) * sizeof(IndexSeg)));
  if (!ix->segs.empty())
    HIP_TRY(c, hipMemcpyAsync(ix->segs_dev.p, ix->segs.data(), ix->segs.size() * sizeof(IndexSeg),
                              hipMemcpyHostToDevice, c->stream));
  return 0;
}

int index_reset_call(fqg_ctx* c) {
  IndexCall z;
  memset(&z, 0, sizeof(z));
  z.first_dup = z.first_wrong = z.first_missing = kNoRecord;
  *c->h_icall = z;
  HIP_TRY(c, hipMemcpyAsync(c->d_icall, c->h_icall, sizeof(IndexCall), hipMemcpyHostToDevice, c->stream));
  return 0;
}

int index_fetch_call(fqg_ctx* c) {
  HIP_TRY(c, hipMemcpyAsync(c->h_icall, c->d_icall, sizeof(IndexCall), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ---- the skeleton of a call.  ix == nullptr is fqg_names_compare: it works on two retained frames, so it needs no
// current frame, uploads no segments, counts no records and leaves last_names_captured alone.
// front: the current frame with its whole line index, the result cleared, the device
int index_call_begin(fqg_ctx* c, const fqg_index* ix, fqg_index_result* out) {
  if (ix) {
    if (!c->frame_valid) return fail(c, FQG_ERR_STATE, "no frame: call fqg_validate first");
    NEED(index_now(c));
  }
  memset(out, 0, sizeof(*out));
  HIP_TRY(c, hipSetDevice(c->device));
  return 0;
}
// ... behind what a call does to the index itself (grow, register, reserve): the segments uploaded, the scalars reset
int index_call_arm(fqg_ctx* c, fqg_index* ix) {
  if (ix) NEED(index_upload_segs(ix));
  return index_reset_call(c);
}
// back: the scalars fetched, any launch error, the pass met each of the n_records once (ablated: a measurement build
// switched work off), last_names_captured.  launch_what: the insert words a launch error itself, the others as HIP_TRY does
int index_call_end(fqg_ctx* c, const fqg_index* ix, uint64_t n_records, int ablated, const char* launch_what) {
  NEED(index_fetch_call(c));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return launch_what ? fail(c, FQG_ERR_HIP, launch_what) : fail(c, FQG_ERR_HIP, "hipGetLastError()", e);
  if (!ix) return 0;
  if (c->h_icall->table_full) return fail(c, FQG_ERR_STATE, "name index full");  // (only an insert raises it)
  if (n_records && c->h_icall->seen != n_records && !measured_wrong(ablated))
    return fail(c, FQG_ERR_STATE, "name index: the pass did not meet every record once");
  c->last_names_captured = c->h_icall->captured;
  return 0;
}

// The earlier of the first header without '@' (`wrong`) and the call's other finding (`other`: a repeated, missing or
// differing name) -> code and record; none: `out` stays cleared.  Both count what the kernel counted, `unit` records each
// (2: the pairs of an interleaved file).  wrong_wins_ties: where the two are one place the header is the finding
void index_finding(fqg_index_result* out, uint64_t wrong, uint64_t other, int other_code, bool wrong_wins_ties, uint64_t unit = 1) {
  if (wrong != kNoRecord && (wrong_wins_ties ? wrong <= other : wrong < other)) {
    out->code = FQG_E_WRONG_HEADER;
    out->record = unit * wrong;
  } else if (other != kNoRecord) {
    out->code = other_code;
    out->record = unit * other;
  }
}

void index_sizes(const fqg_index* ix, uint64_t n_entries, fqg_index_result* out) {
  out->n_entries = n_entries;
  // sizeof(hashtable) + per entry sizeof(INDEX_ENTRY) + len + 1 + sizeof(hashnode)
  out->index_mem = 8 + ix->inserted * (16 + 1 + 24) + ix->name_bytes;
}

unsigned index_grid(fqg_ctx* c, uint64_t n) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)c->cu_count * 16));
}

// ---- names from what the streaming pass captured
// the capture records of the last fqg_validate belong to this frame (FQG_VALIDATE_NAMES, streamed)
// (digests hold no name bytes and are made under one file state: they serve the insert into an index that keeps no name
// records, for that very state - everybody else reads the names through the line index)
bool names_usable(const fqg_ctx* c, const FrameView& fv, const fqg_file_state* st, bool bytes_needed) {
  static const bool off = getenv("FQGPU_NO_NAME_CAPTURE") != nullptr;  // (A/B: always go through the line index)
  if (off || !c->names_img || c->names_img != fv.img || c->names_nbytes != fv.nbytes) return false;
  if (c->names.digests) return !bytes_needed && st->readname_format == c->names.fmt && st->is_pe == c->names.is_pe;
  return true;
}
// record slots of the capture: what k_names_pass and k_build_scatter<0/2> walk
uint64_t names_slots(const fqg_ctx* c) { return (uint64_t)c->names.cr.n_chunks << c->names.k_shift; }
// the lists k_names_pass fills for k_names_rest
int names_prepare(fqg_ctx* c) {
  NEED(ensure(c, c->name_redo, ((names_slots(c) + 63) / 64 + 1) * 8));
  NEED(ensure(c, c->name_redo_chunks, (((size_t)std::max<uint32_t>(c->names.cr.n_chunks, 1) + 15) & ~(size_t)15) + 16));
  c->names.redo_bits = (unsigned long long*)c->name_redo.p;
  c->names.chunk_redo = (uint8_t*)c->name_redo_chunks.p;
  static const int abl = measure_int("FQGPU_NAMES_ABL");
  c->names.ablate = abl;
  return 0;
}
// (measurement knobs: FQGPU_NAMES_BLOCKS_PER_CU, FQGPU_NAMES_DYN_LDS - bytes of unused LDS per workgroup, which caps the
// workgroups a CU holds -, FQGPU_NAMES_NT=0 for plain instead of non-temporal loads of the capture records)
unsigned names_grid(fqg_ctx* c) {
  static const int per_cu = std::max(1, env_int("FQGPU_NAMES_BLOCKS_PER_CU", 16));
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((names_slots(c) + kBlock - 1) / kBlock, (uint64_t)c->cu_count * per_cu));
}
template <bool MATCH, bool NT, bool DIGEST>
void names_pass(fqg_ctx* c, const FrameView& fv, const IndexView& iv, const fqg_file_state* st, uint64_t base, unsigned long long* found) {
  static const unsigned dyn_lds = (unsigned)std::max(0, env_int("FQGPU_NAMES_DYN_LDS", 0));
  hipLaunchKernelGGL((k_names_pass<MATCH, NT, DIGEST>), dim3(names_grid(c)), dim3(kBlock), dyn_lds, c->stream, fv, c->names, iv,
                     st->readname_format, st->is_pe, base, found, c->d_icall);
}
void launch_names_pass(fqg_ctx* c, bool match, const FrameView& fv, const IndexView& iv, const fqg_file_state* st,
                       uint64_t base, unsigned long long* found) {
  static const bool nt = env_int("FQGPU_NAMES_NT", 1) != 0;
  if (match) nt ? names_pass<true, true, false>(c, fv, iv, st, base, found) : names_pass<true, false, false>(c, fv, iv, st, base, found);
  else if (c->names.digests) names_pass<false, true, true>(c, fv, iv, st, base, found);
  else nt ? names_pass<false, true, false>(c, fv, iv, st, base, found) : names_pass<false, false, false>(c, fv, iv, st, base, found);
}

// ---- the table built part by part in LDS from the capture of the current frame (fqg_names_build_kernels.hip) instead of
// one CAS per name: plan, reserve, scatter (one or two levels), parts, spill, finish
constexpr unsigned long long kBuildSpillCap = 1ull << 20;
struct NamesBuild {
  fqg_ctx* c;
  fqg_index* ix;
  const FrameView& fv;
  const fqg_file_state* st;
  uint64_t record_base;
  BuildPlan p;
};

int build_reserve(const NamesBuild& b) {
  fqg_ctx* c = b.c;
  NEED(ensure(c, c->build_keys[0], (size_t)(b.p.cap0 << b.p.bits0) * sizeof(BuildKey)));
  if (b.p.bits1) NEED(ensure(c, c->build_keys[1], (size_t)(b.p.cap1 << b.p.part_bits) * sizeof(BuildKey)));
  NEED(ensure(c, c->build_cursor, b.p.n_cursors * 4));
  NEED(ensure(c, c->build_spill, (size_t)kBuildSpillCap * sizeof(BuildKey)));
  HIP_TRY(c, hipMemsetAsync(c->build_cursor.p, 0, b.p.n_cursors * 4, c->stream));
  return 0;
}

// -> the last level: one bucket per part
BuildLevel build_scatter(const NamesBuild& b) {
  fqg_ctx* c = b.c;
  const BuildPlan& p = b.p;
  const uint64_t mask = b.ix->capacity - 1;
  unsigned int* cur0 = (unsigned int*)c->build_cursor.p;
  BuildLevel L0{(BuildKey*)c->build_keys[0].p, cur0, p.cap0, p.part_log + p.bits1, p.bits0};
  {
    ProfScope ps(c, "k_names_build_scatter0");
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((names_slots(c) + kBuildTile - 1) / kBuildTile, (uint64_t)c->cu_count * 8));
    if (!c->names.digests)  // (an index that keeps name records: keys and names[] from the capture records)
      hipLaunchKernelGGL(k_build_scatter<2>, dim3(grid), dim3(kBuildThreads), 0, c->stream, b.fv, c->names, b.record_base, mask, L0,
                         (const BuildKey*)nullptr, (const unsigned int*)nullptr, 0ull, c->d_icall,
                         b.ix->keep_names ? (NameRec*)b.ix->names.p : (NameRec*)nullptr, b.st->readname_format, b.st->is_pe);
    else
      hipLaunchKernelGGL(k_build_scatter<0>, dim3(grid), dim3(kBuildThreads), 0, c->stream, b.fv, c->names, b.record_base, mask, L0,
                         (const BuildKey*)nullptr, (const unsigned int*)nullptr, 0ull, c->d_icall, (NameRec*)nullptr, 0, 0);
  }
  if (!p.bits1) return L0;
  BuildLevel L1{(BuildKey*)c->build_keys[1].p, cur0 + (1u << p.bits0), p.cap1, p.part_log, p.bits1};
  ProfScope ps(c, "k_names_build_scatter1");
  const unsigned tiles = (unsigned)((p.cap0 + kBuildTile - 1) / kBuildTile);
  hipLaunchKernelGGL(k_build_scatter<1>, dim3(tiles, 1u << p.bits0), dim3(kBuildThreads), 0, c->stream, b.fv, c->names, b.record_base, mask, L1,
                     (const BuildKey*)L0.out, (const unsigned int*)L0.cursor, p.cap0, c->d_icall, (NameRec*)nullptr, 0, 0);
  return L1;
}

template <uint32_t PART_LOG>
void build_parts(const NamesBuild& b, const BuildLevel& last) {
  ProfScope ps(b.c, "k_names_build_parts");
  hipLaunchKernelGGL(k_build_parts<PART_LOG>, dim3(1u << b.p.part_bits), dim3(kBlock), 0, b.c->stream, b.fv, index_view(b.ix), b.record_base,
                     (const BuildKey*)last.out, (const unsigned int*)last.cursor, last.cap, b.ix->n_records_total == 0 ? 0 : 1,
                     (BuildKey*)b.c->build_spill.p, kBuildSpillCap, b.c->d_icall);
}

void build_spill(const NamesBuild& b) {
  ProfScope ps(b.c, "k_names_build_spill");
  hipLaunchKernelGGL(k_build_spill, dim3(64), dim3(kBlock), 0, b.c->stream, b.fv, index_view(b.ix), b.record_base,
                     (const BuildKey*)b.c->build_spill.p, kBuildSpillCap, b.c->d_icall);
}

// the call's scalars; 1: a bucket overflowed (nothing has touched the table)
int build_finish(const NamesBuild& b) {
  NEED(index_fetch_call(b.c));
  // (gigabytes that only this call needs: a context that keeps them is what the next large allocation of the process
  // fails on - the bench's 200 M-pair leg did, with 4 GB free of 288)
  release(b.c->build_keys[0]);
  release(b.c->build_keys[1]);
  return b.c->h_icall->build_overflow ? 1 : 0;
}

// Returns 0 when it ran (the call's scalars hold its counts and findings), 1 when it does not apply or a bucket
// overflowed (nothing has touched the table: the caller takes k_names_pass), < 0 on errors.
int names_build(fqg_ctx* c, fqg_index* ix, const FrameView& fv, const fqg_file_state* st, uint64_t record_base) {
  // (both read on every call: tests switch them within one process)
  const int mode = env_int("FQGPU_NAMES_BUILD", -1);  // 0: never, 1: whenever the table allows it (tests), -1: by size
  const int forced = env_int("FQGPU_BUILD_PART_LOG", 0);  // (A/B)
  const NamesBuild b{c, ix, fv, st, record_base,
                     build_plan(ix->capacity, fv.n_records, ix->n_records_total == 0, mode, forced, kPartLogMin, kPartLogMax)};
  if (!b.p.applies) return 1;
  NEED(build_reserve(b));
  const BuildLevel last = build_scatter(b);
  b.p.part_log == 12 ? build_parts<12>(b, last) : build_parts<13>(b, last);
  build_spill(b);
  return build_finish(b);
}

// rebuild the table at a larger capacity from the retained segments
int index_grow(fqg_index* ix, uint64_t need_names) {
  fqg_ctx* c = ix->ctx;
  uint64_t cap = ix->capacity ? ix->capacity : 1024;
  while (cap < 2 * need_names) cap <<= 1;
  if (cap == ix->capacity) return 0;
  NEED(index_alloc_table(ix, cap));
  NEED(index_upload_segs(ix));
  for (size_t s = 0; s < ix->segs.size(); ++s) {
    if (!ix->segs[s].n_records) continue;  // (a frame whose insert failed: kept for ownership only)
    NEED(index_reset_call(c));
    FrameView fv = ix->frames[s]->fv;
    ProfScope ps(c, "k_index_insert(regrow)");
    IndexView v = index_view(ix);
    v.names = nullptr;  // (the name records of these frames are in place)
    hipLaunchKernelGGL(k_index_insert, dim3(index_grid(c, fv.n_records)), dim3(kBlock), 0, c->stream, fv, v,
                       ix->segs[s].record_base, c->d_icall);
  }
  return 0;
}

// A frame handed to the index stays with it whatever happens next (fqg_index_destroy frees it), but its records count
// only once the insert has succeeded.  Registers the frame and its segment; unless commit() is reached the segment is
// left for ownership only (n_records 0: index_grow skips it) and the index's counts have not moved.
struct SegmentGuard {
  fqg_index* ix;
  bool committed = false;
  SegmentGuard(fqg_index* ix_, fqg_frame* fr) : ix(ix_) {
    ix->frames.push_back(fr);
    ix->segs.push_back(IndexSeg{fr->fv.img, fr->fv.line_end, fr->fv.nbytes, fr->fv.n_records, ix->n_records_total});
  }
  ~SegmentGuard() {
    if (!committed) ix->segs.back().n_records = 0;
  }
  void commit(const IndexCall& call, bool found_none) {
    ix->n_records_total += ix->segs.back().n_records;
    ix->inserted += call.inserted;
    ix->name_bytes += call.name_bytes;
    ix->names_once = ix->names_once && found_none;
    committed = true;
  }
};

// the frame's names into the table: from the capture - the build, or the CAS pass where it does not apply, and behind
// either what they left for the line index -, or all of them through the line index
int insert_launch(fqg_ctx* c, fqg_index* ix, const FrameView& fv, const fqg_file_state* st, uint64_t record_base, bool captured) {
  if (!fv.n_records) return 0;
  if (!captured) {
    ProfScope ps(c, "k_index_insert");
    hipLaunchKernelGGL(k_index_insert, dim3(index_grid(c, fv.n_records)), dim3(kBlock), 0, c->stream, fv, index_view(ix),
                       record_base, c->d_icall);
    return 0;
  }
  NEED(names_prepare(c));
  const int built = names_build(c, ix, fv, st, record_base);
  if (built < 0) return built;
  if (built == 1) {
    NEED(index_reset_call(c));
    ProfScope ps(c, "k_names_insert");
    launch_names_pass(c, false, fv, index_view(ix), st, record_base, nullptr);
  }
  ProfScope ps(c, "k_names_rest");
  hipLaunchKernelGGL(k_names_rest<false>, dim3(c->cu_count * 4), dim3(kBlock), 0, c->stream, fv, c->names, index_view(ix),
                     st->readname_format, st->is_pe, record_base, (unsigned long long*)nullptr, c->d_icall);
  return 0;
}

}  // namespace
}  // extern "C++"

int fqg_index_create(fqg_ctx* c, uint64_t expected_names, fqg_index** out) {
  if (!c || !out) return FQG_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  fqg_index* ix = new fqg_index();
  ix->ctx = c;
  uint64_t cap = 1024;
  while (cap < 2 * expected_names) cap <<= 1;
  int rc = index_alloc_table(ix, cap);
  if (rc) {
    fqg_index_destroy(ix);
    return rc;
  }
  *out = ix;
  return 0;
}

int fqg_index_expect_lookups(fqg_index* ix, int yes) {
  if (!ix) return FQG_ERR_ARG;
  if (ix->n_records_total) return fail(ix->ctx, FQG_ERR_STATE, "fqg_index_expect_lookups: the index is not empty");
  ix->keep_names = yes != 0;
  return 0;
}

void fqg_index_destroy(fqg_index* ix) {
  if (!ix) return;
  (void)hipStreamSynchronize(ix->ctx->stream);
  for (auto* f : ix->frames) fqg_frame_release(f);
  release(ix->slots);
  release(ix->names);
  release(ix->claims);
  release(ix->segs_dev);
  release(ix->found);
  release(ix->match);
  delete ix;
}

uint64_t fqg_index_names_captured(const fqg_ctx* c) { return c ? c->last_names_captured : 0; }
const fqg_frame* fqg_index_frame(const fqg_index* ix, uint64_t k) {
  return (ix && k < ix->frames.size()) ? ix->frames[k] : nullptr;
}
uint64_t fqg_index_n_frames(const fqg_index* ix) { return ix ? ix->frames.size() : 0; }

int fqg_index_insert_unique(fqg_ctx* c, fqg_index* ix, const fqg_file_state* st, fqg_index_result* out) {
  if (!c || !ix || !st || !out || ix->ctx != c) return FQG_ERR_ARG;
  NEED(index_call_begin(c, ix, out));
  fqg_frame* fr = nullptr;
  NEED(fqg_frame_retain(c, &fr));
  if (ix->frames.empty()) {
    ix->fmt = st->readname_format;
    ix->is_pe = st->is_pe;
  }
  ix->flags |= fr->flags;
  const FrameView& fv = fr->fv;
  // grow first: index_grow re-inserts the segments registered so far, and this frame is not yet one of them
  const int grown = 2 * (ix->inserted + fv.n_records) > ix->capacity ? index_grow(ix, ix->inserted + fv.n_records) : 0;
  SegmentGuard seg(ix, fr);  // (from here on every return but the last leaves the frame for ownership only)
  NEED(grown);
  const uint64_t base = ix->segs.back().record_base;
  NEED(index_reserve_records(ix, base + fv.n_records));
  NEED(index_call_arm(c, ix));
  const bool captured = names_usable(c, fv, st, ix->keep_names);
  NEED(insert_launch(c, ix, fv, st, base, captured));
  NEED(index_call_end(c, ix, fv.n_records, captured && c->names.ablate, "k_index_insert"));
  const uint64_t w = c->h_icall->first_wrong;
  // (the kernels know a repeated name by its global record - that is what the table holds -, a header by its record in
  // the frame: the finding is the frame's)
  const uint64_t d = c->h_icall->first_dup == kNoRecord ? kNoRecord : c->h_icall->first_dup - base;
  seg.commit(*c->h_icall, w == kNoRecord && d == kNoRecord);
  index_finding(out, w, d, FQG_E_DUP_NAME, false);  // (strict: they are records, and one record is never both)
  index_sizes(ix, ix->inserted, out);
  return 0;
}

static int index_match_impl(fqg_ctx* c, fqg_index* ix, const fqg_file_state* st, uint64_t* match, fqg_index_result* out) {
  if (!c || !ix || !st || !out || ix->ctx != c) return FQG_ERR_ARG;
  NEED(index_call_begin(c, ix, out));
  if (!ix->claims.p) NEED(index_reserve_records(ix, std::max<uint64_t>(ix->n_records_total, 1)));
  NEED(index_call_arm(c, ix));
  const FrameView fv = c->frame;
  unsigned long long *d_slot = nullptr, *d_match = nullptr;
  if (match && fv.n_records) {
    NEED(ensure(c, ix->found, fv.n_records * 8));
    NEED(ensure(c, ix->match, fv.n_records * 8));
    d_slot = (unsigned long long*)ix->found.p;
    d_match = (unsigned long long*)ix->match.p;
  }
  if (fv.n_records) {
    if (names_usable(c, fv, st, true)) {
      NEED(names_prepare(c));
      {
        ProfScope ps(c, "k_names_match");
        launch_names_pass(c, true, fv, index_view(ix), st, ix->n_askers_total, d_slot);
      }
      ProfScope ps(c, "k_names_rest");
      hipLaunchKernelGGL(k_names_rest<true>, dim3(c->cu_count * 4), dim3(kBlock), 0, c->stream, fv, c->names, index_view(ix),
                         st->readname_format, st->is_pe, ix->n_askers_total, d_slot, c->d_icall);
    } else {
      ProfScope ps(c, "k_index_match_delete");
      hipLaunchKernelGGL(k_index_match_delete, dim3(index_grid(c, fv.n_records)), dim3(kBlock), 0, c->stream, fv,
                         index_view(ix), st->readname_format, st->is_pe, (c->frame_flags & kFlagNul) ? 1 : 0,
                         ix->n_askers_total, d_slot, c->d_icall);
    }
    if (match) {
      {
        ProfScope ps(c, "k_index_probe_resolve");
        hipLaunchKernelGGL(k_index_probe_resolve, dim3((unsigned)((fv.n_records + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           c->stream, fv.n_records, (const unsigned long long*)d_slot, index_view(ix), ix->n_askers_total,
                           d_match);
      }
      HIP_TRY(c, hipMemcpyAsync(match, d_match, fv.n_records * 8, hipMemcpyDeviceToHost, c->stream));
    }
  }
  // (ablated whichever way the names came: names.ablate is what the last names_prepare left, as it has always been read here)
  NEED(index_call_end(c, ix, fv.n_records, c->names.ablate, nullptr));
  ix->matched += c->h_icall->matched;
  ix->n_askers_total += fv.n_records;
  index_finding(out, c->h_icall->first_wrong, c->h_icall->first_missing, FQG_E_UNPAIRED, false);  // (strict: records, as in the insert)
  index_sizes(ix, ix->inserted - ix->matched, out);
  return 0;
}

int fqg_index_match_delete(fqg_ctx* c, fqg_index* ix, const fqg_file_state* st, fqg_index_result* out) {
  return index_match_impl(c, ix, st, nullptr, out);
}

int fqg_index_probe_delete(fqg_ctx* c, fqg_index* ix, const fqg_file_state* st, uint64_t* match, fqg_index_result* out) {
  if (!match && c && c->frame_valid && c->frame.n_records) return FQG_ERR_ARG;
  return index_match_impl(c, ix, st, match, out);
}

int fqg_index_alive(fqg_ctx* c, fqg_index* ix, uint8_t* alive, uint64_t cap) {
  if (!c || !ix || ix->ctx != c || (!alive && cap)) return FQG_ERR_ARG;
  if (cap < ix->n_records_total) return fail(c, FQG_ERR_ARG, "fqg_index_alive: buffer too small");
  if (!ix->n_records_total) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  NEED(index_upload_segs(ix));
  uint8_t* d = nullptr;
  if (hipMalloc((void**)&d, ix->n_records_total) != hipSuccess) return fail(c, FQG_ERR_NOMEM, "fqg_index_alive: device allocation failed");
  (void)hipMemsetAsync(d, 0, ix->n_records_total, c->stream);
  IndexView v = index_view(ix);
  hipLaunchKernelGGL(k_index_alive, dim3((unsigned)((ix->capacity + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, v,
                     ix->n_records_total, d);
  hipError_t e = hipMemcpyAsync(alive, d, ix->n_records_total, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(c, FQG_ERR_HIP, "fqg_index_alive", e);
  return 0;
}

int fqg_names_compare(fqg_ctx* c, const fqg_frame* a, const fqg_file_state* sa, const fqg_frame* b,
                      const fqg_file_state* sb, fqg_index_result* out) {
  if (!c || !a || !sa || !out || (b && !sb)) return FQG_ERR_ARG;
  NEED(index_call_begin(c, nullptr, out));
  NEED(index_call_arm(c, nullptr));
  const int interleaved = b ? 0 : 1;
  const uint64_t n_pairs = interleaved ? a->fv.n_records / 2 : std::min(a->fv.n_records, b->fv.n_records);
  if (n_pairs) {
    ProfScope ps(c, "k_names_compare");
    const uint32_t fl = a->flags | (b ? b->flags : 0u);
    hipLaunchKernelGGL(k_names_compare, dim3(index_grid(c, n_pairs)), dim3(kBlock), 0, c->stream, a->fv,
                       sa->readname_format, sa->is_pe, b ? b->fv : a->fv, b ? sb->readname_format : sa->readname_format,
                       b ? sb->is_pe : sa->is_pe, interleaved, (fl & kFlagNul) ? 1 : 0, n_pairs, c->d_icall);
  }
  NEED(index_call_end(c, nullptr, 0, 0, nullptr));
  // (the kernel counts pairs, and a pair can be both a header without '@' and a differing name: the header is tested
  // first, so it wins the tie; an interleaved file has two records a pair)
  index_finding(out, c->h_icall->first_wrong, c->h_icall->first_missing, interleaved ? FQG_E_UNPAIRED : FQG_E_NAME_MISMATCH, true,
                interleaved ? 2 : 1);
  return 0;
}
