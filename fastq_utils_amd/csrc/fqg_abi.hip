// fqg_abi.hip - the C-ABI of libfqgpu.so (include/fqg.h): contexts, workspaces, launches.
// Single translation unit: the kernels are included so that launch sites see them directly.
#include <hip/hip_runtime.h>

#include <cstring>  // (before rocPRIM, whose texture iterator calls memset unqualified)
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>
#include <optional>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fqg_device.h"
#include "fqg_kernels.hip"
#include "fqg_stream_kernels.hip"
#include "fqg_index_kernels.hip"
#include "fqg_names_build_kernels.hip"
#include "fqg_barcode_kernels.hip"
#include "fqg_census_kernels.hip"
#include "fqg_census_umi_kernels.hip"
#include "fqg_filter_kernels.hip"
#include "fqg_split_kernels.hip"
#include "fqg_umi_kernels.hip"
#include "fqg_umi_rl_kernels.hip"
#include "fqg_umi_cell_kernels.hip"
#include "fqg_bamtags_kernels.hip"
#include "fqg_bam2fastq_kernels.hip"
#include "fqg_deflate_kernels.hip"
#include "fqg_inflate_kernels.hip"
#include "fqg_bam_index_kernels.hip"
#include "fqg_names_build_plan.h"

using namespace fqg;

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
namespace {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

// The text a call produced, on the device until an `_output` call copies it (fqg_text_out.inc): up to FQG_B2F_STREAMS
// streams behind each other in one block.
struct OutText {
  DevBuf buf;
  uint64_t at[FQG_B2F_STREAMS] = {}, bytes[FQG_B2F_STREAMS] = {};  // per stream: where it starts, what was produced
  hipStream_t copy_stream = nullptr;  // text_copy_begin: device-to-host copies beside the next piece's upload
  hipEvent_t ready = nullptr;         // ... recorded on the context's stream where the output was produced
  bool pending = false;
};

struct ProfEvent {
  int slot;
  hipEvent_t a, b;
};

struct ProfSlot {
  std::string name;
  uint64_t launches = 0;
  double ms = 0;
};

// Ablation switches (FQGPU_LINES_ABL, FQGPU_NAMES_ABL, FQGPU_BC_ABL, FQGPU_UMI_INSERT_ABL: kernels that skip a part
// of their work and give knowingly WRONG results, for tools/*_abl.sh) exist only in a library built with
// -DFQG_MEASURE (`make MEASURE=1`).  The shipped library does not read these variables at all: a drop-in program
// that inherits one of them must not change what it computes.
// (the "every record met once" self-checks are never bypassed in the shipped library)
inline bool measured_wrong(int ablate) {
#ifdef FQG_MEASURE
  return ablate != 0;
#else
  (void)ablate;
  return false;
#endif
}
// a tuning knob that changes HOW a result is computed, never the result (A/B runs)
inline int env_int_early(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline int measure_int(const char* name) {
#ifdef FQG_MEASURE
  const char* e = getenv(name);
  const int v = e ? atoi(e) : 0;
  if (v) fprintf(stderr, "libfqgpu (FQG_MEASURE build): %s=%d - results of this call are NOT valid\n", name, v);
  return v;
#else
  (void)name;
  return 0;
#endif
}

}  // namespace

struct fqg_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  int cu_count = 256;
  int lines_per_cu = 0;  // workgroups of k_stream_lines a CU holds (asked once)
  int lines_fast_per_cu = 0;  // ... of k_stream_lines_fast
  uint64_t stream_min = 1ull << 20;  // images at least this large take the single-pass framing path (FQGPU_STREAM_MIN)

  DevBuf image;       // staging for host images
  DevBuf tile_counts; // u32 per tile
  DevBuf tile_local;  // u32 per tile
  DevBuf span_sums;   // u64 per span
  DevBuf line_end;    // u64 per line (+1)
  DevBuf records;     // fqg_record staging for fqg_frame_records
  DevBuf suspect;     // 1 bit per record: the fast path could not vouch for it
  DevBuf list;        // u64 record indices queued for the exact validator
  DevBuf stage;       // streaming path: u16 staged newline entries, kStageCap per chunk
  DevBuf cinfo;       // streaming path: u32 info word per chunk
  DevBuf queue;       // streaming path: u64 suspect byte positions
  DevBuf redo;        // streaming path: u32 chunks whose checks are repeated with the true rank
  DevBuf lines_slow;  // streaming path: one byte per step that k_stream_lines_fast leaves to the general kernel
  // The line index on demand (LinesArgs::no_index): the streaming path's line kernels have checked the records but
  // stored only the index's tail; `args` are the arguments of the run that stores it all (index_now).
  struct LazyIndex {
    bool pending = false;
    bool fast = false;  // k_stream_lines_fast + the steps it marked, or the general kernel alone
    unsigned grid = 0, grid_f = 0;
    LinesArgs args;
  } lazy;
  // the streaming pass in parts (k_stream_pass1_lines): the line workers' statistics until the image has passed
  AccState* pipe_acc = nullptr;
  unsigned long long* pipe_hist = nullptr;
  bool pipe_dirty = false;  // a parted pass left without its merge (an error in between): cleared by the next one
  uint64_t bc_status_valid = 0;  // iterations of the last fqg_barcodes_transform whose status bytes stand (fqg_barcodes_census)
  DevBuf build_keys[2], build_cursor, build_spill;  // the name table built in LDS (fqg_names_build_kernels.hip)
  DevBuf name_recs;   // streaming path with FQG_VALIDATE_NAMES: 64-byte header records, K per chunk (NameCapture)
  DevBuf name_hcount; // ... and the headers every chunk saw
  DevBuf name_redo, name_redo_chunks;  // what the capture-fed name kernel leaves to the line-index one
  NamesView names{};            // what the name kernels need of the last capture
  uint64_t last_names_captured = 0;    // of the last index call: records whose name came straight from a capture record
  const uint8_t* names_img = nullptr;  // the image it belongs to (null: no capture) - the current frame's, or the
  uint64_t names_nbytes = 0;           // capture is not used
  DevBuf umi_names, umi_cells, umi_umis, umi_entries[2];  // results of the last fqg_umi_count
  uint64_t umi_n_umis = 0;
  uint64_t umi_n_features = 0, umi_n_cells = 0, umi_n_entries[2] = {0, 0};
  void* umi_state = nullptr;  // UmiState of a deferred fqg_umi_count (fqg_umi_abi.inc)
  DevBuf umi_arena;           // scratch memory of fqg_umi_count, kept between calls
  size_t umi_arena_wanted = 0;
  CallState* d_cs = nullptr;
  CallState* h_cs = nullptr;  // pinned
  uint64_t* h_scalar = nullptr;  // pinned, 8 x u64

  FrameView frame{};
  bool frame_valid = false;
  bool frame_img_owned = false;  // the frame's image lives in `image` (host input), not with the caller
  bool frame_borrowed = false;   // the current frame is a retained frame made current again (fqg_frame_make_current)
  uint32_t frame_flags = 0;      // kFlagNul / kFlagCr of the framed image
  DevBuf bc_status, bc_len[3], bc_off[3], bc_sum[3], bc_tile_big;
  DevBuf wl_cells;  // fqg_barcodes_whitelist_correct: one 8-byte value per record
  BcCall* d_bcall = nullptr;
  BcCall* h_bcall = nullptr;  // pinned
  // the text of the last transform (streams 0..2), filter or gather (1), split (1, 2); of the last fqg_bam_add_tags;
  // of the last fqg_bam2fastq - three stores: the text of a BAM call survives a FASTQ-side call and the other way round
  OutText bc_text, bt_text, b2f_text;
  bool bt_begun = false;  // fqg_bam_add_tags has been called: FQG_TEXT_BAM_TAGS names a store
  uint64_t split_info[4] = {0, 0, 0, 0};  // of the last fqg_records_split: tiles, tiles on the direct path, emit grid, T
  uint64_t filter_info[6] = {0, 0, 0, 0, 0, 0};  // of the last fqg_records_filter: the same four, then in_cap and out_cap
  DevBuf bam_in, bam_off, bam_size, bam_local, bam_sums;  // scratch of one fqg_bam_add_tags / fqg_bam2fastq call
  DevBuf bt_tables, bt_call;  // fqg_bam_add_tags
  DevBuf b2f_call;            // fqg_bam2fastq
  // fqg_deflate / fqg_text_deflate: the members (and the text behind them) of the last call in a store of their own, and
  // the call's scratch - uploaded source and carry, member slots, their sizes and the sizes' scan, the token arena, tables
  OutText gz_text;
  DevBuf gz_in, gz_carry, gz_slots, gz_sizes, gz_off, gz_sums, gz_toks, gz_tab;
  bool gz_tab_ready = false;
  // fqg_bgzf_inflate: the inflated stream of the last call in a buffer no other call moves (the BAM calls read it where it
  // lies), and the call's scratch - the file, one row per block, their status words, the two first-block cells
  DevBuf inf_out, inf_raw, inf_rows, inf_status, inf_first;
  uint64_t inf_bytes = 0;
  bool inf_valid = false;
  // fqg_bam_index_device: the offsets of the last call in a buffer no other call moves, and the call's scratch - the two
  // tables of one window, its stretches, the follower's state
  DevBuf bx_offsets, bx_entries, bx_counts, bx_stretch, bx_state;
  uint64_t bx_n = 0;
  bool bx_valid = false;
  const unsigned long long* bam_offs = nullptr;  // the offsets of the running fqg_bam_add_tags / fqg_bam2fastq call
  IndexCall* d_icall = nullptr;
  IndexCall* h_icall = nullptr;  // pinned

  bool profiling = false;
  std::vector<ProfSlot> slots;
  std::vector<ProfEvent> pending;
  std::vector<hipEvent_t> free_events;
};

struct fqg_acc {
  fqg_ctx* ctx = nullptr;
  AccState* d_state = nullptr;
  unsigned long long* d_hist = nullptr;  // FQG_MAX_READ_LENGTH bins
  std::vector<unsigned long long> h_hist;
};

namespace {

int fail(fqg_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
  if (c) {
    c->err = what;
    if (e != hipSuccess) {
      c->err += ": ";
      c->err += hipGetErrorString(e);
    }
  }
  return code;
}

#define HIP_TRY(c, call)                                              \
  do {                                                                \
    hipError_t e__ = (call);                                          \
    if (e__ != hipSuccess) return fail((c), FQG_ERR_HIP, #call, e__); \
  } while (0)

#define NEED(rc_)        \
  do {                   \
    int r__ = (rc_);     \
    if (r__) return r__; \
  } while (0)

int ensure(fqg_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return 0;
  if (b.p) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, FQG_ERR_HIP, "hipStreamSynchronize", e);
    (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
  }
  size_t want = bytes + bytes / 8 + 256;
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) {
    want = bytes;
    e = hipMalloc(&b.p, want);
  }
  if (e != hipSuccess) return fail(c, FQG_ERR_NOMEM, "hipMalloc", e);
  b.cap = want;
  return 0;
}

void release(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

int prof_slot(fqg_ctx* c, const char* name) {
  for (size_t i = 0; i < c->slots.size(); ++i)
    if (c->slots[i].name == name) return (int)i;
  ProfSlot s;
  s.name = name;
  c->slots.push_back(s);
  return (int)c->slots.size() - 1;
}

hipEvent_t get_event(fqg_ctx* c) {
  if (!c->free_events.empty()) {
    hipEvent_t e = c->free_events.back();
    c->free_events.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

// fold finished event pairs into the per-kernel totals (call after the stream is idle)
void prof_drain(fqg_ctx* c) {
  for (auto& p : c->pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      c->slots[p.slot].launches++;
      c->slots[p.slot].ms += ms;
    }
    c->free_events.push_back(p.a);
    c->free_events.push_back(p.b);
  }
  c->pending.clear();
}

struct ProfScope {
  fqg_ctx* c;
  ProfEvent ev{};
  bool on;
  ProfScope(fqg_ctx* ctx, const char* name) : c(ctx), on(ctx->profiling) {
    if (!on) return;
    ev.slot = prof_slot(c, name);
    ev.a = get_event(c);
    ev.b = get_event(c);
    (void)hipEventRecord(ev.a, c->stream);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(ev.b, c->stream);
    c->pending.push_back(ev);
  }
};

void umi_drop_state(fqg_ctx* c);  // fqg_umi_abi.inc

#include "fqg_text_out.inc"

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the FUNCTION ON A DEVICE, not to a context: two contexts of one
// device (FQGPU_DEVICES=0,0,0) share it.  The largest size asked for so far is kept per (device, kernel) for the whole
// process and only ever raised - a context that needs less never lowers what another one is about to launch with - and
// the attribute is set when (and only when) the mark moves, not per call.
int raise_dynamic_lds(fqg_ctx* c, const void* kernel, size_t bytes) {
  static std::mutex mu;
  static std::vector<std::pair<std::pair<int, const void*>, size_t>> marks;
  std::lock_guard<std::mutex> lock(mu);
  size_t* mark = nullptr;
  for (auto& m : marks)
    if (m.first.first == c->device && m.first.second == kernel) mark = &m.second;
  if (!mark) {
    marks.push_back({{c->device, kernel}, 0});
    mark = &marks.back().second;
  }
  if (bytes <= *mark) return 0;
  HIP_TRY(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  *mark = bytes;
  return 0;
}

int grid_for_waves(fqg_ctx* c, uint64_t n_records) {
  // persistent wave-per-record kernels: enough workgroups to fill every CU 8 deep
  uint64_t want = (n_records + (kBlock / kWave) - 1) / (kBlock / kWave);
  uint64_t cap = (uint64_t)c->cu_count * 8;
  return (int)std::max<uint64_t>(1, std::min(want, cap));
}

// ---- what fqg_bam_add_tags and fqg_bam2fastq (`name`) share --------------------------------------
// The input side: the argument checks, then `begin()` (the call's own checks; its result and its last output
// cleared), the offsets, and the stream on the device at a 16-byte boundary (the tiles are staged with 16-byte
// loads) with its offsets in c->bam_off (c->bam_offs: where they are).  *d_buf: the stream there; nothing is copied for
// a call without records.  FQG_MEM_DEVICE_INDEXED: the offsets are device memory and are read where they lie - the host
// cannot look at them, so that they ascend inside the stream is the caller's word (fqg_bam_index_device keeps it); the
// first one comes back (*first_offset: eight bytes) for the mean record size, as a piece of a stream that is handed over
// with its front has nbytes far above what its records take.
template <class Begin>
int bam_input(fqg_ctx* c, const char* name, bool have_args, const void* stream, uint64_t nbytes, int mem, const uint64_t* offsets,
              uint64_t n_records, Begin begin, const uint8_t** d_buf, uint64_t* first_offset) {
  if (!c || !have_args || (n_records && (!stream || !offsets))) return FQG_ERR_ARG;
  if (mem != FQG_MEM_HOST && mem != FQG_MEM_DEVICE && mem != FQG_MEM_DEVICE_INDEXED) return FQG_ERR_ARG;
  if (n_records >= 0x7FFFFFFFull) return fail(c, FQG_ERR_ARG, (std::string(name) + ": more than 2^31 alignments in one call").c_str());
  NEED(begin());
  HIP_TRY(c, hipSetDevice(c->device));
  *d_buf = nullptr;
  if (!n_records) return 0;
  const uint32_t n = (uint32_t)n_records;
  if (mem != FQG_MEM_DEVICE_INDEXED)
    for (uint32_t k = 0; k < n; ++k)  // (a tile is the span from its first record to the end of its last)
      if (offsets[k] + 36 > nbytes || (k && offsets[k] <= offsets[k - 1]))
        return fail(c, FQG_ERR_ARG, (std::string(name) + ": offsets must ascend and lie inside the stream (fqg_bam_index_records)").c_str());
  if (mem == FQG_MEM_HOST || ((uintptr_t)stream & 15u)) {
    NEED(ensure(c, c->bam_in, nbytes + 64));
    HIP_TRY(c, hipMemcpyAsync(c->bam_in.p, stream, nbytes, mem == FQG_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    *d_buf = (const uint8_t*)c->bam_in.p;
  } else *d_buf = (const uint8_t*)stream;
  if (mem == FQG_MEM_DEVICE_INDEXED) {
    c->bam_offs = reinterpret_cast<const unsigned long long*>(offsets);  // (the caller's, in HBM)
    HIP_TRY(c, hipMemcpyAsync(&c->h_scalar[5], offsets, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *first_offset = c->h_scalar[5];
    if (*first_offset + 36 > nbytes) return fail(c, FQG_ERR_ARG, (std::string(name) + ": the first offset lies outside the stream").c_str());
    return 0;
  }
  *first_offset = offsets[0];
  NEED(ensure(c, c->bam_off, (size_t)n * 8));
  HIP_TRY(c, hipMemcpyAsync(c->bam_off.p, offsets, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  c->bam_offs = (const unsigned long long*)c->bam_off.p;
  return 0;
}

// Records per tile and the two LDS areas: what the mean record needs (a tile that does not fit takes the slow path);
// small areas let more wavefronts share a CU.  out_per_rec: the output bytes a record is expected to make, with its
// margin (a guess: sizes are not known yet).  `env`: the variable that asks for smaller tiles (measurement).
//   fqg_bam_add_tags  out_cap = (uint32_t)(1.15 * (mean_in + 64 + (tx_tag ? 40 : 0)) * T) + 256, in 16s, at most 28 KiB
//   fqg_bam2fastq     out_cap = (uint32_t)(2.3 * mean_in * T) + 32 * streams + 256, in 16s, at most 36 KiB
void bam_tile_shape(BamTiles& A, uint32_t in_lds, uint32_t out_lds, double mean_in, double out_per_rec, uint32_t pad, const char* env) {
  A.T = (uint32_t)std::max(1.0, std::min(64.0, std::floor(((double)in_lds - 64.0) / (1.1 * mean_in + 1.0))));
  if (const char* e = getenv(env)) A.T = (uint32_t)std::max(1, std::min<int>((int)A.T, atoi(e)));
  A.in_cap = std::min<uint32_t>(in_lds, ((uint32_t)(1.15 * mean_in * A.T) + 256u + 15u) & ~15u);
  A.out_cap = std::min<uint32_t>(out_lds, ((uint32_t)(out_per_rec * A.T) + pad + 256u + 15u) & ~15u);
}

}  // namespace

extern "C" {

int fqg_abi_version(void) { return FQG_ABI_VERSION; }

// The runtime prepares its path for copies of more than a few KiB when the first one is submitted (13 ms,
// tools/kbench/firstcopy.hip), and threads that submit their first ones at the same moment - the contexts of
// FQGPU_DEVICES, a thread each, every one with the first piece of a file - can die inside that preparation or leave a
// copy that never completes: 27 of 2 600 runs of one fuzz-campaign case ended with SIGSEGV below hipMemcpyAsync and
// one hung in hipStreamSynchronize, none of 3 900 with such a copy made beforehand by ONE thread
// (tools/repro_campaign_case.py, profiles/r05t_first_copy_race.txt).  So when a process opens a SECOND context - the
// only way two threads can be copying at once: a context is one thread's at a time - the opening thread makes that
// first copy on every device that has a context, before it hands anything to other threads.  (A process with one
// context does not pay for it: most never copy that much.)  FQGPU_NO_FIRST_COPY=1 leaves it out, for that tool.
static void first_large_copy(int device) {
  static std::mutex mu;
  static std::vector<int> opened, copied;  // devices, each once
  static unsigned n_opens = 0;
  static const bool off = getenv("FQGPU_NO_FIRST_COPY") != nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (std::find(opened.begin(), opened.end(), device) == opened.end()) opened.push_back(device);
  if (off || ++n_opens < 2) return;
  constexpr size_t kBytes = 256u << 10;
  for (int dev : opened) {
    if (std::find(copied.begin(), copied.end(), dev) != copied.end()) continue;
    copied.push_back(dev);
    void *h = nullptr, *d = nullptr;
    hipStream_t st = nullptr;
    if (hipSetDevice(dev) == hipSuccess && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
        hipHostMalloc(&h, kBytes, hipHostMallocPortable) == hipSuccess && hipMalloc(&d, kBytes) == hipSuccess) {
      (void)hipMemcpyAsync(d, h, kBytes, hipMemcpyHostToDevice, st);
      (void)hipMemcpyAsync(h, d, kBytes, hipMemcpyDeviceToHost, st);
      (void)hipStreamSynchronize(st);
    }
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
    if (st) (void)hipStreamDestroy(st);
  }
  (void)hipSetDevice(device);
}

int fqg_open(int device_ordinal, fqg_ctx** out) {
  if (!out) return FQG_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FQG_ERR_NO_DEVICE;
  if (device_ordinal < 0 || device_ordinal >= n) return FQG_ERR_ARG;
  if (hipSetDevice(device_ordinal) != hipSuccess) return FQG_ERR_NO_DEVICE;
  fqg_ctx* c = new fqg_ctx();
  c->device = device_ordinal;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess) c->cu_count = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return FQG_ERR_HIP;
  }
  c->stream = c->own_stream;
  if (const char* e = getenv("FQGPU_STREAM_MIN")) c->stream_min = std::max<uint64_t>(256, strtoull(e, nullptr, 10));
  if (hipMalloc((void**)&c->d_bcall, sizeof(BcCall) + 64) != hipSuccess ||
      hipHostMalloc((void**)&c->h_bcall, sizeof(BcCall) + 64, hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void**)&c->d_icall, sizeof(IndexCall)) != hipSuccess ||
      hipHostMalloc((void**)&c->h_icall, sizeof(IndexCall), hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void**)&c->d_cs, sizeof(CallState)) != hipSuccess ||
      hipHostMalloc((void**)&c->h_cs, sizeof(CallState), hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&c->h_scalar, 8 * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) {
    fqg_close(c);
    return FQG_ERR_NOMEM;
  }
  first_large_copy(device_ordinal);
  *out = c;
  return 0;
}

void fqg_close(fqg_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  prof_drain(c);
  umi_drop_state(c);
  for (auto e : c->free_events) (void)hipEventDestroy(e);
  release(c->image);
  release(c->tile_counts);
  release(c->tile_local);
  release(c->span_sums);
  release(c->line_end);
  release(c->records);
  release(c->suspect);
  release(c->list);
  release(c->stage);
  release(c->cinfo);
  release(c->queue);
  release(c->redo);
  release(c->lines_slow);
  if (c->pipe_acc) (void)hipFree(c->pipe_acc);
  if (c->pipe_hist) (void)hipFree(c->pipe_hist);
  release(c->build_keys[0]);
  release(c->build_keys[1]);
  release(c->build_cursor);
  release(c->build_spill);
  release(c->name_recs);
  release(c->name_hcount);
  release(c->name_redo);
  release(c->name_redo_chunks);
  release(c->umi_arena);
  release(c->umi_names);
  release(c->umi_cells);
  release(c->umi_umis);
  release(c->umi_entries[0]);
  release(c->umi_entries[1]);
  release(c->bc_status);
  release(c->wl_cells);
  release(c->bc_tile_big);
  for (DevBuf* b : {&c->bam_in, &c->bam_off, &c->bam_size, &c->bam_local, &c->bam_sums, &c->bt_tables, &c->bt_call,
                    &c->b2f_call, &c->bc_text.buf, &c->bt_text.buf, &c->b2f_text.buf, &c->gz_text.buf, &c->gz_in, &c->gz_carry,
                    &c->gz_slots, &c->gz_sizes, &c->gz_off, &c->gz_sums, &c->gz_toks, &c->gz_tab, &c->inf_out, &c->inf_raw,
                    &c->inf_rows, &c->inf_status, &c->inf_first, &c->bx_offsets, &c->bx_entries, &c->bx_counts, &c->bx_stretch,
                    &c->bx_state})
    release(*b);
  for (int i = 0; i < 3; ++i) {
    release(c->bc_len[i]);
    release(c->bc_off[i]);
    release(c->bc_sum[i]);
  }
  if (c->d_bcall) (void)hipFree(c->d_bcall);
  if (c->h_bcall) (void)hipHostFree(c->h_bcall);
  if (c->d_icall) (void)hipFree(c->d_icall);
  if (c->h_icall) (void)hipHostFree(c->h_icall);
  if (c->d_cs) (void)hipFree(c->d_cs);
  if (c->h_cs) (void)hipHostFree(c->h_cs);
  if (c->h_scalar) (void)hipHostFree(c->h_scalar);
  for (OutText* o : {&c->bc_text, &c->gz_text}) {
    if (o->copy_stream) {
      (void)hipStreamSynchronize(o->copy_stream);
      (void)hipStreamDestroy(o->copy_stream);
    }
    if (o->ready) (void)hipEventDestroy(o->ready);
  }
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

const char* fqg_last_error(const fqg_ctx* c) { return c ? c->err.c_str() : "no context"; }

int fqg_set_stream(fqg_ctx* c, void* s) {
  if (!c) return FQG_ERR_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return 0;
}

int fqg_synchronize(fqg_ctx* c) {
  if (!c) return FQG_ERR_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

void* fqg_host_alloc(fqg_ctx* c, size_t bytes) {
  void* p = nullptr;
  if (!c || hipSetDevice(c->device) != hipSuccess) return nullptr;  // (callable from the programs' reader threads)
  // (portable: the pieces one reader thread fills are handed to whichever device's context is free, host/fq_multi.h)
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) return nullptr;
  return p;
}
void fqg_host_free(fqg_ctx* c, void* p) {
  (void)c;
  if (p) (void)hipHostFree(p);
}

// Everything the context keeps between calls only so that the next call does not allocate again - the framing buffers
// of the largest image seen, capture records, the tile kernels' plan and output text - given back to the device.
// The current frame goes with them (retained frames own their buffers and stay).
int fqg_release_scratch(fqg_ctx* c) {
  if (!c) return FQG_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  NEED(text_wait(c, c->bc_text));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (DevBuf* b : {&c->image, &c->tile_counts, &c->tile_local, &c->span_sums, &c->line_end, &c->records, &c->suspect, &c->list,
                    &c->stage, &c->cinfo, &c->queue, &c->redo, &c->lines_slow, &c->build_keys[0], &c->build_keys[1],
                    &c->build_cursor, &c->build_spill, &c->name_recs, &c->name_hcount, &c->name_redo, &c->name_redo_chunks,
                    &c->bc_status, &c->wl_cells, &c->bc_tile_big, &c->inf_out, &c->inf_raw, &c->inf_rows, &c->inf_status, &c->inf_first,
                    &c->bx_offsets, &c->bx_entries, &c->bx_counts, &c->bx_stretch, &c->bx_state})
    release(*b);
  c->inf_valid = false;  // (fqg_inflate_device: valid until here)
  c->inf_bytes = 0;
  c->bx_valid = false;  // (fqg_bam_index_offsets: valid until here)
  c->bx_n = 0;
  for (int i = 0; i < 3; ++i) {
    release(c->bc_len[i]);
    release(c->bc_off[i]);
    release(c->bc_sum[i]);
  }
  text_release(c->bc_text);  // (the BAM calls' text stays)
  c->frame_valid = false;
  c->frame_borrowed = false;
  c->lazy.pending = false;
  c->names_img = nullptr;
  c->bc_status_valid = 0;
  return 0;
}

// ---- accumulator --------------------------------------------------------------------------
int fqg_acc_reset(fqg_acc* a) {
  if (!a) return FQG_ERR_ARG;
  fqg_ctx* c = a->ctx;
  AccState init;
  init.num_rds = 0;
  init.min_rl = FQG_MAX_READ_LENGTH;
  init.max_rl = 0;
  init.min_qbyte = 255;
  init.max_qbyte = 0;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(a->d_state, &init, sizeof(init), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemset(a->d_hist, 0, sizeof(unsigned long long) * FQG_MAX_READ_LENGTH));
  return 0;
}

int fqg_acc_create(fqg_ctx* c, fqg_acc** out) {
  if (!c || !out) return FQG_ERR_ARG;
  fqg_acc* a = new fqg_acc();
  a->ctx = c;
  if (hipSetDevice(c->device) != hipSuccess ||
      hipMalloc((void**)&a->d_state, sizeof(AccState)) != hipSuccess ||
      hipMalloc((void**)&a->d_hist, sizeof(unsigned long long) * FQG_MAX_READ_LENGTH) != hipSuccess) {
    fqg_acc_destroy(a);
    return fail(c, FQG_ERR_NOMEM, "accumulator allocation");
  }
  int rc = fqg_acc_reset(a);
  if (rc) {
    fqg_acc_destroy(a);
    return rc;
  }
  *out = a;
  return 0;
}

void fqg_acc_destroy(fqg_acc* a) {
  if (!a) return;
  if (a->ctx) (void)hipSetDevice(a->ctx->device);
  if (a->d_state) (void)hipFree(a->d_state);
  if (a->d_hist) (void)hipFree(a->d_hist);
  delete a;
}

static int acc_fetch_state(fqg_acc* a, AccState* s) {
  fqg_ctx* c = a->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(s, a->d_state, sizeof(AccState), hipMemcpyDeviceToHost));
  return 0;
}

// the reference widens each quality char through (unsigned int): bytes >= 0x80 sign-extend
static uint64_t widen_qual(unsigned b) { return b < 128 ? b : (0xFFFFFF00ull | b); }

int fqg_acc_read(fqg_acc* a, fqg_file_stats* out) {
  if (!a || !out) return FQG_ERR_ARG;
  AccState s;
  int rc = acc_fetch_state(a, &s);
  if (rc) return rc;
  out->num_rds = s.num_rds;
  out->min_rl = s.min_rl;
  out->max_rl = s.max_rl;
  // FASTQ_FILE starts at min_qual=126, max_qual=0 (src/fastq.c:174-175)
  if (s.min_qbyte <= s.max_qbyte) {
    out->min_qual = std::min<uint64_t>(FQG_MAX_PHRED_QUAL, widen_qual(s.min_qbyte));
    out->max_qual = widen_qual(s.max_qbyte);
  } else {
    out->min_qual = FQG_MAX_PHRED_QUAL;
    out->max_qual = 0;
  }
  return 0;
}

static int acc_fetch_hist(fqg_acc* a) {
  fqg_ctx* c = a->ctx;
  a->h_hist.resize(FQG_MAX_READ_LENGTH);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(a->h_hist.data(), a->d_hist, sizeof(unsigned long long) * FQG_MAX_READ_LENGTH,
                       hipMemcpyDeviceToHost));
  return 0;
}

int fqg_acc_hist_nonzero(fqg_acc* a, uint64_t* lens, uint64_t* counts, size_t cap, size_t* n) {
  if (!a || !n) return FQG_ERR_ARG;
  int rc = acc_fetch_hist(a);
  if (rc) return rc;
  size_t k = 0;
  for (size_t i = 0; i < (size_t)FQG_MAX_READ_LENGTH; ++i)
    if (a->h_hist[i]) {
      if (k < cap && lens && counts) {
        lens[k] = i;
        counts[k] = a->h_hist[i];
      }
      ++k;
    }
  *n = k;
  return 0;
}

// median_rl(), reference src/fastq_info.c:39-55
int fqg_acc_median(fqg_acc* a, fqg_acc* b, uint64_t* median) {
  if (!a || !median) return FQG_ERR_ARG;
  AccState sa, sb;
  int rc = acc_fetch_state(a, &sa);
  if (rc) return rc;
  if (sa.num_rds == 1 && !b) {
    *median = sa.min_rl;
    return 0;
  }
  uint64_t nreads = sa.num_rds;
  if ((rc = acc_fetch_hist(a))) return rc;
  if (b) {
    if ((rc = acc_fetch_state(b, &sb))) return rc;
    if ((rc = acc_fetch_hist(b))) return rc;
    nreads += sb.num_rds;
  }
  unsigned long long ctr = 0;
  uint64_t crl = 1;
  while (crl < FQG_MAX_READ_LENGTH) {
    ctr += a->h_hist[crl];
    if (b) ctr += b->h_hist[crl];
    if (sa.num_rds > 1 && ctr > nreads / 2) break;
    ++crl;
  }
  *median = crl;
  return 0;
}

// export layout: AccState | u64 n | n x (u64 len, u64 count)
int fqg_acc_export(fqg_acc* a, void* buf, size_t cap, size_t* used) {
  if (!a || !used) return FQG_ERR_ARG;
  AccState s;
  int rc = acc_fetch_state(a, &s);
  if (rc) return rc;
  if ((rc = acc_fetch_hist(a))) return rc;
  std::vector<uint64_t> pairs;
  for (size_t i = 0; i < (size_t)FQG_MAX_READ_LENGTH; ++i)
    if (a->h_hist[i]) {
      pairs.push_back(i);
      pairs.push_back(a->h_hist[i]);
    }
  const size_t need = sizeof(AccState) + 8 + pairs.size() * 8;
  *used = need;
  if (!buf || cap < need) return buf ? FQG_ERR_ARG : 0;
  char* w = (char*)buf;
  memcpy(w, &s, sizeof(s));
  const uint64_t n = pairs.size() / 2;
  memcpy(w + sizeof(s), &n, 8);
  if (n) memcpy(w + sizeof(s) + 8, pairs.data(), pairs.size() * 8);
  return 0;
}

int fqg_acc_merge(fqg_acc* a, const void* buf, size_t used) {
  if (!a || !buf || used < sizeof(AccState) + 8) return FQG_ERR_ARG;
  fqg_ctx* c = a->ctx;
  AccState mine, other;
  int rc = acc_fetch_state(a, &mine);
  if (rc) return rc;
  const char* r = (const char*)buf;
  memcpy(&other, r, sizeof(other));
  uint64_t n;
  memcpy(&n, r + sizeof(other), 8);
  if (used < sizeof(AccState) + 8 + n * 16) return FQG_ERR_ARG;
  mine.num_rds += other.num_rds;
  mine.min_rl = std::min(mine.min_rl, other.min_rl);
  mine.max_rl = std::max(mine.max_rl, other.max_rl);
  mine.min_qbyte = std::min(mine.min_qbyte, other.min_qbyte);
  mine.max_qbyte = std::max(mine.max_qbyte, other.max_qbyte);
  HIP_TRY(c, hipMemcpy(a->d_state, &mine, sizeof(mine), hipMemcpyHostToDevice));
  if (n) {
    if ((rc = acc_fetch_hist(a))) return rc;
    const uint64_t* pr = (const uint64_t*)(r + sizeof(other) + 8);
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t len = pr[2 * i], cnt = pr[2 * i + 1];
      if (len >= (uint64_t)FQG_MAX_READ_LENGTH) return FQG_ERR_ARG;
      a->h_hist[len] += cnt;
      HIP_TRY(c, hipMemcpy(a->d_hist + len, &a->h_hist[len], 8, hipMemcpyHostToDevice));
    }
  }
  return 0;
}

// ---- framing + validation -------------------------------------------------------------------
namespace {

struct Framed {
  uint64_t n_newlines = 0;
  bool last_nl = false;
  uint32_t img_flags = 0;
  bool checks_done = false;  // the byte-class checks of the tiled path ran over the image
  bool records_done = false; // lengths, statistics and suspect bits of every record are done too (k_stream_lines)
};

void init_call_state(fqg_ctx* c) {
  CallState init;
  memset(&init, 0, sizeof(init));
  init.first_key = ~0ull;
  init.stop_record = ~0ull;
  init.trunc_record = ~0ull;
  init.qmin_byte = 255;
  init.boot_qmin = 255;
  *c->h_cs = init;
}

// "call state back to the host and wait" - `also`: eight more bytes (of the line index) in the same wait
int read_call_state(fqg_ctx* c, const uint64_t* also = nullptr, uint64_t* also_to = nullptr) {
  HIP_TRY(c, hipMemcpyAsync(c->h_cs, c->d_cs, sizeof(CallState), hipMemcpyDeviceToHost, c->stream));
  if (also) HIP_TRY(c, hipMemcpyAsync(also_to, also, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

// Two passes over the image: newline census per chunk, prefix over the counts, then the line
// index (with or without the byte-class checks).  Sizes every buffer exactly.
int frame_two_pass(fqg_ctx* c, const uint8_t* d_img, uint64_t nbytes, uint32_t n_chunks, bool final,
                   bool want_checks, SuspectMap sm, Framed* out) {
  int rc;
  const uint32_t n_spans = (n_chunks + kScanSpan - 1) / kScanSpan;
  if ((rc = ensure(c, c->tile_counts, (size_t)n_chunks * 4))) return rc;
  if ((rc = ensure(c, c->tile_local, (size_t)n_chunks * 4))) return rc;
  if ((rc = ensure(c, c->span_sums, (size_t)n_spans * 8))) return rc;
  init_call_state(c);
  HIP_TRY(c, hipMemcpyAsync(c->d_cs, c->h_cs, sizeof(CallState), hipMemcpyHostToDevice, c->stream));
  {
    ProfScope ps(c, "k_count_nl");
    hipLaunchKernelGGL(k_count_nl, dim3((n_chunks + 3) / 4), dim3(kBlock), 0, c->stream, d_img, nbytes, n_chunks,
                       (uint32_t*)c->tile_counts.p, c->d_cs);
  }
  {
    ProfScope ps(c, "k_scan");
    hipLaunchKernelGGL(k_scan_a, dim3(n_spans), dim3(kBlock), 0, c->stream, (const uint32_t*)c->tile_counts.p,
                       n_chunks, (uint32_t*)c->tile_local.p, (unsigned long long*)c->span_sums.p);
    hipLaunchKernelGGL(k_scan_b, dim3(1), dim3(kBlock), 0, c->stream, (unsigned long long*)c->span_sums.p,
                       n_spans, d_img, nbytes, c->d_cs);
  }
  if ((rc = read_call_state(c))) return rc;
  out->n_newlines = c->h_cs->n_newlines;
  out->last_nl = c->h_cs->last_byte_is_nl != 0;
  out->img_flags = c->h_cs->flags;
  const uint64_t n_lines_all = out->n_newlines + (out->last_nl ? 0 : 1);
  const uint64_t usable = (final || out->last_nl) ? n_lines_all : out->n_newlines;
  const uint64_t line_cap = n_lines_all + 17;
  if ((rc = ensure(c, c->line_end, (size_t)line_cap * 8))) return rc;
  const bool checks = want_checks && !(out->img_flags & (kFlagNul | kFlagCr));
  const unsigned grid = (unsigned)std::min<uint64_t>((n_chunks + 3) / 4, (uint64_t)c->cu_count * 8);
  ProfScope ps(c, checks ? "k_frame_fast" : "k_lines");
  // one argument list for both: with the checks (and the records they cover: `limit`) or the line index alone
  auto launch = [&](auto kernel, uint64_t limit) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, c->stream, d_img, nbytes, n_chunks,
                       (const uint32_t*)c->tile_local.p, (const unsigned long long*)c->span_sums.p,
                       (uint64_t*)c->line_end.p, line_cap, limit, sm, c->d_cs, (const uint32_t*)nullptr,
                       (const uint32_t*)nullptr);
  };
  if (checks) launch(k_frame_fast_t<0u>, 4 * (usable / 4));
  else launch(k_frame_fast_t<7u>, (uint64_t)0);
  out->checks_done = checks;
  return 0;
}

constexpr uint32_t kStreamBootBytes = kBootMax;   // prefix whose quality range seeds the range test (64 KiB: LDS of k_stream_boot)
constexpr uint64_t kStreamQueueCap = 1ull << 20;

struct RecordDuties {  // what k_stream_lines needs from the caller of frame_stream
  int space;
  uint32_t weight;
  AccState* acc;
  unsigned long long* hist;
  int fmt, is_pe;  // name digests are made under the caller's file state
};

// how a run of the line kernels treats the line index: its room, and whether only the tail from `keep_from` is
// stored (LinesArgs::no_index)
struct IndexMode {
  uint64_t* line_end;
  uint64_t line_cap;
  bool no_index;
  uint64_t keep_from;
};

// What the phases of one frame_stream call share: the image and what the caller wants, then what each phase settles
// for the ones behind it.  Lives for the call.
struct StreamCall {
  const uint8_t* img;
  uint64_t nbytes;
  uint32_t n_chunks, n_spans;
  bool final;
  SuspectMap sm;
  RecordDuties rd;
  int want_names;  // 0, 1 = records, 2 = digests
  bool want_index;
  StreamOut so{};
  NameCapture nc{};
  ChunkRanks cr{};
  // the plan of the parts
  uint32_t n_parts = 1;
  int last_pct = 16;
  uint64_t early_line_cap = 0;  // room of the line index sized from the boot window (the line workers store into it)
  uint64_t todo_steps_cap = 0;  // marks of the general line kernel made ready in front of the pass
  LinesArgs PA{};  // what the line workers inside the pass-1 launches go by (the rest comes from the call state)
  // known once the pass is through
  uint64_t n_newlines = 0, n_lines_all = 0, line_cap = 0, limit = 0;
  bool index_lost = false;

  // the boot window: what k_stream_boot reads, and what the estimates from its line count go by
  uint32_t boot_span() const { return (uint32_t)std::min<uint64_t>(kStreamBootBytes, nbytes & ~255ull); }
  // The LAST part is the small one: its line work has no pass-1 launch behind it to hide in - it is what runs alone
  // at the end of the call - while the line work of the parts before it runs inside the next part's launch at next to no
  // cost.  FQGPU_STREAM_LAST_PART_PCT (default 16: parts of 28 / 28 / 28 / 16 % of the image; 25: equal parts, as this was
  // first built).  The line workers are not quite free - what the tail loses the launches gain back in part: one box, two
  // runs each, ms per step: 25 % 7.89 / 7.96, 16 % 7.88 / 7.87, 12 % 7.96 / 7.90, 8 % 7.96 / 7.98, 5 % 8.19 / 8.20 (there
  // pass 1 of the last part no longer outlasts the line workers of the part before).
  // (The name modes, whose line workers store the line index as they go, like it too - the pass with digests, one box, two
  // runs each: 25 % 10.10 / 10.12 ms + 0.34 behind it, 16 % 10.01 / 10.06 + 0.26.  Boxes differ by more than that.)
  uint32_t part_begin(uint32_t part) const {  // in spans
    if (part == 0 || n_parts <= 1) return part == 0 ? 0u : n_spans;
    if (part >= n_parts) return n_spans;
    const uint32_t last = std::min<uint32_t>(n_spans - (n_parts - 1), std::max<uint32_t>(1u, (uint32_t)((uint64_t)n_spans * (uint32_t)last_pct / 100u)));
    return (uint32_t)((uint64_t)(n_spans - last) * part / (n_parts - 1));
  }
  // The arguments of the line kernels of this call.  What its variations differ in is named here or where they are
  // made: the chunk ranks, where the statistics go (null: none), and the index mode.  n_newlines / n_lines / limit /
  // ablate stay zero: the line workers inside the pass-1 launches take them from the call state; who launches behind
  // the pass sets them.
  LinesArgs lines_args(const fqg_ctx* c, const ChunkRanks& cr, AccState* acc, unsigned long long* hist, const IndexMode& ix) const {
    LinesArgs A{};
    A.img = img;
    A.n = nbytes;
    A.cr = cr;
    A.stage = (const uint16_t*)c->stage.p;
    A.line_end = ix.line_end;
    A.line_cap = ix.line_cap;
    A.suspect_bits = sm.bits;
    A.suspect_cap = sm.cap;
    A.flags = sm.flags;
    A.space = rd.space;
    A.weight = rd.weight;
    A.acc = acc;
    A.hist = hist;
    A.no_index = ix.no_index ? 1u : 0u;
    A.index_only = 0u;
    A.keep_from = ix.keep_from;
    return A;
  }
};

ChunkRanks chunk_ranks(const fqg_ctx* c, uint32_t n_chunks) {
  ChunkRanks cr;
  cr.counts = (const uint32_t*)c->tile_counts.p;
  cr.local = (const uint32_t*)c->tile_local.p;
  cr.span_excl = (const unsigned long long*)c->span_sums.p;
  cr.n_chunks = n_chunks;
  return cr;
}

// the statistics of the parted pass: folded into `dst` (null: nowhere - the pass is left without them, nothing reaches
// the caller's accumulator), and the scratch cleared
void fold_parted(fqg_ctx* c, AccState* dst, unsigned long long* dst_hist) {
  hipLaunchKernelGGL(k_acc_merge, dim3(64), dim3(kBlock), 0, c->stream, c->pipe_acc, c->pipe_hist, dst, dst_hist, dst ? 0 : 1);
  hipLaunchKernelGGL(k_acc_scratch_reset, dim3(1), dim3(1), 0, c->stream, c->pipe_acc);
  c->pipe_dirty = false;
}

// workgroups of `kernel` a CU holds, asked once
// (per context: a context is one device, and contexts run on threads of their own)
int resident_per_cu(int& asked, const void* kernel) {
  if (!asked) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, kBlock, 0) != hipSuccess || nb < 1) nb = 4;
    asked = nb;
  }
  return asked;
}

// phase 1: the buffers, the call state, the quality range of the boot window
int stream_begin(fqg_ctx* c, StreamCall& s) {
  int rc;
  if ((rc = ensure(c, c->tile_counts, (size_t)s.n_chunks * 4))) return rc;
  if ((rc = ensure(c, c->tile_local, (size_t)s.n_chunks * 4))) return rc;
  if ((rc = ensure(c, c->span_sums, (size_t)s.n_spans * 8))) return rc;
  if ((rc = ensure(c, c->cinfo, (size_t)s.n_chunks * 4))) return rc;
  if ((rc = ensure(c, c->redo, (size_t)s.n_chunks * 4))) return rc;
  if ((rc = ensure(c, c->stage, (size_t)s.n_chunks * kStageCap * 2))) return rc;
  if ((rc = ensure(c, c->queue, (size_t)kStreamQueueCap * 8))) return rc;
  init_call_state(c);
  HIP_TRY(c, hipMemcpyAsync(c->d_cs, c->h_cs, sizeof(CallState), hipMemcpyHostToDevice, c->stream));
  s.so.counts = (uint32_t*)c->tile_counts.p;
  s.so.cinfo = (uint32_t*)c->cinfo.p;
  s.so.stage = (uint16_t*)c->stage.p;
  s.so.queue = (unsigned long long*)c->queue.p;
  s.so.queue_cap = kStreamQueueCap;
  s.cr = chunk_ranks(c, s.n_chunks);
  ProfScope ps(c, "k_stream_boot");
  hipLaunchKernelGGL(k_stream_boot, dim3(1), dim3(kBootBlock), 0, c->stream, s.img, s.boot_span(), c->d_cs);
  return 0;
}

// phase 2 (name modes): record slots per chunk from the mean record of the boot window: a power of two with a quarter
// of headroom (a chunk that sees more headers is read through the line index instead)
int stream_name_setup(fqg_ctx* c, StreamCall& s) {
  int rc;
  if ((rc = read_call_state(c))) return rc;
  const double per_chunk = (double)(c->h_cs->boot_lines / 4 + 1) * (double)kChunkBytes / (double)std::max<uint32_t>(s.boot_span(), 1);
  uint32_t shift = 3;
  while (shift < 7 && (double)(1u << shift) < 1.25 * per_chunk + 1.0) ++shift;
  s.nc.K = 1u << shift;
  s.nc.fmt = s.rd.fmt;
  s.nc.is_pe = s.rd.is_pe;
  if ((rc = ensure(c, c->name_recs, ((size_t)s.n_chunks << shift) * (s.want_names == 2 ? kDigestWords : kNameRecWords) * 8))) return rc;
  if ((rc = ensure(c, c->name_hcount, (size_t)s.n_chunks * 2))) return rc;
  s.nc.recs = (unsigned long long*)c->name_recs.p;
  s.nc.hcount = (uint16_t*)c->name_hcount.p;
  c->names.k_shift = shift;
  return 0;
}

// phase 3: the plan of the parts.
// Large images that only want to be validated take the pass in PARTS: pass 1 of part p shares its launch with the line
// workers of part p - 1 (k_stream_pass1_lines), whose statistics wait in accumulators of the context until the whole
// image has passed without a flag that sends it to the two-pass path.  FQGPU_STREAM_PARTS=1: one launch, as before.
// (read per call: tests and A/B runs switch them inside one process)
int stream_plan_parts(fqg_ctx* c, StreamCall& s) {
  int rc;
  const int parts_env = env_int_early("FQGPU_STREAM_PARTS", 4);
  const uint32_t parts_min_spans = (uint32_t)std::max(env_int_early("FQGPU_STREAM_PARTS_MIN_SPANS", 24), 1);  // (16 MiB each)
  // (with the index wanted - the name modes - the line workers store it as they go, into room sized from the boot window)
  s.n_parts = ((s.want_names || !s.want_index) && s.rd.acc && s.n_spans >= parts_min_spans)
                  ? (uint32_t)std::min(std::max(parts_env, 1), 4) : 1u;
  s.n_parts = std::min(s.n_parts, s.n_spans);
  s.last_pct = std::min(std::max(env_int_early("FQGPU_STREAM_LAST_PART_PCT", 16), 1), 100);  // (see StreamCall::part_begin)
  if (s.n_parts <= 1) return 0;
  if (s.want_index) {
    // lines of the image from the lines of the boot window (the name modes have waited for it above), a quarter more
    const double per_byte = (double)(c->h_cs->boot_lines + 4) / (double)std::max<uint32_t>(s.boot_span(), 1);
    s.early_line_cap = (uint64_t)(per_byte * 1.25 * (double)s.nbytes) + 4096;
    if ((rc = ensure(c, c->line_end, (size_t)s.early_line_cap * 8))) return rc;
  }
  if (!c->pipe_hist) {
    if (!c->pipe_acc) HIP_TRY(c, hipMalloc((void**)&c->pipe_acc, sizeof(AccState)));
    HIP_TRY(c, hipMalloc((void**)&c->pipe_hist, sizeof(unsigned long long) * FQG_MAX_READ_LENGTH));
    HIP_TRY(c, hipMemsetAsync(c->pipe_hist, 0, sizeof(unsigned long long) * FQG_MAX_READ_LENGTH, c->stream));
    hipLaunchKernelGGL(k_acc_scratch_reset, dim3(1), dim3(1), 0, c->stream, c->pipe_acc);
    c->pipe_dirty = false;
  }
  if (c->pipe_dirty) fold_parted(c, nullptr, nullptr);  // (a parted pass left without its merge: an error in between)
  c->pipe_dirty = true;
  // one mark per step for the general line kernel: every line has a byte, 512 lines a step
  s.todo_steps_cap = s.nbytes / (uint64_t)(4 * kWave * kLinesPer) + 8;
  if ((rc = ensure(c, c->lines_slow, (size_t)s.todo_steps_cap + 4))) return rc;
  HIP_TRY(c, hipMemsetAsync(c->lines_slow.p, 0, (size_t)s.todo_steps_cap, c->stream));
  // the line workers: no chunk count (their launch has it), statistics to the scratch, the whole index or none of it
  s.PA = s.lines_args(c, chunk_ranks(c, 0), c->pipe_acc, c->pipe_hist,
                    s.want_index ? IndexMode{(uint64_t*)c->line_end.p, s.early_line_cap, false, ~0ull}
                                 : IndexMode{nullptr, ~0ull, true, ~0ull});
  return 0;
}

// phase 4: pass 1, part by part (from the second on with the line workers of the part before), and the prefix over
// each part's newline counts
void stream_pass1_parts(fqg_ctx* c, const StreamCall& s) {
  const unsigned workers = (unsigned)c->cu_count;  // one line-worker workgroup per CU
  for (uint32_t part = 0; part < s.n_parts; ++part) {
    const uint32_t span_lo = s.part_begin(part), span_hi = s.part_begin(part + 1);
    const uint32_t chunk_lo = span_lo * kScanSpan, chunk_hi = std::min<uint32_t>(s.n_chunks, span_hi * kScanSpan);
    const unsigned blocks = (chunk_hi - chunk_lo + 3) / 4;
    {
      ProfScope ps(c, s.want_names == 2 ? (part ? "k_stream_pass1_lines(digests)" : "k_stream_pass1(digests)")
                      : s.want_names    ? (part ? "k_stream_pass1_lines(names)" : "k_stream_pass1(names)")
                      : part            ? "k_stream_pass1_lines" : "k_stream_pass1");
#define FQG_PASS1_PART(N)                                                                                                    \
  do {                                                                                                                       \
    if (part == 0)                                                                                                           \
      hipLaunchKernelGGL((k_stream_pass1<0u, N>), dim3(blocks), dim3(kBlock), 0, c->stream, s.img, s.nbytes, chunk_hi, s.so,  \
                         c->d_cs, s.nc);                                                                                     \
    else                                                                                                                     \
      hipLaunchKernelGGL(k_stream_pass1_lines<N>, dim3(workers + blocks), dim3(kBlock), 0, c->stream, s.img, s.nbytes,       \
                         chunk_lo, chunk_hi, s.so, c->d_cs, s.PA, (uint8_t*)c->lines_slow.p, workers, part - 1, s.nc);       \
  } while (0)
      if (s.want_names == 2) FQG_PASS1_PART(2);
      else if (s.want_names) FQG_PASS1_PART(1);
      else FQG_PASS1_PART(0);
#undef FQG_PASS1_PART
    }
    ProfScope ps(c, "k_scan");
    // (two launches: ONE, with the workgroup that finishes last doing phase B, was tried - the release fence every
    // workgroup needs in front of its count writes the L2 back: 0.21 ms a step instead of 0.11)
    hipLaunchKernelGGL(k_scan_a, dim3(span_hi - span_lo), dim3(kBlock), 0, c->stream, (const uint32_t*)c->tile_counts.p,
                       s.n_chunks, (uint32_t*)c->tile_local.p, (unsigned long long*)c->span_sums.p, span_lo);
    hipLaunchKernelGGL(k_scan_b, dim3(1), dim3(kBlock), 0, c->stream, (unsigned long long*)c->span_sums.p,
                       span_hi, s.img, s.nbytes, c->d_cs, span_lo, part);
  }
}

// phase 6: the per-chunk duties, then the line kernels behind the parts, the merge of the parted statistics and the
// record of what an index on demand would run
int stream_lines(fqg_ctx* c, const StreamCall& s) {
  int rc;
  {
    ProfScope ps(c, "k_stream_chunks");
    hipLaunchKernelGGL(k_stream_chunks, dim3((s.n_chunks + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, s.cr,
                       (const uint32_t*)c->cinfo.p, s.limit, (uint32_t*)c->redo.p, c->d_cs);
  }
  // the index on demand: when the caller has not said it wants it, and nothing queued by pass 1 needs it (the
  // queue kernel finds its records through the index)
  const bool lazy = !s.want_index && c->h_cs->queue_count == 0;
  // the steps the line workers inside the pass-1 launches have done (the parted pass): the launches below begin behind
  // them, and every line kernel of such a call adds to the context's accumulators, merged at the end
  const bool parted = s.n_parts > 1;
  const uint64_t done_steps = parted ? c->h_cs->lines_done_steps : 0;
  static const int lines_abl = measure_int("FQGPU_LINES_ABL");
  LinesArgs A = s.lines_args(c, s.cr, parted ? c->pipe_acc : s.rd.acc, parted ? c->pipe_hist : s.rd.hist,
                           IndexMode{(uint64_t*)c->line_end.p, s.line_cap, lazy, s.limit >= 8 ? s.limit - 8 : 0});
  A.n_newlines = s.n_newlines;
  A.n_lines = s.n_lines_all;
  A.limit = s.limit;
  A.ablate = lines_abl;
  c->lazy.pending = false;
  {
    ProfScope ps(c, "k_stream_lines");
    const uint64_t groups = (s.n_lines_all + 4 * kWave - 1) / (4 * kWave);
    // a persistent grid: every workgroup must be resident from the start (one that is not would do its whole
    // share after the others have finished)
    const uint64_t per_gpu = (uint64_t)c->cu_count * resident_per_cu(c->lines_per_cu, reinterpret_cast<const void*>(k_stream_lines<false>));
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((groups + 3) / 4, per_gpu));
    // (more than 64 newlines in an average chunk - reads below 100 bases - or fewer than 32 - reads of kilobases: hardly a
    // step would qualify for the kernel without a search)
    const double nl_per_chunk = (double)s.n_newlines / (double)std::max<uint32_t>(s.n_chunks, 1);
    c->lazy.grid = grid;
    c->lazy.fast = false;
    if (done_steps == 0 && (nl_per_chunk > 60.0 || nl_per_chunk < 32.0)) {
      hipLaunchKernelGGL(k_stream_lines<false>, dim3(grid), dim3(kBlock), 0, c->stream, A, (const uint8_t*)nullptr);
    } else {
      // the steps of ordinary records in the kernel without a search, what it marks in the general one behind it
      const uint64_t n_steps = (groups + kLinesPer - 1) / kLinesPer;
      if (parted && n_steps + 4 > s.todo_steps_cap) return fail(c, FQG_ERR_STATE, "streaming pass: more steps than lines");
      if (!parted) {
        if ((rc = ensure(c, c->lines_slow, (size_t)n_steps + 4))) return rc;
        HIP_TRY(c, hipMemsetAsync(c->lines_slow.p, 0, (size_t)n_steps, c->stream));
      }
      // (at most seven workgroups per CU: its LDS lets eight be resident, and with eight the kernel is slower - 0.148 ms
      // against 0.129 ms for its launches of a step of 100 M reads, profiles/r18_ab_bench_waves.txt)
      constexpr int kLinesFastPerCuMax = 7;
      const uint64_t fast_per_gpu = (uint64_t)c->cu_count * std::min(kLinesFastPerCuMax, resident_per_cu(c->lines_fast_per_cu, reinterpret_cast<const void*>(k_stream_lines_fast)));
      auto grid_fast = [&](uint64_t steps) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((steps + 3) / 4, fast_per_gpu)); };
      if (done_steps && !lazy && (!s.early_line_cap || s.index_lost)) {
        // the index is wanted after all (pass 1 queued byte positions), or its room was too small: the stores of the
        // steps that are done
        LinesArgs I = A;
        I.index_only = 1u;
        I.acc = nullptr;
        I.hist = nullptr;
        I.step_lo = 0;
        I.step_hi = done_steps;
        hipLaunchKernelGGL(k_stream_lines_fast, dim3(grid_fast(done_steps)), dim3(kBlock), 0, c->stream, I, (uint8_t*)c->lines_slow.p);
      }
      LinesArgs F = A;  // the steps behind the ones that are done, to the last
      F.step_lo = done_steps;
      F.step_hi = 0;
      hipLaunchKernelGGL(k_stream_lines_fast, dim3(grid_fast(n_steps - std::min(done_steps, n_steps))), dim3(kBlock), 0, c->stream, F, (uint8_t*)c->lines_slow.p);
      hipLaunchKernelGGL(k_stream_lines<true>, dim3(grid), dim3(kBlock), 0, c->stream, A, (const uint8_t*)c->lines_slow.p);
      c->lazy.grid_f = grid_fast(n_steps);
      c->lazy.fast = true;
    }
  }
  if (parted) {
    ProfScope ps(c, "k_acc_merge");
    fold_parted(c, s.rd.acc, s.rd.hist);
  }
  if (lazy) {  // the same launches once more, stores only (index_now)
    c->lazy.pending = true;
    c->lazy.args = A;
    c->lazy.args.no_index = 0u;
    c->lazy.args.index_only = 1u;
    c->lazy.args.acc = nullptr;
    c->lazy.args.hist = nullptr;
  }
  return 0;
}

// phase 7: the suspect positions pass 1 queued, the chunks whose checks are repeated, the capture handed to the name kernels
void stream_finish(fqg_ctx* c, const StreamCall& s) {
  if (!c->lazy.pending) {  // (on demand only when pass 1 queued nothing: see stream_lines)
    ProfScope ps(c, "k_stream_queue");
    hipLaunchKernelGGL(k_stream_queue, dim3(64), dim3(kBlock), 0, c->stream, (const unsigned long long*)c->queue.p,
                       (unsigned long long)kStreamQueueCap, (const uint64_t*)c->line_end.p, s.n_lines_all, s.limit / 4, s.sm,
                       c->d_cs);
  }
  {
    // chunks whose speculated line type was wrong or missing: the two-pass kernel repeats the checks
    // with the true rank (no line-index stores)
    ProfScope ps(c, "k_stream_redo");
    // (ordinary reads send a handful of chunks here - the ones whose speculation failed -, reads of kilobases a quarter of
    // all: a grid that fills the GPU costs 0.06 ms to start and end for the former)
    const double nlpc = (double)s.n_newlines / (double)std::max<uint32_t>(s.n_chunks, 1);
    const unsigned grid = (unsigned)std::min<uint64_t>((s.n_chunks + 3) / 4, (uint64_t)c->cu_count * (nlpc >= 32.0 ? 1 : 8));
    hipLaunchKernelGGL(k_frame_fast_t<8u>, dim3(grid), dim3(kBlock), 0, c->stream, s.img, s.nbytes, s.n_chunks,
                       (const uint32_t*)c->tile_local.p, (const unsigned long long*)c->span_sums.p,
                       (uint64_t*)c->line_end.p, s.line_cap, s.limit, s.sm, c->d_cs, (const uint32_t*)c->redo.p,
                       (const uint32_t*)&c->d_cs->redo_count);
  }
  if (s.want_names) {
    c->names.recs = s.nc.recs;
    c->names.hcount = s.nc.hcount;
    c->names.cinfo = (const uint32_t*)c->cinfo.p;
    c->names.cr = s.cr;
    c->names.K = s.nc.K;
    c->names.digests = s.want_names == 2 ? 1u : 0u;
    c->names.fmt = s.rd.fmt;
    c->names.is_pe = s.rd.is_pe;
    c->names_img = s.img;
    c->names_nbytes = s.nbytes;
  }
}

// One pass over the image (see fqg_stream_kernels.hip), phase by phase in the order its launches go out.  Returns 1
// when the image is not eligible (NUL / CR bytes, bytes >= 0x80, more newlines per chunk than the staging area
// holds): the caller then runs frame_two_pass, which also decides about the exact path.
int frame_stream(fqg_ctx* c, const uint8_t* d_img, uint64_t nbytes, uint32_t n_chunks, bool final, SuspectMap sm,
                 const RecordDuties& rd, int want_names /* 0, 1 = records, 2 = digests */, bool want_index, Framed* out) {
  int rc;
  c->names_img = nullptr;
  StreamCall s{d_img, nbytes, n_chunks, (n_chunks + kScanSpan - 1) / kScanSpan, final, sm, rd, want_names, want_index};
  if ((rc = stream_begin(c, s))) return rc;
  if (want_names && (rc = stream_name_setup(c, s))) return rc;
  if ((rc = stream_plan_parts(c, s))) return rc;
  stream_pass1_parts(c, s);
  // phase 5: the flags of the whole image, its lines
  if ((rc = read_call_state(c))) return rc;
  if (c->h_cs->flags & (kFlagNul | kFlagCr | kFlagHigh | kFlagStageOverflow)) {
    if (s.n_parts > 1) fold_parted(c, nullptr, nullptr);  // (not eligible: the two-pass path makes the statistics)
    return 1;
  }
  out->n_newlines = s.n_newlines = c->h_cs->n_newlines;
  out->last_nl = c->h_cs->last_byte_is_nl != 0;
  out->img_flags = 0;
  s.n_lines_all = s.n_newlines + (out->last_nl ? 0 : 1);
  const uint64_t usable = (final || out->last_nl) ? s.n_lines_all : s.n_newlines;
  s.line_cap = s.n_lines_all + 17;
  s.limit = 4 * (usable / 4);
  // (the parted pass of a name mode: its line workers have stored index entries already - into room sized from the
  // boot window.  Too small after all: a new allocation, and their stores once more, in stream_lines)
  s.index_lost = s.early_line_cap && (size_t)s.line_cap * 8 > c->line_end.cap;
  if ((rc = ensure(c, c->line_end, (size_t)s.line_cap * 8))) return rc;
  if ((rc = stream_lines(c, s))) return rc;
  out->records_done = true;
  stream_finish(c, s);
  out->checks_done = true;
  return 0;
}

// The line index of the current frame, if the call that framed it left it for later (LinesArgs::no_index): the line
// kernels once more, stores only, on the context's stream - whatever is launched behind them there finds it written.
int index_now(fqg_ctx* c) {
  if (!c->lazy.pending) return 0;
  c->lazy.pending = false;
  HIP_TRY(c, hipSetDevice(c->device));
  ProfScope ps(c, "k_stream_lines_index");
  const LinesArgs& A = c->lazy.args;
  if (c->lazy.fast) {
    hipLaunchKernelGGL(k_stream_lines_fast, dim3(c->lazy.grid_f), dim3(kBlock), 0, c->stream, A, (uint8_t*)c->lines_slow.p);
    hipLaunchKernelGGL(k_stream_lines<true>, dim3(c->lazy.grid), dim3(kBlock), 0, c->stream, A, (const uint8_t*)c->lines_slow.p);
  } else {
    hipLaunchKernelGGL(k_stream_lines<false>, dim3(c->lazy.grid), dim3(kBlock), 0, c->stream, A, (const uint8_t*)nullptr);
  }
  HIP_TRY(c, hipGetLastError());
  return 0;
}

// What the steps of one fqg_validate call behind the framing share.
struct ValidateCall {
  FrameView fv;
  const fqg_file_state* st;
  fqg_acc* acc;  // null: no statistics
  uint32_t weight;
  SuspectMap sm;
  bool frame_only;
  uint64_t list_cap = 0;  // room of the list of records for the exact validator (the tiled paths)
  bool tail_is_stop = false, nul_truncated = false;  // what find_stop saw
};

// what varies between the launches of k_validate_exact
struct ExactRun {
  unsigned grid;
  bool listed;      // the records of the context's list (their number is read on the device), or every record
  bool stats;       // into the caller's accumulator, or none
  uint32_t weight;
  uint64_t record;  // kNoRecord, or the one record whose finding's arguments are wanted
};
void launch_exact(fqg_ctx* c, const ValidateCall& v, const ExactRun& r, const char* scope /* null: none */) {
  std::optional<ProfScope> ps;
  if (scope) ps.emplace(c, scope);
  const bool stats = r.stats && v.acc;
  hipLaunchKernelGGL(k_validate_exact, dim3(r.grid), dim3(kBlock), 0, c->stream, v.fv, v.st->is_pe, v.st->readname_format,
                     v.st->space, r.weight, stats ? v.acc->d_state : (AccState*)nullptr,
                     stats ? v.acc->d_hist : (unsigned long long*)nullptr, c->d_cs, r.record,
                     r.listed ? (const unsigned long long*)c->list.p : (const unsigned long long*)nullptr,
                     r.listed ? (const unsigned long long*)&c->d_cs->list_count : (const unsigned long long*)nullptr);
}

// the gzgets limits, where the record-wise checks do not look: every line of an image that is only framed, and the
// lines of an incomplete last record (the reference reads THOSE in pieces too before it finds the file truncated)
void check_overlong(fqg_ctx* c, const FrameView& fv, uint64_t from, uint64_t upto) {
  if (upto <= from) return;
  ProfScope ps(c, "k_overlong");
  FrameView lv = fv;
  lv.n_lines = upto;
  hipLaunchKernelGGL(k_overlong, dim3((unsigned)((upto - from + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, lv, from,
                     c->d_cs);
}

// a record that starts with NUL ends the file silently (src/fastq.c:250): the records in front of it stand, and
// v.fv.n_records says how many.  `tail`: lines of an incomplete last record that nothing more can follow
int find_stop(fqg_ctx* c, ValidateCall& v, bool tail, fqg_validate_result* out) {
  int rc;
  uint64_t n_records = v.fv.n_records;
  if (n_records) {
    ProfScope ps(c, "k_find_stop");
    hipLaunchKernelGGL(k_find_stop, dim3((unsigned)((n_records + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       c->stream, v.fv, c->d_cs, v.frame_only ? 1 : 0);
  }
  if (tail) {
    // first byte of the incomplete trailing group
    c->h_scalar[0] = ~0ull;
    if ((rc = read_call_state(c, n_records ? v.fv.line_end + 4 * n_records - 1 : nullptr, &c->h_scalar[0]))) return rc;
    const uint64_t at = c->h_scalar[0] + 1;
    uint8_t b = 1;
    HIP_TRY(c, hipMemcpy(&b, v.fv.img + at, 1, hipMemcpyDeviceToHost));
    v.tail_is_stop = (b == 0);
  } else if ((rc = read_call_state(c))) return rc;
  if (c->h_cs->stop_record < n_records) {
    n_records = c->h_cs->stop_record;
    out->stopped = 1;
  }
  if (c->h_cs->trunc_record < n_records) {  // (frame-only: an earlier record with an empty line - the file is truncated THERE)
    n_records = c->h_cs->trunc_record;
    out->stopped = 0;
    v.nul_truncated = true;
  }
  v.fv.n_records = n_records;
  return 0;
}

// The tiled paths: the records the line kernels (or k_records_fast, behind the two-pass framing) could not vouch for
// are listed, and the exact validator reads the list - unless the line index is still to be written: then once the
// number of listed records is known, in fqg_validate
int check_records(fqg_ctx* c, ValidateCall& v, bool records_done) {
  int rc;
  const uint64_t n_records = v.fv.n_records;
  v.list_cap = std::max<uint64_t>(1u << 20, n_records / 16);
  if (v.list_cap > n_records) v.list_cap = n_records;
  if ((rc = ensure(c, c->list, (size_t)v.list_cap * 8))) return rc;
  const unsigned grid_r =
      (unsigned)std::min<uint64_t>((n_records + kBlock - 1) / kBlock, (uint64_t)c->cu_count * 8);
  if (records_done) {
    ProfScope ps(c, "k_suspect_list");
    hipLaunchKernelGGL(k_suspect_list, dim3((unsigned)std::min<uint64_t>((n_records / 32 + kBlock) / kBlock, 1024)), dim3(kBlock), 0,
                       c->stream, (const uint32_t*)v.sm.bits, std::min<uint64_t>(n_records, v.sm.cap),
                       (unsigned long long*)c->list.p, v.list_cap, &c->d_cs->list_count, v.acc ? v.acc->d_state : nullptr,
                       (const CallState*)c->d_cs);
  } else {
    ProfScope ps(c, "k_records_fast");
    hipLaunchKernelGGL(k_records_fast, dim3(grid_r), dim3(kBlock), 0, c->stream, v.fv, v.st->space, v.weight, v.sm,
                       (unsigned long long*)c->list.p, v.list_cap, &c->d_cs->list_count,
                       v.acc ? v.acc->d_state : nullptr, v.acc ? v.acc->d_hist : nullptr, c->d_cs);
  }
  if (!c->lazy.pending) launch_exact(c, v, {(unsigned)c->cu_count * 2, true, false, v.weight, kNoRecord}, "k_validate_exact");
  return 0;
}

// The call state, read back, into the caller's result: the first finding with its arguments, or the truncated file.
// `leftover`: lines of an incomplete last record that nothing more can follow
int report_result(fqg_ctx* c, const ValidateCall& v, uint64_t leftover, fqg_validate_result* out) {
  int rc;
  const bool truncated = v.nul_truncated || (leftover && !out->stopped && !v.tail_is_stop);
  out->tail_lines = v.nul_truncated ? 1 : truncated ? (int32_t)leftover : 0;
  if (c->h_cs->first_key != ~0ull) {
    out->record = c->h_cs->first_key >> 8;
    out->code = (int32_t)(c->h_cs->first_key & 0xFF);
    if (out->code != FQG_E_LINE_TOO_LONG) {  // (that one has no arguments, and its record may be the incomplete last one)
      if ((rc = index_now(c))) return rc;
      launch_exact(c, v, {1u, false, false, 1u, out->record}, nullptr);
      if ((rc = read_call_state(c))) return rc;
      out->aux0 = c->h_cs->aux0;
      out->aux1 = c->h_cs->aux1;
    }
  } else if (truncated) {
    // src/fastq.c:254-257: fewer than four lines left (or, in an image that is only framed, a record with a line that
    // starts with NUL - an empty string to the reference: n_records counts the records in front of it)
    out->code = FQG_E_TRUNCATED;
    out->record = v.fv.n_records;
  } else if (v.tail_is_stop && !out->stopped) {
    out->stopped = 1;
  }
  return 0;
}

}  // namespace

int fqg_validate(fqg_ctx* c, fqg_acc* acc, const void* image, uint64_t nbytes, int mem, int final,
                 const fqg_file_state* st, uint32_t flags, fqg_validate_result* out) {
  if (!c || !out || !st || (nbytes && !image)) return FQG_ERR_ARG;
  if (!(flags & (FQG_VALIDATE_NO_STATS | FQG_VALIDATE_FRAME_ONLY)) && !acc)
    return fail(c, FQG_ERR_ARG, "fqg_validate: acc is NULL");
  if (mem != FQG_MEM_HOST && mem != FQG_MEM_DEVICE) return FQG_ERR_ARG;
  if (flags & FQG_VALIDATE_NO_STATS) acc = nullptr;
  memset(out, 0, sizeof(*out));
  c->frame_valid = false;
  c->frame_borrowed = false;
  c->lazy.pending = false;
  c->names_img = nullptr;
  HIP_TRY(c, hipSetDevice(c->device));
  if (nbytes == 0) return 0;
  if (nbytes >= (1ull << 44)) return fail(c, FQG_ERR_ARG, "image too large");

  // ---- the image on the device
  int rc;
  const uint8_t* d_img;
  if (mem == FQG_MEM_HOST) {
    if ((rc = ensure(c, c->image, nbytes + 64))) return rc;
    ProfScope ps(c, "h2d_image");
    HIP_TRY(c, hipMemcpyAsync(c->image.p, image, nbytes, hipMemcpyHostToDevice, c->stream));
    d_img = (const uint8_t*)c->image.p;
  } else {
    if (((uintptr_t)image & 15u) != 0) return fail(c, FQG_ERR_ARG, "device image must be 16-byte aligned");
    d_img = (const uint8_t*)image;
  }
  const uint32_t n_chunks = (uint32_t)((nbytes + kChunkBytes - 1) / kChunkBytes);
  const bool frame_only = (flags & FQG_VALIDATE_FRAME_ONLY) != 0;
  if (frame_only) acc = nullptr;
  const uint32_t name_flags = flags & (FQG_VALIDATE_NAMES | FQG_VALIDATE_NAME_DIGESTS);
  const bool may_stream = nbytes >= c->stream_min && !(flags & FQG_VALIDATE_TWO_PASS);
  // (frame only + names: the single-pass framing runs for its capture records; what its checks find is not looked at)
  const bool names_only = frame_only && name_flags && may_stream;
  const bool want_checks = !(flags & FQG_VALIDATE_FORCE_EXACT) && (!frame_only || names_only);
  const uint32_t weight = (flags & FQG_VALIDATE_COUNT_TWICE) ? 2u : 1u;

  // ---- suspect bitmap, sized from the image (>= 16 bytes per record assumed; denser images overflow
  // it, which sends every record to the exact validator)
  SuspectMap sm;
  sm.cap = std::max<uint64_t>(nbytes / 16, 1024);
  sm.flags = &c->d_cs->flags;
  sm.bits = nullptr;
  const size_t suspect_bytes = (size_t)(sm.cap / 32 + 2) * 4;
  if (want_checks) {
    if ((rc = ensure(c, c->suspect, suspect_bytes))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->suspect.p, 0, suspect_bytes, c->stream));
    sm.bits = (uint32_t*)c->suspect.p;
  }

  // ---- framing: one pass where the image allows it, else two
  Framed fr;
  bool streamed = false;
  if (want_checks && may_stream) {
    RecordDuties rd{st->space, weight, acc ? acc->d_state : nullptr, acc ? acc->d_hist : nullptr, st->readname_format, st->is_pe};
    // (digests need a format to canonicalise under: a file state that has none yet gets records)
    const int names_mode = (flags & FQG_VALIDATE_NAME_DIGESTS) && st->readname_format != FQG_NAME_UNDEF ? 2 : name_flags ? 1 : 0;
    rc = frame_stream(c, d_img, nbytes, n_chunks, final != 0, sm, rd, names_mode, name_flags || (flags & FQG_VALIDATE_INDEX), &fr);
    if (rc < 0) return rc;
    streamed = rc == 0;
    if (!streamed) HIP_TRY(c, hipMemsetAsync(c->suspect.p, 0, suspect_bytes, c->stream));
  }
  if (!streamed && (rc = frame_two_pass(c, d_img, nbytes, n_chunks, final != 0, want_checks && !frame_only, sm, &fr))) return rc;
  const uint64_t n_lines_all = fr.n_newlines + (fr.last_nl ? 0 : 1);
  // an unterminated last line is only a line when nothing more can follow
  const uint64_t usable = (final || fr.last_nl) ? n_lines_all : fr.n_newlines;
  const uint64_t leftover = usable % 4;
  ValidateCall v{FrameView{}, st, acc, weight, sm, frame_only};
  FrameView& fv = v.fv;
  fv.img = d_img;
  fv.nbytes = nbytes;
  fv.line_end = (const uint64_t*)c->line_end.p;
  fv.n_lines = n_lines_all;
  fv.n_records = usable / 4;
  fv.reframed = (flags & FQG_VALIDATE_REFRAMED) ? 1u : 0u;
  if (!fv.reframed) check_overlong(c, fv, frame_only ? 0 : 4 * fv.n_records, final ? n_lines_all : usable);
  if ((fr.img_flags & kFlagNul) && (rc = find_stop(c, v, leftover && final, out))) return rc;
  const uint64_t n_records = fv.n_records;  // (in front of a record that starts with NUL)

  // ---- the records.  The tiled path needs an image without NUL / CR bytes (then every line is terminated by its
  // '\n' alone and the statistics follow from the line index); anything else goes through the
  // exact wave-per-record validator as a whole.
  const bool fast = fr.checks_done && !frame_only;
  if (fast) {
    out->path = streamed ? 3 : 2;
    if (n_records && (rc = check_records(c, v, fr.records_done))) return rc;
  } else if (n_records && !frame_only) {
    launch_exact(c, v, {(unsigned)grid_for_waves(c, n_records), false, true, weight, kNoRecord}, "k_validate_exact");
    out->path = 1;
  }
  // ---- what was found, and where the last complete record ends
  if ((rc = read_call_state(c, n_records ? fv.line_end + 4 * n_records - 1 : nullptr, &c->h_scalar[1]))) return rc;
  auto overflow = [&] { return c->h_cs->list_count > v.list_cap || (c->h_cs->flags & (kFlagSuspectOverflow | kFlagQueueOverflow)); };
  if (c->lazy.pending && fast && n_records && c->h_cs->list_count > 0 && !overflow()) {
    // records the line kernels could not vouch for: the exact validator reads them through the index
    if ((rc = index_now(c))) return rc;
    launch_exact(c, v, {(unsigned)c->cu_count * 2, true, false, weight, kNoRecord}, "k_validate_exact");
    if ((rc = read_call_state(c))) return rc;
  }
  out->n_records = n_records;
  out->n_lines = n_lines_all;
  out->consumed = n_records ? c->h_scalar[1] + 1 : 0;
  if (out->consumed > nbytes) out->consumed = nbytes;  // unterminated last line
  if (fast && n_records && overflow()) {
    // more suspects than the queue / bitmap holds (e.g. every record carries its name on line 3):
    // let the exact validator look at every record; the statistics of the tiled pass stand
    if ((rc = index_now(c))) return rc;
    launch_exact(c, v, {(unsigned)grid_for_waves(c, n_records), false, false, weight, kNoRecord}, "k_validate_exact");
    if ((rc = read_call_state(c))) return rc;
  }
  if ((rc = report_result(c, v, final ? leftover : 0, out))) return rc;
  c->frame = fv;
  c->frame_valid = true;
  c->frame_img_owned = (mem == FQG_MEM_HOST);
  c->frame_flags = fr.img_flags;
  HIP_TRY(c, hipGetLastError());
  return 0;
}

int fqg_frame_records(fqg_ctx* c, uint64_t first, uint64_t count, fqg_record* out, int mem) {
  if (!c || (!out && count)) return FQG_ERR_ARG;
  if (!c->frame_valid) return fail(c, FQG_ERR_STATE, "no frame: call fqg_validate first");
  if (const int irc = index_now(c)) return irc;
  if (first + count > c->frame.n_records) return fail(c, FQG_ERR_ARG, "record range outside the frame");
  if (!count) return 0;
  int rc;
  fqg_record* d_out = out;
  if (mem == FQG_MEM_HOST) {
    if ((rc = ensure(c, c->records, count * sizeof(fqg_record)))) return rc;
    d_out = (fqg_record*)c->records.p;
  }
  {
    ProfScope ps(c, "k_records");
    hipLaunchKernelGGL(k_records, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                       c->frame, first, count, d_out);
  }
  if (mem == FQG_MEM_HOST) {
    HIP_TRY(c, hipMemcpyAsync(out, d_out, count * sizeof(fqg_record), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ---- frames ---------------------------------------------------------------------------------
struct fqg_frame {
  fqg_ctx* ctx = nullptr;
  FrameView fv{};
  DevBuf image;     // owned copy of a host image (empty for caller-owned device images)
  DevBuf line_end;  // owned line index
  uint32_t flags = 0;
};

int fqg_frame_make_current(fqg_ctx* c, const fqg_frame* f) {
  if (!c || !f || f->ctx != c) return FQG_ERR_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->frame = f->fv;
  c->lazy.pending = false;  // (a retained frame has its index: fqg_frame_retain)
  c->frame_flags = f->flags;
  c->frame_valid = true;
  c->frame_img_owned = false;
  c->frame_borrowed = true;
  return 0;
}

int fqg_frame_retain(fqg_ctx* c, fqg_frame** out) {
  if (!c || !out) return FQG_ERR_ARG;
  if (!c->frame_valid) return fail(c, FQG_ERR_STATE, "no frame: call fqg_validate first");
  if (const int irc = index_now(c)) return irc;
  if (c->frame_borrowed) return fail(c, FQG_ERR_STATE, "the current frame is a retained one: it cannot be retained again");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  fqg_frame* f = new fqg_frame();
  f->ctx = c;
  f->fv = c->frame;
  f->flags = c->frame_flags;
  f->line_end = c->line_end;  // the context allocates fresh buffers on its next call
  c->line_end = DevBuf();
  if (c->frame_img_owned) {
    f->image = c->image;
    c->image = DevBuf();
  }
  c->frame_valid = false;
  *out = f;
  return 0;
}

void fqg_frame_release(fqg_frame* f) {
  if (!f) return;
  (void)hipStreamSynchronize(f->ctx->stream);
  release(f->image);
  release(f->line_end);
  delete f;
}

uint64_t fqg_frame_n_records(const fqg_frame* f) { return f ? f->fv.n_records : 0; }

#include "fqg_barcode_abi.inc"  // (in front of the filters and the split: bc_tile_one and the output calls are theirs too)
#include "fqg_filter_abi.inc"

// ---- measurement ----------------------------------------------------------------------------
int fqg_profile_enable(fqg_ctx* c, int on) {
  if (!c) return FQG_ERR_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  c->profiling = on != 0;
  return 0;
}
int fqg_profile_reset(fqg_ctx* c) {
  if (!c) return FQG_ERR_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  for (auto& s : c->slots) {
    s.launches = 0;
    s.ms = 0;
  }
  return 0;
}
int fqg_profile_read(fqg_ctx* c, fqg_kernel_time* out, size_t cap, size_t* n) {
  if (!c || !n) return FQG_ERR_ARG;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  size_t k = 0;
  for (auto& s : c->slots) {
    if (k < cap && out) {
      memset(&out[k], 0, sizeof(out[k]));
      strncpy(out[k].name, s.name.c_str(), sizeof(out[k].name) - 1);
      out[k].launches = s.launches;
      out[k].total_ms = s.ms;
    }
    ++k;
  }
  *n = k;
  return 0;
}

// ---- synthetic data -------------------------------------------------------------------------
uint64_t fqg_synth_record_bytes(uint32_t read_len) { return (uint64_t)kSynthHdr + 2ull * (read_len + 1) + 2; }

int fqg_synth_fastq(fqg_ctx* c, void* device_out, uint64_t n_records, uint32_t read_len, uint64_t first_index,
                    uint64_t seed, int mate) {
  if (!c || !device_out || read_len == 0 || read_len >= FQG_MAX_READ_LENGTH - 2) return FQG_ERR_ARG;
  if (((uintptr_t)device_out & 15u) != 0) return fail(c, FQG_ERR_ARG, "output must be 16-byte aligned");
  if (first_index + n_records > 9999999999ull) return fail(c, FQG_ERR_ARG, "index does not fit 10 digits");
  if (!n_records) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t total = n_records * fqg_synth_record_bytes(read_len);
  const uint64_t threads = (total + 15) / 16;
  const uint64_t blocks = std::min<uint64_t>((threads + kBlock - 1) / kBlock, (uint64_t)c->cu_count * 32);
  ProfScope ps(c, "k_synth");
  hipLaunchKernelGGL(k_synth, dim3((unsigned)blocks), dim3(kBlock), 0, c->stream, (uint8_t*)device_out, n_records,
                     read_len, first_index, seed, mate == 2 ? 2 : 1);
  HIP_TRY(c, hipGetLastError());
  return 0;
}

#include "fqg_umi_abi.inc"
#include "fqg_index_abi.inc"
#include "fqg_fp_abi.inc"
#include "fqg_bamtags_abi.inc"
#include "fqg_bam2fastq_abi.inc"
#include "fqg_split_abi.inc"
#include "fqg_deflate_abi.inc"
#include "fqg_inflate_abi.inc"
#include "fqg_bam_index_abi.inc"

}  // extern "C"
