// fqg_split_kernels.hip - fastq_split_interleaved on the GPU (reference src/fastq_split_interleaved.c:59-89): the
// records of an interleaved frame dealt into two streams, record first + 2k to stream 0 and first + 2k + 1 to stream 1,
// each written as fastq_write_entry writes it (src/fastq.c:265-272: the four lines as C strings).
//
// A de-interleave is a fixed permutation: where a record lies and where it goes follow from the line index alone - no
// list of records, no per-record length array on the way out.  Same tile scheme as the record filters
// (fqg_filter_kernels.hip):
//   k_split_lens        one thread per record: its output bytes, into the array of its stream
//   k_scan64_a/_b       the two 64-bit exclusive prefixes in one launch pair
//   k_split_tile_flags  one thread per tile of T records (T even: a tile holds whole pairs): does its span fit LDS
//   k_split_emit_tile   one wavefront per tile: the tile's span of the image lands in LDS with aligned 16-byte loads, every
//                       lane copies its record inside LDS into the image of its stream (the two images lie behind each
//                       other in ONE output area: together they hold exactly the span's bytes, however unequal the
//                       mates), both images leave with aligned 16-byte stores (emit_flush); tile_walk (fqg_fastq_tile.h)
//   k_split_emit_direct tiles that do not fit (long reads) and images with NUL bytes (lines are C strings there,
//                       bc_clip_nul): one wavefront per record, image to image
#include "fqg_device.h"
#include "fqg_fastq_tile.h"

namespace fqg {

struct SplitArgs {
  FrameView fv;
  uint64_t first, n_rec;        // records [first, first + n_rec) of the frame, n_rec even
  uint32_t T, in_cap, out_cap;  // records per tile (even, <= 64); LDS bytes of the staged span and of the two images
  int32_t has_nul;
  uint32_t* len[2];             // per stream: bytes of its p-th record (record first + 2p + stream)
  unsigned long long* local[2]; // ... their exclusive prefix inside a span of kScan64Span
  unsigned long long* sums[2];  // ... and the prefix of the span sums
  uint8_t* out[2];
  uint8_t* tile_big;
  unsigned long long* n_big;    // tiles that take the direct path
};

__global__ __launch_bounds__(kBlock) void k_split_lens(SplitArgs A) {
  for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < A.n_rec; k += (uint64_t)gridDim.x * kBlock) {
    const uint64_t r = A.first + k;
    uint32_t len;
    if (A.has_nul) {
      BcLine ln[4];
      frame_lines(A.fv, r, true, ln);
      len = ln[0].len + ln[0].nl + ln[1].len + ln[1].nl + ln[2].len + ln[2].nl + ln[3].len + ln[3].nl;
    } else {
      const uint64_t b = r == 0 ? 0 : A.fv.line_end[4 * r - 1] + 1;
      const uint64_t e = A.fv.line_end[4 * r + 3];
      len = (uint32_t)(e - b) + (e < A.fv.nbytes ? 1u : 0u);
    }
    A.len[k & 1][k >> 1] = len;
  }
}

// bytes the two images of a tile need on top of the span's own (two skews below 16, the second image on a 16-byte
// boundary behind the first)
constexpr uint32_t kSplitOutSlack = 64;

__global__ __launch_bounds__(kBlock) void k_split_tile_flags(SplitArgs A) {
  const uint64_t n_tiles = (A.n_rec + A.T - 1) / A.T;
  const uint64_t tile = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool big = false;
  if (tile < n_tiles) {
    const uint64_t k0 = tile * A.T, k1 = (k0 + A.T < A.n_rec ? k0 + A.T : A.n_rec) - 1;
    uint64_t n;
    const bool fit = frame_span_fits(A.fv, A.first + k0, A.first + k1, A.in_cap, n) && n + kSplitOutSlack <= (uint64_t)A.out_cap;
    big = A.has_nul || !fit;
    A.tile_big[tile] = big ? 1 : 0;
  }
  const unsigned long long m = __ballot(big);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(A.n_big, (unsigned long long)__builtin_popcountll(m));
}

// what a lane knows of its record: two words of the line index, its place in its stream
struct SplitGeo {
  uint64_t praw, e3;  // end of the line in front of the record (record 0 of the frame: unused), end of its last line
  unsigned long long off, sum;  // its place in its stream is off + sum (added where it is used: see TileGeo)
  uint32_t r0;
  uint8_t big;
  __device__ __forceinline__ uint64_t start() const { return r0 ? 0ull : praw + 1; }
};
__global__ __launch_bounds__(kWave, 2) void k_split_emit_tile(SplitArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_lds[];
  uint8_t* s_in = s_lds;
  uint8_t* s_out = s_lds + A.in_cap;
  const int lane = (int)threadIdx.x;
  auto geo_of = [&](const TileAt& at, SplitGeo& g) {  // (Tn: even, >= 2)
    const uint64_t k = at.tile * A.T + ((uint32_t)lane < at.Tn ? (uint32_t)lane : at.Tn - 1);
    const uint64_t r = A.first + k;
    const uint64_t* __restrict__ le = A.fv.line_end + 4 * r;
    g.r0 = r == 0 ? 1u : 0u;
    g.praw = le[r == 0 ? 0 : -1];
    g.e3 = le[3];
    g.off = A.local[k & 1][k >> 1];
    g.sum = A.sums[k & 1][(k >> 1) / kScan64Span];
    g.big = A.tile_big[at.tile];
  };
  auto span = [&](const SplitGeo& g, const TileAt& at) { return span_of(A.fv, g.start(), g.e3, (int)at.Tn - 1); };
  auto fetch = [&](const SplitGeo& g, const TileAt& at, bc_u32x4(&pf)[kSpanPf]) { span_fetch(span(g, at), lane, pf); };
  auto stage = [&](const SplitGeo& cur, const TileAt& at, bool big, const bc_u32x4(&pf)[kSpanPf], BcLine& rec) {  // rec: the lane's record in LDS
    const Span sp = span(cur, at);
    if (!big) span_land(sp, lane, pf, s_in);  // (fits: k_split_tile_flags checked)
    const uint64_t b = cur.start();
    rec.len = (uint32_t)((cur.e3 < A.fv.nbytes ? cur.e3 + 1 : cur.e3) - b);
    rec.p = s_in + sp.skew + (uint32_t)(b - sp.s0);
  };
  auto work = [&](const SplitGeo& cur, const TileAt& at, const BcLine& rec) {
    const uint32_t Tn = at.Tn, len = rec.len;
    // the images of the two streams: lanes 0, 2, .. write the first, lanes 1, 3, .. the second
    const unsigned long long where = cur.off + cur.sum;
    const unsigned long long at0 = rl64(where, 0), at1 = rl64(where, 1);
    const uint32_t total0 = (uint32_t)(rl64(where + len, (int)Tn - 2) - at0);
    const uint32_t total1 = (uint32_t)(rl64(where + len, (int)Tn - 1) - at1);
    uint8_t* dst0 = A.out[0] + at0;
    uint8_t* dst1 = A.out[1] + at1;
    const uint32_t skew0 = (uint32_t)((uintptr_t)dst0 & 15u), skew1 = (uint32_t)((uintptr_t)dst1 & 15u);
    const uint32_t base1 = (skew0 + total0 + 15u) & ~15u;
    if ((uint32_t)lane < Tn) {
      const bool second = (lane & 1) != 0;
      LaneWriter w{s_out + (second ? base1 + skew1 : skew0) + (uint32_t)(where - (second ? at1 : at0))};
      w.bytes(rec.p, len);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    emit_flush(s_out, skew0, total0, dst0, lane);
    emit_flush(s_out + base1, skew1, total1, dst1, lane);
    __builtin_amdgcn_wave_barrier();
  };
  tile_walk<SplitGeo, BcLine>(A.n_rec, A.T, geo_of, fetch, stage, work);
}

// records of the tiles that do not fit LDS, and every record of an image with NUL bytes: one wavefront per record,
// straight from image to image
__device__ __forceinline__ void split_copy_wave(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t n, int lane) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(1)));
  for (uint32_t o = (uint32_t)lane * 16u; o < n; o += 16u * kWave) {
    if (o + 16u <= n) *reinterpret_cast<u32x4*>(dst + o) = *reinterpret_cast<const u32x4*>(src + o);
    else
      for (uint32_t q = o; q < n; ++q) dst[q] = src[q];
  }
}
__global__ __launch_bounds__(kBlock) void k_split_emit_direct(SplitArgs A) {
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kWave);
  const int lane = (int)(threadIdx.x & 63), wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (uint64_t k = (uint64_t)blockIdx.x * (kBlock / kWave) + wv; k < A.n_rec; k += n_waves) {
    if (!A.tile_big[k / A.T]) continue;
    const uint64_t r = A.first + k, p = k >> 1;
    uint8_t* dst = A.out[k & 1] + A.local[k & 1][p] + A.sums[k & 1][p / kScan64Span];
    if (A.has_nul) {  // what gzputs writes of a line is the C string: four pieces
      BcLine ln[4];
      frame_lines(A.fv, r, true, ln);
      const uint32_t m0 = ln[0].len + ln[0].nl, m1 = ln[1].len + ln[1].nl, m2 = ln[2].len + ln[2].nl, m3 = ln[3].len + ln[3].nl;
      split_copy_wave(ln[0].p, dst, m0, lane);
      split_copy_wave(ln[1].p, dst + m0, m1, lane);
      split_copy_wave(ln[2].p, dst + m0 + m1, m2, lane);
      split_copy_wave(ln[3].p, dst + m0 + m1 + m2, m3, lane);
    } else {
      const uint64_t b = r == 0 ? 0 : A.fv.line_end[4 * r - 1] + 1;
      const uint64_t e = A.fv.line_end[4 * r + 3];
      split_copy_wave(A.fv.img + b, dst, (uint32_t)(e - b) + (e < A.fv.nbytes ? 1u : 0u), lane);
    }
  }
}

}  // namespace fqg
