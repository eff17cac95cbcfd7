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
//                       mates), both images leave with aligned 16-byte stores (emit_flush); three tiles under way
//   k_split_emit_direct tiles that do not fit (long reads) and images with NUL bytes (lines are C strings there,
//                       bc_clip_nul): one wavefront per record, image to image
#include "fqg_device.h"
#include "fqg_tile.h"

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

// the four lines of record r as C strings (images with NUL bytes only)
__device__ __forceinline__ void split_lines_nul(const FrameView& f, uint64_t r, BcLine (&ln)[4]) {
  uint64_t prev = r == 0 ? ~0ull : f.line_end[4 * r - 1];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t e = f.line_end[4 * r + i];
    ln[i].p = f.img + prev + 1;
    ln[i].len = (uint32_t)(e - prev - 1);
    ln[i].nl = e < f.nbytes ? 1u : 0u;
    prev = e;
  }
  bc_clip_nul(ln[0]);
  bc_clip_nul(ln[1]);
  bc_clip_nul(ln[2]);
  bc_clip_nul(ln[3]);
}

__global__ __launch_bounds__(kBlock) void k_split_lens(SplitArgs A) {
  for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < A.n_rec; k += (uint64_t)gridDim.x * kBlock) {
    const uint64_t r = A.first + k;
    uint32_t len;
    if (A.has_nul) {
      BcLine ln[4];
      split_lines_nul(A.fv, r, ln);
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
    const uint64_t r0 = A.first + k0, r1 = A.first + k1;
    const uint64_t s0 = r0 == 0 ? 0 : A.fv.line_end[4 * r0 - 1] + 1, e3l = A.fv.line_end[4 * r1 + 3];
    const uint64_t n = (e3l < A.fv.nbytes ? e3l + 1 : e3l) - s0;
    const uint32_t skew = (uint32_t)((uintptr_t)(A.fv.img + s0) & 15u);
    bool fit = n <= (uint64_t)A.in_cap && n + kSplitOutSlack <= (uint64_t)A.out_cap;
    if (fit) fit = (uint64_t)((skew + (uint32_t)n + 15u) >> 4) * 16u + 32u <= (uint64_t)A.in_cap;
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
// the tile's span of the image in 16-byte units aligned on the image ADDRESS
struct SplitSpan {
  const uint8_t* gbase;
  uint64_t s0;
  uint32_t units, skew;
};
__device__ __forceinline__ void split_span(const SplitArgs& A, const SplitGeo& g, int last_lane, SplitSpan& sp) {
  sp.s0 = rfl64(g.start());
  const uint64_t e3l = rl64(g.e3, last_lane);
  const uint64_t n = (e3l < A.fv.nbytes ? e3l + 1 : e3l) - sp.s0;
  sp.skew = (uint32_t)((uintptr_t)(A.fv.img + sp.s0) & 15u);
  sp.gbase = A.fv.img + sp.s0 - sp.skew;
  const uint64_t units = ((uint64_t)sp.skew + n + 15u) >> 4;
  sp.units = units > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)units;  // (a tile that large is a big one: nothing lands)
}
__device__ __forceinline__ bc_u32x4 split_unit(const SplitSpan& sp, uint32_t u) {
  u = u < sp.units ? u : (sp.units ? sp.units - 1 : 0u);  // clamped: no branch, every load of a round in flight
  return __builtin_nontemporal_load(reinterpret_cast<const bc_u32x4*>(sp.gbase + 16ull * u));
}
__device__ __forceinline__ void split_fetch(const SplitSpan& sp, int lane, bc_u32x4 (&v)[kSpanPf]) {
#pragma unroll
  for (int j = 0; j < kSpanPf; ++j) v[j] = split_unit(sp, (uint32_t)(j * kWave + lane));
}
__device__ __forceinline__ void split_land(const SplitSpan& sp, int lane, const bc_u32x4 (&v)[kSpanPf], uint8_t* s_in) {
#pragma unroll
  for (int j = 0; j < kSpanPf; ++j) {
    const uint32_t u = (uint32_t)(j * kWave + lane);
    if (u < sp.units) *reinterpret_cast<bc_u32x4*>(s_in + 16u * u) = v[j];
  }
  for (uint32_t u0 = kSpanPf * kWave; u0 < sp.units; u0 += 8 * kWave) {  // (larger tiles: the rest now)
    bc_u32x4 q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = split_unit(sp, u0 + j * kWave + lane);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t u = u0 + j * kWave + lane;
      if (u < sp.units) *reinterpret_cast<bc_u32x4*>(s_in + 16u * u) = q[j];
    }
  }
}

__global__ __launch_bounds__(kWave, 2) void k_split_emit_tile(SplitArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_lds[];
  uint8_t* s_in = s_lds;
  uint8_t* s_out = s_lds + A.in_cap;
  const int lane = (int)threadIdx.x;
  const uint64_t n_tiles = (A.n_rec + A.T - 1) / A.T;
  auto tile_size = [&](uint64_t tile) {
    const uint64_t left = A.n_rec - tile * A.T;
    return (uint32_t)(left < (uint64_t)A.T ? left : (uint64_t)A.T);  // (even, >= 2)
  };
  auto geo_of = [&](uint64_t tile, SplitGeo& g) {
    const uint32_t Tn = tile_size(tile);
    const uint64_t k = tile * A.T + ((uint32_t)lane < Tn ? (uint32_t)lane : Tn - 1);
    const uint64_t r = A.first + k;
    const uint64_t* __restrict__ le = A.fv.line_end + 4 * r;
    g.r0 = r == 0 ? 1u : 0u;
    g.praw = le[r == 0 ? 0 : -1];
    g.e3 = le[3];
    g.off = A.local[k & 1][k >> 1];
    g.sum = A.sums[k & 1][(k >> 1) / kScan64Span];
    g.big = A.tile_big[tile];
  };
  // three tiles under way per wavefront, every request without a branch (see k_bc_emit_tile)
  const uint64_t stride = gridDim.x;
  auto clamp_tile = [&](uint64_t t) { return t < n_tiles ? t : n_tiles - 1; };
  SplitGeo cur, nxt, nx2;
  bc_u32x4 pf[kSpanPf];
  if (blockIdx.x < n_tiles) {
    geo_of(blockIdx.x, cur);
    geo_of(clamp_tile(blockIdx.x + stride), nxt);
    SplitSpan sp;
    split_span(A, cur, (int)tile_size(blockIdx.x) - 1, sp);
    split_fetch(sp, lane, pf);
  }
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += stride, cur = nxt, nxt = nx2) {
    const uint32_t Tn = tile_size(tile);
    const bool valid = (uint32_t)lane < Tn;
    const bool big = __builtin_amdgcn_readfirstlane((int)cur.big) != 0;
    const uint8_t* src;
    uint32_t len;
    {
      SplitSpan sp;
      split_span(A, cur, (int)Tn - 1, sp);
      if (!big) split_land(sp, lane, pf, s_in);  // (fits: k_split_tile_flags checked)
      const uint64_t b = cur.start();
      len = (uint32_t)((cur.e3 < A.fv.nbytes ? cur.e3 + 1 : cur.e3) - b);
      src = s_in + sp.skew + (uint32_t)(b - sp.s0);
    }
    {
      const uint64_t tn = clamp_tile(tile + stride);
      SplitSpan sp;
      split_span(A, nxt, (int)tile_size(tn) - 1, sp);
      split_fetch(sp, lane, pf);
    }
    geo_of(clamp_tile(tile + 2 * stride), nx2);
    if (big) continue;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the images of the two streams: lanes 0, 2, .. write the first, lanes 1, 3, .. the second
    const unsigned long long where = cur.off + cur.sum;
    const unsigned long long at0 = rl64(where, 0), at1 = rl64(where, 1);
    const uint32_t total0 = (uint32_t)(rl64(where + len, (int)Tn - 2) - at0);
    const uint32_t total1 = (uint32_t)(rl64(where + len, (int)Tn - 1) - at1);
    uint8_t* dst0 = A.out[0] + at0;
    uint8_t* dst1 = A.out[1] + at1;
    const uint32_t skew0 = (uint32_t)((uintptr_t)dst0 & 15u), skew1 = (uint32_t)((uintptr_t)dst1 & 15u);
    const uint32_t base1 = (skew0 + total0 + 15u) & ~15u;
    if (valid) {
      const bool second = (lane & 1) != 0;
      LaneWriter w{s_out + (second ? base1 + skew1 : skew0) + (uint32_t)(where - (second ? at1 : at0))};
      w.bytes(src, len);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    emit_flush(s_out, skew0, total0, dst0, lane);
    emit_flush(s_out + base1, skew1, total1, dst1, lane);
    __builtin_amdgcn_wave_barrier();
  }
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
      split_lines_nul(A.fv, r, ln);
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
