// fqg_fastq_tile.h - the tile frame of the kernels that walk a FASTQ frame (k_bc_emit_tile, k_rf_emit_tile,
// k_split_emit_tile): one wavefront per tile of T consecutive records (iterations), one lane per record.  A tile's
// records are ONE byte span of every image, cut into 16-byte units aligned on the image ADDRESS (a unit holds at least
// one byte of the image and never leaves its page); a span that fits lands in LDS, what the tile writes is built in an
// LDS image of its output span and leaves with 16-byte stores (emit_flush).  What a lane loads of its record, and the
// records, are the kernel's business.  The first part - does a span fit - is plain C++: the kernels that FLAG a tile and
// the kernels that LAND it count with one function, and a CPU test includes this header as they compile it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQG_TILE_HD __host__ __device__ __forceinline__
#else
#define FQG_TILE_HD inline __attribute__((always_inline))
#endif

namespace fqg {

// 16-byte units of n bytes whose first byte lies `skew` (0..15) bytes behind a 16-byte boundary
FQG_TILE_HD uint32_t span_units(uint32_t skew, uint32_t n) { return (skew + n + 15u) >> 4; }
// Does a span of n bytes at address skew `skew` fit an input area of in_cap bytes, behind the `units` units of the files
// in front of it (numbered through: one file starts at 0)?  A span longer than the area is refused before its units are
// added; 32 bytes stay free (the lane writers read behind a line): a yes means 16 * units <= in_cap - 32.
FQG_TILE_HD bool span_fits(uint32_t skew, uint64_t n, uint32_t in_cap, uint32_t& units) {
  bool fit = true;
  if (n > (uint64_t)in_cap) fit = false;
  else units += span_units(skew, (uint32_t)n);
  if ((uint64_t)units * 16u + 32u > (uint64_t)in_cap) fit = false;
  return fit;
}

}  // namespace fqg

#if defined(__HIPCC__) || defined(__CUDACC__)
#include "fqg_tile.h"

namespace fqg {

// ---- the lines of a record ---------------------------------------------------------------------------
struct BcLine {
  const uint8_t* p;
  uint32_t len;  // bytes before '\n'
  uint32_t nl;
};

// A line as the reference holds it: gzgets puts it into a buffer and everything after that is a C string function
// (strlen, gzputs, printf("%s"), strncpy, the scans) - the line ENDS at its first NUL byte, and a line that ends there
// has no '\n'.  This is also what a line cut at the gzgets limits is (host/fq_reframe.h: the piece is followed by
// "\0\n").  Only images that hold a NUL byte come here; the line is in global memory.
__device__ __forceinline__ void bc_clip_nul(BcLine& l) {
  const uint32_t n = l.len;
  uint32_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    __builtin_memcpy(&w, l.p + i, 8);
    const uint64_t z = (w - 0x0101010101010101ull) & ~w & 0x8080808080808080ull;  // 0x80 in the lowest zero byte (and maybe above it)
    if (z) {
      l.len = i + ((uint32_t)__builtin_ctzll(z) >> 3);
      l.nl = 0;
      return;
    }
  }
  for (; i < n; ++i)
    if (l.p[i] == 0) {
      l.len = i;
      l.nl = 0;
      return;
    }
}

// the four lines of record r where they lie in the image; nul: as C strings (an image that holds NUL bytes)
__device__ __forceinline__ void frame_lines(const FrameView& f, uint64_t r, bool nul, BcLine ln[4]) {
  uint64_t prev = r == 0 ? ~0ull : f.line_end[4 * r - 1];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint64_t e = f.line_end[4 * r + i];
    ln[i].p = f.img + prev + 1;
    ln[i].len = (uint32_t)(e - prev - 1);
    ln[i].nl = e < f.nbytes ? 1u : 0u;
    prev = e;
  }
  if (nul) {  // (four calls, not a loop over ln[i]: an index that is no constant puts the lines in scratch memory)
    bc_clip_nul(ln[0]);
    bc_clip_nul(ln[1]);
    bc_clip_nul(ln[2]);
    bc_clip_nul(ln[3]);
  }
}

// what a lane knows of its record from the line index
struct BcGeo {
  uint64_t praw, e[4];  // line ends of the lane's record, and of the line before it (record 0: its own first line end, unused)
  uint32_t r0;          // the lane's record is record 0 of its file
  __device__ __forceinline__ uint64_t start() const { return r0 ? 0ull : praw + 1; }  // first byte of the record
};

// ---- spans ---------------------------------------------------------------------------------------------
// The span of ONE file: image bytes [s0, ..) in `units` units, unit u at gbase + 16 u, the first byte `skew` bytes into
// unit 0.  (Several files numbered through: SpanPlan, fqg_barcode_kernels.hip; span_base says where its unit u lies.)
struct Span {
  const uint8_t* gbase;
  uint64_t s0;
  uint32_t units, skew;
};
// my_start, my_e3: the lane's record start and the end of its last line (the span: first lane's to last_lane's record)
__device__ __forceinline__ Span span_of(const FrameView& f, uint64_t my_start, uint64_t my_e3, int last_lane) {
  Span sp;
  sp.s0 = rfl64(my_start);
  const uint64_t e3l = rl64(my_e3, last_lane);
  const uint64_t n = (e3l < f.nbytes ? e3l + 1 : e3l) - sp.s0;
  sp.skew = (uint32_t)((uintptr_t)(f.img + sp.s0) & 15u);
  sp.gbase = f.img + sp.s0 - sp.skew;
  const uint64_t units = ((uint64_t)sp.skew + n + 15u) >> 4;
  sp.units = units > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)units;  // (a tile that large is a big one: nothing lands)
  return sp;
}
__device__ __forceinline__ const uint8_t* span_base(const Span& sp, uint32_t) { return sp.gbase; }
// one thread (the flag kernels): do records r0 .. r1 of a frame, a span of n bytes, fit an input area of in_cap bytes
__device__ __forceinline__ bool frame_span_fits(const FrameView& f, uint64_t r0, uint64_t r1, uint32_t in_cap, uint64_t& n) {
  const uint64_t s0 = r0 == 0 ? 0 : f.line_end[4 * r0 - 1] + 1, e3l = f.line_end[4 * r1 + 3];
  n = (e3l < f.nbytes ? e3l + 1 : e3l) - s0;
  uint32_t units = 0;
  return span_fits((uint32_t)((uintptr_t)(f.img + s0) & 15u), n, in_cap, units);
}

// unit u of a tile, clamped to its last unit: no branch, every load of a round in flight (no unit at all: unit 0, never stored)
template <class S>
__device__ __forceinline__ bc_u32x4 span_unit(const S& sp, uint32_t u) {
  u = u < sp.units ? u : (sp.units ? sp.units - 1 : 0u);
  return __builtin_nontemporal_load(reinterpret_cast<const bc_u32x4*>(span_base(sp, u) + 16ull * u));
}
// units from_unit .. of the tile -> s_in, 8 loads in flight per lane
template <class S>
__device__ __forceinline__ void span_copy(const S& sp, uint32_t from_unit, int lane, uint8_t* s_in) {
  for (uint32_t u0 = from_unit; u0 < sp.units; u0 += 8 * kWave) {
    bc_u32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = span_unit(sp, u0 + j * kWave + lane);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t u = u0 + j * kWave + lane;
      if (u < sp.units) *reinterpret_cast<bc_u32x4*>(s_in + 16u * u) = v[j];
    }
  }
}
// The walk requests the first kSpanPf * 64 units of a tile (10 KiB: every tile of the default LDS budget) as
// straight-line code - a loop makes the compiler wait for every request in flight where the loop begins, the next
// tile's index among them.
constexpr int kSpanPf = 10;
template <class S>
__device__ __forceinline__ void span_fetch(const S& sp, int lane, bc_u32x4 (&v)[kSpanPf]) {
#pragma unroll
  for (int j = 0; j < kSpanPf; ++j) v[j] = span_unit(sp, (uint32_t)(j * kWave + lane));
}
template <class S>
__device__ __forceinline__ void span_land(const S& sp, int lane, const bc_u32x4 (&v)[kSpanPf], uint8_t* s_in) {
#pragma unroll
  for (int j = 0; j < kSpanPf; ++j) {
    const uint32_t u = (uint32_t)(j * kWave + lane);
    if (u < sp.units) *reinterpret_cast<bc_u32x4*>(s_in + 16u * u) = v[j];
  }
  span_copy(sp, kSpanPf * kWave, lane, s_in);  // (larger tiles: the rest now)
}

// ---- the walk ------------------------------------------------------------------------------------------
// A wavefront's tiles: blockIdx.x, + gridDim.x, ...  Three tiles are under way per wavefront: the current tile is
// written while the spans of the next one (registers) and the line index of the one after it are in flight.  Every
// request is made without a branch and nothing is computed from a loaded value before the tile it belongs to begins - a
// value that is loaded on one path only is copied where the paths meet, and an instruction that reads it is a wait for
// it: the tile behind the last one is the last one again, a tile that does not fit LDS fetches (and drops) what its
// clamped span says.  Per tile, in this order:
//   stage(cur, at, big, pf, staged)  lands what was fetched for the tile (not if big); staged: what `work` needs of it
//   fetch(nxt, at, pf)               requests the next tile's spans
//   geo_of(at, nx2)                  requests the index of the tile after that (Geo: what a lane loads, and the flag `big`)
//   (a big tile ends here: the record-by-record kernel writes it)  the wavefront's fence and barrier
//   work(cur, at, staged)            every lane may read all of the landed spans
// (k_bc_emit_tile has this loop written out, fqg_barcode_kernels.hip: a change of the order is made in both places.)
struct TileAt {
  uint64_t tile;
  uint32_t Tn;  // its records: T, fewer in the last tile
};
template <class Geo, class Staged, class GeoOf, class Fetch, class Stage, class Work>
__device__ __forceinline__ void tile_walk(uint64_t n_items, uint32_t T, GeoOf geo_of, Fetch fetch, Stage stage, Work work) {
  const uint64_t n_tiles = (n_items + T - 1) / T;
  const uint64_t stride = gridDim.x;
  auto at = [&](uint64_t tile) {
    const uint64_t left = n_items - tile * T;
    return TileAt{tile, (uint32_t)(left < (uint64_t)T ? left : (uint64_t)T)};
  };
  auto clamped = [&](uint64_t t) { return at(t < n_tiles ? t : n_tiles - 1); };
  Geo cur, nxt, nx2;
  bc_u32x4 pf[kSpanPf];
  if (blockIdx.x < n_tiles) {
    geo_of(at(blockIdx.x), cur);
    geo_of(clamped(blockIdx.x + stride), nxt);
    fetch(cur, at(blockIdx.x), pf);
  }
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += stride, cur = nxt, nxt = nx2) {
    const TileAt here = at(tile);
    const bool big = __builtin_amdgcn_readfirstlane((int)cur.big) != 0;
    Staged staged;
    stage(cur, here, big, pf, staged);
    fetch(nxt, clamped(tile + stride), pf);
    geo_of(clamped(tile + 2 * stride), nx2);
    if (big) continue;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    work(cur, here, staged);
  }
}

// ---- the lane's place in a tile's output image -----------------------------------------------------------
// The lane's text goes to out + where and has my_len bytes (0: none - `where` ascends with the lanes, such a lane has the
// place of the next text), `before` more in front of it (the mate that shares an iteration's place).  The tile writes
// dst[0, total); in the LDS image the lane's text starts at skew + start (emit_flush).
struct TileImage {
  uint8_t* dst;
  uint32_t skew, start, total;
};
__device__ __forceinline__ TileImage tile_image(uint8_t* out, unsigned long long where, uint32_t my_len, uint32_t before = 0) {
  const unsigned long long tile_at = rfl64(where);
  const uint32_t start = (uint32_t)(where - tile_at) + before;
  uint8_t* const dst = out + tile_at;
  return TileImage{dst, (uint32_t)((uintptr_t)dst & 15u), start, wave_max32(start + my_len)};
}
// ... written by its lanes: out it goes
__device__ __forceinline__ void tile_image_flush(const TileImage im, const uint8_t* s_out, int lane, bool flush = true) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (flush) emit_flush(s_out, im.skew, im.total, im.dst, lane);
  __builtin_amdgcn_wave_barrier();
}

}  // namespace fqg
#endif
