// fqg_line_window.h - where the chunk window of a step of the line kernel without a search begins.
//
// A step of k_stream_lines_fast (fqg_stream_kernels.hip) covers the ranks [512 s - 1, 512 s + 512) and loads the chunk
// table of 64 consecutive chunks that should hold them: a window that begins a little in front of the chunk the step's
// first rank is estimated to live in, rank * n_chunks / n_newlines.  The estimate was double-precision arithmetic in every
// lane, once per step, on values that are the same in the whole wavefront; here it is integer arithmetic the scalar unit
// does: the ratio once per wavefront as a binary fraction (LineWindow), one 64-bit multiplication and a shift per step.
//
// What the kernel needs of it: the window must not begin LATER than the double-precision one did - a window that begins
// behind the chunk of the step's first rank sends the step to the general kernel - and not much earlier (the window is
// 64 chunks, a step takes up to 16).  line_window_start gives the chunk of
//
//     floor(rank * n_chunks / n_newlines - d),   2^-16 <= d < 2^-16 + rank / 2^frac_bits
//
// less the two chunks of margin the kernel always kept.  The double-precision estimate lies within 2^-19 of the exact
// quotient (three roundings of 2^-53 each, estimates below 2^32), so with rank / 2^frac_bits < 1/2 the start is the
// double-precision one or the chunk in front of it, never a later one.  frac_bits is as large as 64-bit products allow:
// 62 less the bits of n_chunks, which keeps rank / 2^frac_bits below 1/2 while n_newlines * n_chunks < 2^60 (an image of
// 512 GiB of 150-base reads); beyond that the window only begins earlier.
//
// No HIP header is needed: a CPU program includes this file and runs the very arithmetic the kernel compiles
// (tests/test_line_window.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQG_LINE_WINDOW_HD __host__ __device__ inline
#else
#define FQG_LINE_WINDOW_HD inline
#endif

namespace fqg {

constexpr uint32_t kLineWindowChunks = 64;  // chunks of a window: one per lane
constexpr uint32_t kLineWindowMargin = 2;   // chunks the window begins in front of the estimate
constexpr int kLineWindowBiasBits = 16;     // the estimate is lowered by 2^-16 of a chunk: below the double-precision one

struct LineWindow {
  uint64_t ratio;    // floor(n_chunks * 2^frac_bits / n_newlines); 0 without newlines
  uint64_t round;    // 2^frac_bits - 2^(frac_bits - kLineWindowBiasBits): one chunk less the bias
  uint32_t frac_bits;
  uint32_t last;     // the last chunk a window may begin at: n_chunks - 64, 0 for a table of 64 chunks or fewer
};

// once per wavefront (one 64-bit division)
FQG_LINE_WINDOW_HD LineWindow line_window(uint32_t n_chunks, uint64_t n_newlines) {
  LineWindow w;
  const int bits = n_chunks ? 32 - __builtin_clz(n_chunks) : 0;
  w.frac_bits = (uint32_t)(62 - bits);  // 30 .. 62
  w.ratio = n_newlines ? ((uint64_t)n_chunks << w.frac_bits) / n_newlines : 0;
  w.round = (1ull << w.frac_bits) - (1ull << (w.frac_bits - kLineWindowBiasBits));
  w.last = n_chunks > kLineWindowChunks ? n_chunks - kLineWindowChunks : 0;
  return w;
}

// The first chunk of the window of the step whose first rank is `rank` (<= n_newlines: the product is below 2^62), kept
// inside the chunk table: [0, n_chunks - 64].  No comparison of 64-bit values (the scalar unit has none but for equality):
// one chunk is added with the bias and taken off with the margin; the sum is n_chunks + 1 at the most (a table of 2^32 - 1
// chunks, 16 TiB, is one too many).
FQG_LINE_WINDOW_HD uint32_t line_window_start(const LineWindow& w, uint64_t rank) {
  const uint32_t est1 = (uint32_t)((rank * w.ratio + w.round) >> w.frac_bits);  // floor(estimate - bias) + 1
  const uint32_t cw = est1 > kLineWindowMargin + 1 ? est1 - (kLineWindowMargin + 1) : 0;
  return cw < w.last ? cw : w.last;
}

}  // namespace fqg
