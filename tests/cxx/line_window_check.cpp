// line_window_check.cpp - line_window_start (fastq_utils_amd/csrc/fqg_line_window.h, the text k_stream_lines_fast
// compiles): the first chunk of a step's window by integer arithmetic against the double-precision formula the kernel
// had before, restated here.
//
//   densities  28 .. 64 newlines per 4 KiB chunk in steps of 1/8 (n_newlines = density * n_chunks, rounded down)
//   n_chunks   257, 4096 (every step) and 8 500 000 (the bench's image: 10 000 steps spread over it, the first two and
//              the last two among them)
//
// For every step: the integer start is the double-precision one or ONE LESS, never later (a window that begins behind
// the chunk of the step's first rank sends the step to the general kernel), the product rank * ratio stays below 2^62
// (no wrap), and the start lies inside the chunk table.  The step beyond the last - the kernel requests its window too and
// clamps it to the last step - is included.
// Prints the counts; exit status 1 on the first difference.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../fastq_utils_amd/csrc/fqg_line_window.h"

// the formula of the kernel before (window_request in stream_lines_fast_body and k_stream_lines)
static uint32_t start_double(uint64_t step, uint64_t n_steps, uint32_t n_chunks, uint64_t n_newlines) {
  const double chunks_per_line = n_newlines ? (double)n_chunks / (double)n_newlines : 0.0;
  const uint64_t g = (step < n_steps ? step : n_steps - 1) * 2;
  const uint64_t Rw = g ? 4 * g * 64 - 1 : 0;
  const double est = (double)Rw * chunks_per_line;
  uint32_t cw = est > 2.0 ? (uint32_t)(est - 2.0) : 0u;
  if (cw + 64 > n_chunks) cw = n_chunks > 64u ? n_chunks - 64 : 0u;
  return cw;
}

// as the kernel calls it
static uint32_t start_integer(const fqg::LineWindow& w, uint64_t step, uint64_t n_steps) {
  const uint64_t s = step < n_steps ? step : n_steps - 1;
  return fqg::line_window_start(w, s ? s * 512 - 1 : 0);
}

static unsigned long long g_cases = 0, g_equal = 0, g_one_less = 0, g_clamped = 0;

static bool check(uint32_t n_chunks, uint64_t n_newlines, uint64_t step, uint64_t n_steps, const fqg::LineWindow& w) {
  const uint32_t want = start_double(step, n_steps, n_chunks, n_newlines), got = start_integer(w, step, n_steps);
  const uint64_t s = step < n_steps ? step : n_steps - 1, rank = s ? s * 512 - 1 : 0;
  const unsigned __int128 prod = (unsigned __int128)rank * w.ratio;
  bool ok = (got == want || got + 1 == want) && rank <= n_newlines && prod < ((unsigned __int128)1 << 62) &&
            (n_chunks > 64 ? got <= n_chunks - 64 : got == 0);
  ++g_cases;
  if (got == want) ++g_equal;
  else ++g_one_less;
  if (n_chunks > 64 && want == n_chunks - 64) ++g_clamped;
  if (!ok)
    std::printf("n_chunks=%u n_newlines=%llu step=%llu of %llu: integer %u, double %u\n", n_chunks,
                (unsigned long long)n_newlines, (unsigned long long)step, (unsigned long long)n_steps, got, want);
  return ok;
}

int main() {
  const uint32_t sizes[] = {257u, 4096u, 8500000u};
  for (uint32_t n_chunks : sizes) {
    for (int d8 = 28 * 8; d8 <= 64 * 8; ++d8) {
      const uint64_t n_newlines = (uint64_t)d8 * n_chunks / 8;
      const uint64_t n_groups = (n_newlines + 255) / 256, n_steps = (n_groups + 1) / 2;  // (n_lines = n_newlines)
      const fqg::LineWindow w = fqg::line_window(n_chunks, n_newlines);
      if (n_chunks < 100000u) {
        for (uint64_t step = 0; step <= n_steps; ++step)
          if (!check(n_chunks, n_newlines, step, n_steps, w)) return 1;
      } else {
        const uint64_t stride = n_steps / 9996;
        uint64_t n = 0;
        for (uint64_t step = 0; step < n_steps; step += (step < 2 || step + 2 >= n_steps) ? 1 : stride, ++n)
          if (!check(n_chunks, n_newlines, step, n_steps, w)) return 1;
        for (uint64_t step = n_steps - 2; step <= n_steps; ++step)
          if (!check(n_chunks, n_newlines, step, n_steps, w)) return 1;
        if (n < 9990) {
          std::printf("only %llu steps of the large image\n", (unsigned long long)n);
          return 1;
        }
      }
    }
  }
  // images without a window of their own: no newline, fewer chunks than a window, exactly one window
  for (uint32_t n_chunks : {1u, 63u, 64u, 65u})
    for (uint64_t n_newlines : {(uint64_t)0, (uint64_t)1, (uint64_t)40 * n_chunks}) {
      const uint64_t n_steps = n_newlines / 512 + 1;
      const fqg::LineWindow w = fqg::line_window(n_chunks, n_newlines);
      for (uint64_t step = 0; step <= n_steps; ++step)
        if (!check(n_chunks, n_newlines, step, n_steps, w)) return 1;
    }
  std::printf("cases=%llu equal=%llu one_less=%llu clamped=%llu\n", g_cases, g_equal, g_one_less, g_clamped);
  return 0;
}
