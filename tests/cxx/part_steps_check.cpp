// part_steps_check.cpp - part_steps (fastq_utils_amd/csrc/fqg_part_steps.h, the text k_stream_pass1_lines compiles): the
// steps the line workers of the parted streaming pass do, part after part, on every sequence of one to four parts with
//
//   densities  20, 31.9, 32, 45, 60, 60.1, 90 newlines per 4 KiB chunk (31.9 rounded down to whole newlines, 60.1 up:
//              each stays on its side of the bound), once as the density of the PART (the cumulative one, which the
//              workers look at, then drifts between them) and once as the CUMULATIVE density at the part's end (every
//              bound met exactly at every part; sequences whose newline count would fall are left out)
//   sizes      1, 13, 4096 and 5000 chunks a part (4096 is the part of the tests; hardly any count of newlines is a
//              multiple of the 512 of a step)
//
// The parts are chained as the launches chain them: what a part leaves (PartSteps::done) is the next part's prev_done, and
// lines_done_steps is written by the parts that run.  For every sequence:
//   - the ranges of the parts that ran are contiguous from step 0: no gap, no overlap
//   - lines_done_steps is the end of the last range (0: none ran)
//   - the parts that run are the in-range parts in front of the first one out of range (the bounds restated in integers)
//   - a sequence in range throughout gives [R(p-1) / 512, R(p) / 512) for every part: what the kernel did before
// The rule the kernel had before (every part decides alone, from the newlines of the part before) is restated and run
// through the first check: the number of sequences in which it leaves a gap is printed (old_gaps), and must not be 0 -
// the check sees what it is there for.
// Prints the counts; exit status 1 on the first difference.
#include <cstdint>
#include <cstdio>

#include "../../fastq_utils_amd/csrc/fqg_part_steps.h"

static const int kDens10[] = {200, 319, 320, 450, 600, 601, 900};  // tenths of a newline per chunk
static const uint32_t kSizes[] = {1, 13, 4096, 5000};
constexpr int kND = 7, kNS = 4, kMaxParts = 4;

// newlines of `chunks` chunks at d10 / 10 a chunk: down below a bound, up above one
static uint64_t newlines(int d10, uint64_t chunks) {
  const uint64_t x = (uint64_t)d10 * chunks;
  return d10 == 601 ? (x + 9) / 10 : x / 10;
}

struct Range {
  uint64_t lo, hi;
};
struct Outcome {
  int n_ranges = 0;
  Range r[kMaxParts];
  uint64_t lines_done_steps = 0;
  bool ran[kMaxParts] = {false, false, false, false};
};

// the launches of a call, one after the other (k_stream_pass1_lines and the CallState between them)
static Outcome chain(int n, const uint64_t* R, const uint32_t* C) {
  Outcome o;
  uint64_t lines_done[kMaxParts] = {0, 0, 0, 0};
  for (int p = 0; p < n; ++p) {
    const fqg::PartSteps ps = fqg::part_steps(p ? R[p - 1] : 0, R[p], C[p], p ? lines_done[p - 1] : 0);
    lines_done[p] = ps.done;
    if (!ps.run) continue;
    o.ran[p] = true;
    o.lines_done_steps = ps.step_hi;
    o.r[o.n_ranges++] = {ps.step_lo, ps.step_hi};
  }
  return o;
}

// the rule before: a part looks at its own density alone
static Outcome chain_old(int n, const uint64_t* R, const uint32_t* C) {
  Outcome o;
  for (int p = 0; p < n; ++p) {
    const double per_chunk = (double)R[p] / (double)(C[p] ? C[p] : 1u);
    if (per_chunk > 60.0 || per_chunk < 32.0) continue;
    o.ran[p] = true;
    o.lines_done_steps = R[p] / 512;
    o.r[o.n_ranges++] = {(p ? R[p - 1] : 0) / 512, R[p] / 512};
  }
  return o;
}

static bool contiguous(const Outcome& o) {
  uint64_t at = 0;
  for (int i = 0; i < o.n_ranges; ++i) {
    if (o.r[i].lo != at || o.r[i].hi < o.r[i].lo) return false;
    at = o.r[i].hi;
  }
  return o.lines_done_steps == at;
}

static unsigned long long g_cases = 0, g_in_range = 0, g_declined = 0, g_old_gaps = 0, g_odd = 0;

static bool check(int n, const uint64_t* R, const uint32_t* C, const char* mode) {
  ++g_cases;
  const Outcome o = chain(n, R, C);
  bool ok = contiguous(o);
  // the parts that run: in range (in integers: 32 C <= R <= 60 C), and so was every part in front of them
  bool all_in = true, still = true;
  for (int p = 0; p < n; ++p) {
    const bool in = R[p] >= 32ull * C[p] && R[p] <= 60ull * C[p];
    all_in = all_in && in;
    still = still && in;
    ok = ok && o.ran[p] == still;
    if (R[p] % 512) ++g_odd;
  }
  if (all_in) {
    ++g_in_range;
    ok = ok && o.n_ranges == n && o.lines_done_steps == R[n - 1] / 512;
    for (int p = 0; ok && p < n; ++p) ok = o.r[p].lo == (p ? R[p - 1] : 0) / 512 && o.r[p].hi == R[p] / 512;
    const Outcome old = chain_old(n, R, C);
    ok = ok && old.n_ranges == o.n_ranges && old.lines_done_steps == o.lines_done_steps;
    for (int p = 0; ok && p < n; ++p) ok = old.r[p].lo == o.r[p].lo && old.r[p].hi == o.r[p].hi;
  } else {
    ++g_declined;
    if (!contiguous(chain_old(n, R, C))) ++g_old_gaps;
  }
  if (!ok) {
    std::printf("%s, %d parts:", mode, n);
    for (int p = 0; p < n; ++p) std::printf(" R=%llu C=%u ran=%d", (unsigned long long)R[p], C[p], (int)o.ran[p]);
    std::printf(" ranges");
    for (int i = 0; i < o.n_ranges; ++i) std::printf(" [%llu,%llu)", (unsigned long long)o.r[i].lo, (unsigned long long)o.r[i].hi);
    std::printf(" lines_done_steps=%llu\n", (unsigned long long)o.lines_done_steps);
  }
  return ok;
}

int main() {
  unsigned long long skipped = 0;
  for (int n = 1; n <= kMaxParts; ++n) {
    int total = 1;
    for (int i = 0; i < n; ++i) total *= kND * kNS;
    for (int code = 0; code < total; ++code) {
      int d[kMaxParts], s[kMaxParts], c = code;
      for (int p = 0; p < n; ++p) {
        d[p] = kDens10[c % kND];
        c /= kND;
        s[p] = (int)kSizes[c % kNS];
        c /= kNS;
      }
      uint64_t R[kMaxParts];
      uint32_t C[kMaxParts];
      // the density of each part
      uint64_t r = 0;
      uint32_t ch = 0;
      for (int p = 0; p < n; ++p) {
        r += newlines(d[p], (uint64_t)s[p]);
        ch += (uint32_t)s[p];
        R[p] = r;
        C[p] = ch;
      }
      if (!check(n, R, C, "density of the part")) return 1;
      // the cumulative density at each part's end
      bool falls = false;
      for (int p = 0; p < n; ++p) {
        R[p] = newlines(d[p], C[p]);
        falls = falls || (p && R[p] < R[p - 1]);
      }
      if (falls) {
        ++skipped;
        continue;
      }
      if (!check(n, R, C, "cumulative density")) return 1;
    }
  }
  std::printf("cases=%llu in_range=%llu declined=%llu old_gaps=%llu odd=%llu skipped=%llu\n", g_cases, g_in_range, g_declined,
              g_old_gaps, g_odd, skipped);
  return 0;
}
