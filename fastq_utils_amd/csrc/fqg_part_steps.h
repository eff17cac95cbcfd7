// fqg_part_steps.h - which steps the line workers of one part of the parted streaming pass do, if any.
//
// The launch that carries pass 1 of part p + 1 carries the line workers of part p (k_stream_pass1_lines,
// fqg_stream_kernels.hip).  They see the newlines up to the end of their part (R) and of the part before (R0) and the
// chunks in front of the launch's own (chunk_first), and do the FULL steps below R: every rank of such a step has a
// staged entry.  They run only where the kernel without a search pays - 32..60 newlines in an average chunk so far, the
// rule the host applies to the whole image (stream_lines) - so with read lengths that drift along the image the workers
// of one part may decline while those of another would run.  What the host starts behind the parts begins at ONE step
// (CallState::lines_done_steps): the steps in front of it must all be done.  Hence the rule here: the workers of a part
// run only directly behind the steps that are done - the part before them ran and ended at their own first step - and a
// part that declines ends the work of the line workers for the call (kPartDeclined is no step any part begins at).
//
// What a part leaves is CallState::lines_done[part], written by its launch and read by the NEXT launch only: stream
// order between the launches, no workgroup reads what another of the same launch writes.
//
// No HIP header is needed: a CPU program includes this file and runs the very decision the kernel compiles
// (tests/test_part_steps.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQG_PART_HD __host__ __device__ inline
#else
#define FQG_PART_HD inline
#endif

namespace fqg {

constexpr uint64_t kPartStepRanks = 512;     // newlines of a step: 4 lines x 64 lanes x 2 records a lane (4 * kWave * kLinesPer)
constexpr uint64_t kPartDeclined = ~0ull;    // CallState::lines_done of a part whose workers did not run
constexpr double kPartNlMin = 32.0, kPartNlMax = 60.0;  // newlines per chunk the kernel without a search is made for

struct PartSteps {
  bool run;
  uint64_t step_lo, step_hi;  // run: the steps [step_lo, step_hi) - none when the part holds no full step of its own
  uint64_t done;              // -> CallState::lines_done[part]: step_hi, or kPartDeclined
};

// R0, R: newlines up to the end of the part before (0 for the first part) and of this part; chunk_first: chunks in front
// of the launch that carries the workers (the chunks of the parts up to this one); prev_done: lines_done of the part
// before (0 for the first part)
FQG_PART_HD PartSteps part_steps(uint64_t R0, uint64_t R, uint32_t chunk_first, uint64_t prev_done) {
  PartSteps p;
  p.step_lo = R0 / kPartStepRanks;
  p.step_hi = R / kPartStepRanks;
  const double per_chunk = (double)R / (double)(chunk_first ? chunk_first : 1u);
  p.run = !(per_chunk > kPartNlMax || per_chunk < kPartNlMin) && prev_done == p.step_lo;
  p.done = p.run ? p.step_hi : kPartDeclined;
  return p;
}

}  // namespace fqg
