// names_build_plan_print.cpp - what build_plan (fastq_utils_amd/csrc/fqg_names_build_plan.h) gives for one table, as
// names_build asks for it under FQGPU_NAMES_BUILD=1 (mode 1, no forced part size, parts of 2^12 and 2^13 slots), so that a
// test can size its input by the plan's own numbers:  names_build_plan_print <capacity> <n_records> <empty: 0 | 1>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../fastq_utils_amd/csrc/fqg_names_build_plan.h"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const fqg::BuildPlan p = fqg::build_plan(strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10), atoi(argv[3]) != 0, 1, 0, 12, 13);
  printf("applies=%d part_log=%u part_bits=%u bits0=%u bits1=%u cap0=%llu cap1=%llu\n", p.applies ? 1 : 0, p.part_log, p.part_bits,
         p.bits0, p.bits1, p.cap0, p.cap1);
  return 0;
}
