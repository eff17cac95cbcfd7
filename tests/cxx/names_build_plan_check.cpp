// names_build_plan_check.cpp - build_plan (fastq_utils_amd/csrc/fqg_names_build_plan.h, the rules names_build follows)
// against a table worked out by hand from those rules, with part sizes of 2^12 and 2^13 slots:
//
//   a table of 2^k slots has parts of 2^12 slots up to k = 28 (k - 16 <= 12) and of 2^13 at k = 29; a forced part size is
//   raised to k - 16 where that is larger; at least two parts (k >= part_log + 1); bits0 = min(k - part_log, 8), bits1 the
//   rest, at most 8
//   by size (mode < 0) the frame must bring capacity / 16 records into an empty index, capacity / 8 into another
//   a bucket has room for mean + 8 sqrt(mean + 1) + 64 keys, truncated
//
// Prints the counts; exit status 1 on the first difference.
#include <cstdint>
#include <cstdio>

#include "../../fastq_utils_amd/csrc/fqg_names_build_plan.h"

using fqg::BuildPlan;

static BuildPlan plan(uint32_t k, uint64_t n, bool empty, int mode, int forced) {
  return fqg::build_plan(1ull << k, n, empty, mode, forced, 12, 13);
}

struct Row {
  uint32_t k;
  int forced;
  bool applies;
  uint32_t part_log;
  int bits0, bits1;  // -1: the table does not say
};
static const Row kTable[] = {
    {12, 0, false, 0, -1, -1}, {13, 0, true, 12, 1, 0},    {16, 0, true, 12, 4, 0}, {21, 0, true, 12, 8, 1},
    {22, 0, true, 12, 8, 2},   {28, 0, true, 12, 8, 8},    {29, 0, true, 13, 8, 8}, {30, 0, false, 0, -1, -1},
    {20, 13, true, 13, 7, 0},  {29, 12, true, 13, -1, -1}, {13, 13, false, 0, -1, -1},
};

static int fails = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      printf("FAIL %s: ", #cond);                 \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
      ++fails;                                    \
    }                                             \
  } while (0)

int main() {
  int rows = 0, swept = 0, applied = 0, gates = 0;
  for (const Row& r : kTable) {
    const BuildPlan p = plan(r.k, 1ull << r.k, true, -1, r.forced);  // (n = capacity: past the gate)
    CHECK(p.applies == r.applies, "k=%u forced=%d", r.k, r.forced);
    if (r.applies && p.applies) {
      CHECK(p.part_log == r.part_log, "k=%u forced=%d part_log=%u", r.k, r.forced, p.part_log);
      if (r.bits0 >= 0) CHECK((int)p.bits0 == r.bits0 && (int)p.bits1 == r.bits1, "k=%u forced=%d bits %u %u", r.k, r.forced, p.bits0, p.bits1);
    }
    ++rows;
  }
  const int forced_all[] = {0, 12, 13};
  for (uint32_t k = 10; k <= 34; ++k)
    for (int forced : forced_all)
      for (int empty = 0; empty < 2; ++empty) {
        const BuildPlan p = plan(k, 1ull << k, empty != 0, -1, forced);
        ++swept;
        if (!p.applies) continue;
        ++applied;
        CHECK(p.bits0 + p.bits1 + p.part_log == k, "k=%u forced=%d", k, forced);
        CHECK(p.part_bits == p.bits0 + p.bits1, "k=%u forced=%d", k, forced);
        CHECK(p.bits0 <= 8 && p.bits1 <= 8, "k=%u forced=%d", k, forced);
        CHECK(p.part_log == 12 || p.part_log == 13, "k=%u forced=%d part_log=%u", k, forced, p.part_log);
        CHECK(p.n_cursors == ((size_t)1 << p.bits0) + (p.bits1 ? (size_t)1 << p.part_bits : 0), "k=%u forced=%d", k, forced);
        CHECK((p.cap1 == 0) == (p.bits1 == 0), "k=%u forced=%d cap1=%llu", k, forced, p.cap1);
      }
  // the size gate at its edge
  const uint32_t gate_k[] = {13, 16, 20, 24};
  for (uint32_t k : gate_k) {
    const uint64_t cap = 1ull << k;
    CHECK(!plan(k, cap / 16 - 1, true, -1, 0).applies, "k=%u", k);
    CHECK(plan(k, cap / 16, true, -1, 0).applies, "k=%u", k);
    CHECK(!plan(k, cap / 8 - 1, false, -1, 0).applies, "k=%u", k);
    CHECK(plan(k, cap / 8, false, -1, 0).applies, "k=%u", k);
    CHECK(!plan(k, cap / 16, false, -1, 0).applies, "k=%u", k);  // (what an empty index takes is too little for another)
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, cap / 16 - 1, cap / 8 - 1}) {
      CHECK(plan(k, n, true, 1, 0).applies && plan(k, n, false, 1, 0).applies, "k=%u n=%llu", k, (unsigned long long)n);
      CHECK(!plan(k, n, true, 0, 0).applies, "k=%u n=%llu", k, (unsigned long long)n);
    }
    CHECK(!plan(k, cap, true, 0, 0).applies && !plan(k, cap, false, 0, 0).applies, "k=%u", k);
    ++gates;
  }
  // room(1500) = 1500 + 8 sqrt(1501) + 64 = 1873.9...
  {
    const BuildPlan p = plan(15, 12000, true, 1, 0);
    CHECK(p.applies && p.bits0 == 3 && p.bits1 == 0, "bits %u %u", p.bits0, p.bits1);
    CHECK(p.cap0 == 1873, "cap0=%llu", p.cap0);
    CHECK(p.cap1 == 0, "cap1=%llu", p.cap1);
    CHECK(fqg::build_room(1500.0) == 1873, "room");
  }
  printf("rows=%d swept=%d applied=%d gates=%d fails=%d\n", rows, swept, applied, gates, fails);
  return fails ? 1 : 0;
}
