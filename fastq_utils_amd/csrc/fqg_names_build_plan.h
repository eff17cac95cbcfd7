// fqg_names_build_plan.h - the geometry of one build of the read-name table part by part (fqg_names_build_kernels.hip), and
// whether the build applies at all: arithmetic on the table's capacity, the frame's records and two knobs.
// A table of 2^k slots is cut into parts of 2^part_log slots (what k_build_parts holds in LDS).  The keys reach their part
// through one level of 2^bits0 buckets or, beyond 2^8 parts, a second level of 2^bits1 sub-buckets under each:
// bits0 + bits1 + part_log == k.  Buckets have room for the mean of a uniform hash plus eight standard deviations.
// No HIP header is needed: a CPU program runs the very rules names_build follows (tests/test_names_build_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace fqg {

struct BuildPlan {
  bool applies = false;                   // false: the caller takes the CAS pass (the other fields are not to be used)
  uint32_t part_log = 0, part_bits = 0;   // log2 of: slots per part, parts (bits0 + bits1)
  uint32_t bits0 = 0, bits1 = 0;
  unsigned long long cap0 = 0, cap1 = 0;  // room per bucket of level 0, of level 1 (0: there is none)
  size_t n_cursors = 0;                   // one per bucket of either level
};

// room of a bucket that a uniform hash fills with `mean` keys
inline unsigned long long build_room(double mean) { return (unsigned long long)(mean + 8.0 * std::sqrt(mean + 1.0) + 64.0); }

// capacity: slots of the table (a power of two); n_records: of the frame; empty: the index holds nothing yet;
// mode: 0 never, 1 whenever the table allows it, < 0 by size; forced_part_log: 12 or 13 asks for that part size (A/B);
// part_log_min, part_log_max: the part sizes k_build_parts is instantiated for
inline BuildPlan build_plan(uint64_t capacity, uint64_t n_records, bool empty, int mode, int forced_part_log,
                            uint32_t part_log_min, uint32_t part_log_max) {
  BuildPlan p;
  if (mode == 0) return p;
  uint32_t k = 0;
  while ((1ull << k) < capacity) ++k;
  if (k < part_log_min + 1) return p;
  const uint32_t wide = k > 16 ? k - 16 : 0u;  // (two levels of 2^8 buckets reach 2^16 parts)
  p.part_log = std::min(std::max(wide, part_log_min), part_log_max);
  if (forced_part_log == 12 || forced_part_log == 13) p.part_log = std::max<uint32_t>((uint32_t)forced_part_log, wide);
  if (p.part_log > part_log_max || k < p.part_log + 1) return p;
  p.part_bits = k - p.part_log;
  p.bits0 = std::min<uint32_t>(p.part_bits, 8);
  p.bits1 = p.part_bits - p.bits0;
  if (p.bits1 > 8) return p;
  // worth it when the frame brings a sizeable share of the table: the build writes (and, for an index that is not
  // empty, first reads) every part - 8 bytes per SLOT -, the CAS pass costs by the name
  if (mode < 0 && n_records < capacity / (empty ? 16 : 8)) return p;
  p.cap0 = build_room((double)n_records / (double)(1u << p.bits0));
  p.cap1 = p.bits1 ? build_room((double)n_records / (double)(1u << p.part_bits)) : 0;
  p.n_cursors = ((size_t)1 << p.bits0) + (p.bits1 ? (size_t)1 << p.part_bits : 0);
  p.applies = true;
  return p;
}

}  // namespace fqg
