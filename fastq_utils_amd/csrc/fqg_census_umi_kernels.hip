// fqg_census_umi_kernels.hip - the census with UMI collapse (fqg_census_collapse_umis, include/fqg.h).
//
// Not a reference result: bam_umi_count counts every distinct UMI of a cell.  Behind fqg_census_finish the pairs lie
// sorted by (cell, UMI); these kernels make the table of distinct (cell, UMI) rows with their reads, give every row the
// strongest neighbour of its cell that has strictly more reads (its parent), and follow the parents to the root.
//
// Parents without a probe per neighbour.  Two values of d digits that differ in one digit agree on their high
// ceil(d/2) digits or on their low floor(d/2) digits.  In the table's own order the rows of a cell that share the high
// half are a contiguous run (pass A); in a second order of the rows, by (cell, value with its halves swapped), the rows
// that share the low half are one (pass B).  k_cu_run is both passes: one lane per row looks only inside its run - it
// walks it while the run is at most kCuWalk rows, else it searches the 4 * (digits of the varying half) candidates in
// it.  Either way the work of a row has a fixed bound, whatever the size of its cell.
#include "fqg_device.h"
#include "fqg_tile.h"

namespace fqg {

struct CensusUmi {
  unsigned long long cell, umi, reads, root;
};

constexpr int kCuWalk = 64;  // a run of at most this many rows is walked

// The digits of a packed value, three bits each (digit i, the weight 10^i, at bits 3i), and their number - for a value
// whose decimal digits are all 1..5, what char2uint_64 makes of up to 19 bases.  Any other value (0, a digit 0 or 6..9,
// twenty digits - fqg_census_append alone can bring one) has no neighbours: 0.
__device__ __forceinline__ uint32_t cu_digits(unsigned long long v, unsigned long long* pack) {
  unsigned long long pk = 0;
  uint32_t d = 0;
  bool ok = v != 0ull;
#pragma unroll 1
  for (uint32_t i = 0; i < (uint32_t)kWlMaxRescueSize && v; ++i) {
    const unsigned long long q = v / 10ull;
    const uint32_t x = (uint32_t)(v - q * 10ull);
    ok = ok && x >= 1u && x <= 5u;
    pk |= (unsigned long long)(x & 7u) << (3u * i);
    d = i + 1u;
    v = q;
  }
  *pack = pk;
  return ok && !v ? d : 0u;
}

// low * 10^h + high: the halves of a value of d digits (h = ceil(d/2) high ones) swapped - again d digits of 1..5
__device__ __forceinline__ unsigned long long cu_rotate(unsigned long long v, uint32_t d) {
  const unsigned long long pl = kWlPow10[d / 2u];
  const unsigned long long high = v / pl;
  return (v - high * pl) * kWlPow10[(d + 1u) / 2u] + high;
}

// sorted by (cell, UMI): flag[i] = 1 where a new (cell, UMI) begins
__global__ __launch_bounds__(kBlock) void k_cu_flags(const unsigned long long* __restrict__ cells,
                                                     const unsigned long long* __restrict__ umis, uint64_t n,
                                                     uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || cells[i] != cells[i - 1] || umis[i] != umis[i - 1]) ? 1u : 0u;
}

// One row per distinct pair: its UMI, its cell id (the flag/scan scheme of k_census_count, on the arrays fqg_census_finish
// left), where its pairs begin; every cell's first row.  r_head[m] and cell_first[n_cells] close the two lists.
__global__ __launch_bounds__(kBlock) void k_cu_rows(const unsigned long long* __restrict__ umis, uint64_t n,
                                                    const uint32_t* __restrict__ pflag, const unsigned long long* __restrict__ plocal,
                                                    const unsigned long long* __restrict__ pspan, const uint32_t* __restrict__ cflag,
                                                    const unsigned long long* __restrict__ clocal,
                                                    const unsigned long long* __restrict__ cspan, uint64_t m, uint64_t n_cells,
                                                    unsigned long long* __restrict__ r_umi, uint32_t* __restrict__ r_cid,
                                                    uint32_t* __restrict__ r_head, uint32_t* __restrict__ cell_first) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i == 0) {
    r_head[m] = (uint32_t)n;
    cell_first[n_cells] = (uint32_t)m;
  }
  if (i >= n || !pflag[i]) return;
  const unsigned long long row = pspan[i / kScan64Span] + plocal[i];
  const uint32_t cf = cflag[i];
  const unsigned long long cid = cspan[i / kScan64Span] + clocal[i] + cf - 1ull;
  if (row >= m || cid >= n_cells) return;  // (cannot be: the scans counted these flags)
  r_umi[row] = umis[i];
  r_cid[row] = (uint32_t)cid;
  r_head[row] = (uint32_t)i;
  if (cf) cell_first[cid] = (uint32_t)row;
}

// reads = the distance between head positions; with rot: the key of the second order and the row it belongs to
__global__ __launch_bounds__(kBlock) void k_cu_prep(const unsigned long long* __restrict__ r_umi, const uint32_t* __restrict__ r_head,
                                                    uint64_t m, uint32_t* __restrict__ r_reads, unsigned long long* __restrict__ rot,
                                                    uint32_t* __restrict__ perm) {
  const uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= m) return;
  r_reads[row] = r_head[row + 1] - r_head[row];
  if (rot) {
    const unsigned long long v = r_umi[row];
    unsigned long long pk;
    const uint32_t d = cu_digits(v, &pk);
    rot[row] = d ? cu_rotate(v, d) : v;  // (a value without neighbours: anywhere - nothing compares equal to it)
    perm[row] = (uint32_t)row;
  }
}

// between the two stable sorts of the second order: the cell ids in the order of the first, and where each came from
__global__ __launch_bounds__(kBlock) void k_cu_gather_cid(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ r_cid,
                                                          uint64_t m, uint32_t* __restrict__ key, uint32_t* __restrict__ pos) {
  const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= m) return;
  key[j] = r_cid[perm[j]];
  pos[j] = (uint32_t)j;
}
// ... and behind them: keys and rows in the final order
__global__ __launch_bounds__(kBlock) void k_cu_gather_rot(const uint32_t* __restrict__ pos, const unsigned long long* __restrict__ rot,
                                                          const uint32_t* __restrict__ perm, uint64_t m,
                                                          unsigned long long* __restrict__ rot_out, uint32_t* __restrict__ perm_out) {
  const uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= m) return;
  const uint32_t p = pos[j];
  rot_out[j] = rot[p];
  perm_out[j] = perm[p];
}

// first position in [lo, hi) whose key is not below v
__device__ __forceinline__ uint32_t cu_lower_bound(const unsigned long long* __restrict__ key, uint32_t lo, uint32_t hi,
                                                   unsigned long long v) {
#pragma unroll 1
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (key[mid] < v) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

// The row at position jj of this order is a neighbour: the better of it and `best` ("most reads, then smallest value" as
// one word - reads << 32 | (0xFFFFFFFF - row): inside a cell a smaller row is a smaller value), if it is stronger than me.
template <bool ROT>
__device__ __forceinline__ unsigned long long cu_take(uint32_t jj, const uint32_t* __restrict__ perm,
                                                      const uint32_t* __restrict__ r_reads, uint32_t mine, unsigned long long best) {
  const uint32_t row = ROT ? perm[jj] : jj;
  const uint32_t rj = r_reads[row];
  const unsigned long long w = ((unsigned long long)rj << 32) | (unsigned long long)(0xFFFFFFFFu - row);
  return rj > mine && w > best ? w : best;
}

// One lane per row, in the table's order (ROT false: key = the UMI, the low floor(d/2) digits vary inside a run) or in
// the second one (ROT true: key = the rotated UMI, perm = the row, the low ceil(d/2) digits - the value's high ones -
// vary).  Both orders are sorted by (cell, key), so the cell's rows are positions cell_first[c] .. cell_first[c + 1] of
// either, and my run is the keys of [lo, lo + 10^vary) among them.
// Two keys of digits 1..5 inside one run differ in exactly one digit iff |a - b| = k * 10^p with 1 <= k <= 4 and my
// digit p moved by k stays in 1..5 (then b is a with that digit replaced: all its digits are valid ones).
template <bool ROT>
__global__ __launch_bounds__(kBlock) void k_cu_run(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ perm,
                                                   const uint32_t* __restrict__ r_cid, const uint32_t* __restrict__ cell_first,
                                                   const uint32_t* __restrict__ r_reads, uint64_t m,
                                                   unsigned long long* __restrict__ word) {
  const uint64_t j64 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j64 >= m) return;
  const uint32_t j = (uint32_t)j64;
  const unsigned long long a = key[j];
  const uint32_t row = ROT ? perm[j] : j;
  unsigned long long pk;
  const uint32_t d = cu_digits(a, &pk);
  const uint32_t vary = ROT ? (d + 1u) / 2u : d / 2u;
  unsigned long long best = 0;
  if (vary) {
    const uint32_t mine = r_reads[row], c = r_cid[row];
    const uint32_t first = cell_first[c], end = cell_first[c + 1u];
    const unsigned long long span = kWlPow10[vary];
    const unsigned long long lo = a - a % span, hi = lo + span;  // (a < 10^19, span <= 10^10: no wrap)
    bool far = false;  // the run reaches kCuWalk rows or more to one side: it is longer than kCuWalk
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
#pragma unroll 1
      for (uint32_t k = 1;; ++k) {
        if (side == 0 ? j < first + k : j + k >= end) break;
        const uint32_t jj = side == 0 ? j - k : j + k;
        const unsigned long long b = key[jj];
        if (side == 0 ? b < lo : b >= hi) break;
        if (k == (uint32_t)kCuWalk) {
          far = true;
          break;
        }
        const bool up = b > a;
        const unsigned long long diff = up ? b - a : a - b;
        if (!diff) continue;  // (cannot be: the rows of a cell are distinct values)
        uint32_t p = ((64u - (uint32_t)__builtin_clzll(diff)) * 1233u) >> 12;  // floor(log10(diff)), or one more
        if (diff < kWlPow10[p]) --p;
        const unsigned long long pp = kWlPow10[p];
        const int kk = diff == pp ? 1 : diff == 2ull * pp ? 2 : diff == 3ull * pp ? 3 : diff == 4ull * pp ? 4 : 0;
        if (kk && p < vary) {
          const int xb = (int)((pk >> (3u * p)) & 7ull) + (up ? kk : -kk);
          if (xb >= 1 && xb <= 5) best = cu_take<ROT>(jj, perm, r_reads, mine, best);
        }
      }
    }
    if (far) {
      const uint32_t rl = cu_lower_bound(key, first, j, lo), rh = cu_lower_bound(key, j + 1u, end, hi);
#pragma unroll 1
      for (uint32_t p = 0; p < vary; ++p) {
        const int xa = (int)((pk >> (3u * p)) & 7ull);
#pragma unroll 1
        for (int x = 1; x <= 5; ++x) {
          if (x == xa) continue;
          const unsigned long long cand = a + (unsigned long long)(long long)(x - xa) * kWlPow10[p];
          const uint32_t at = cu_lower_bound(key, rl, rh, cand);
          if (at < rh && key[at] == cand) best = cu_take<ROT>(at, perm, r_reads, mine, best);
        }
      }
    }
  }
  // pass A writes every row's word; pass B runs behind it and keeps the better of the two - each row is one lane's
  if (!ROT) word[row] = best;
  else if (best > word[row]) word[row] = best;
}

// One lane per row follows the parents to the root (reads grow strictly on the way: it ends; a chain has fewer steps
// than there are rows) and writes the row's line of the table.  Per cell: the rows that are their own root - the rows
// of one cell are neighbours, so every run of a cell inside a wavefront adds once, by its first lane.  The two totals
// (rows with a parent, the longest chain) leave a workgroup once, as plain stores to its own two slots of `partial`,
// and k_cu_totals folds the slots: as two atomics per workgroup to two addresses they were 0.15 ms of this kernel's
// 0.18 on 2 M rows (8 000 workgroups: the adds to one address come one behind the other).
__global__ __launch_bounds__(kBlock) void k_cu_roots(const unsigned long long* __restrict__ word, const unsigned long long* __restrict__ r_umi,
                                                     const uint32_t* __restrict__ r_cid, const uint32_t* __restrict__ r_reads,
                                                     const CensusCell* __restrict__ lines, uint64_t m, CensusUmi* __restrict__ table,
                                                     unsigned long long* __restrict__ cell_roots, unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long s_abs[kBlock / kWave], s_max[kBlock / kWave];
  const uint64_t row = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = lane_id();
  const bool in = row < m;
  uint32_t steps = 0, cid = 0;
  if (in) {
    uint32_t r = (uint32_t)row;
    unsigned long long w = word[r];
#pragma unroll 1
    while (w && steps < m) {
      r = 0xFFFFFFFFu - (uint32_t)w;
      if (r >= m) break;  // (cannot be: a word holds a row of the table)
      ++steps;
      w = word[r];
    }
    cid = r_cid[row];
    CensusUmi t;
    t.cell = lines[cid].cell;
    t.umi = r_umi[row];
    t.reads = r_reads[row];
    t.root = r_umi[r];
    table[row] = t;
  }
  const uint32_t before = __shfl_up(cid, 1, 64);
  const bool head = in && (lane == 0 || before != cid);
  const unsigned long long hm = __ballot(head), om = __ballot(in && steps == 0u), im = __ballot(in);
  if (head) {
    const unsigned long long above = lane == 63 ? 0ull : (hm >> (lane + 1)) << (lane + 1);
    const int end = above ? __builtin_ctzll(above) : 64;  // first lane beyond my cell's run
    const unsigned long long run = (end == 64 ? ~0ull : ((1ull << end) - 1ull)) & ~((1ull << lane) - 1ull) & im;
    const unsigned long long u = (unsigned long long)__builtin_popcountll(run & om);
    if (u) atomicAdd(&cell_roots[cid], u);
  }
  unsigned long long absorbed = (unsigned long long)__builtin_popcountll(im & ~om), longest = steps;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const unsigned long long o = __shfl_down(longest, s, 64);
    longest = o > longest ? o : longest;
  }
  if (lane == 0) {
    s_abs[threadIdx.x >> 6] = absorbed;
    s_max[threadIdx.x >> 6] = longest;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0, mx = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) {
      sum += s_abs[w];
      mx = s_max[w] > mx ? s_max[w] : mx;
    }
    partial[2ull * blockIdx.x] = sum;
    partial[2ull * blockIdx.x + 1ull] = mx;
  }
}

// one workgroup: the sum of the first and the greatest of the second of k_cu_roots' `blocks` pairs of slots
__global__ __launch_bounds__(kBlock) void k_cu_totals(const unsigned long long* __restrict__ partial, uint64_t blocks,
                                                      unsigned long long* __restrict__ totals) {
  __shared__ unsigned long long s_abs[kBlock / kWave], s_max[kBlock / kWave];
  unsigned long long sum = 0, mx = 0;
  for (uint64_t b = threadIdx.x; b < blocks; b += kBlock) {
    sum += partial[2ull * b];
    const unsigned long long v = partial[2ull * b + 1ull];
    mx = v > mx ? v : mx;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    sum += __shfl_down(sum, s, 64);
    const unsigned long long o = __shfl_down(mx, s, 64);
    mx = o > mx ? o : mx;
  }
  if (lane_id() == 0) {
    s_abs[threadIdx.x >> 6] = sum;
    s_max[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    sum = mx = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) {
      sum += s_abs[w];
      mx = s_max[w] > mx ? s_max[w] : mx;
    }
    totals[0] = sum;
    totals[1] = mx;
  }
}

}  // namespace fqg
