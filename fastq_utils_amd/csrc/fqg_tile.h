// fqg_tile.h - what the tile kernels of every file share: wavefront helpers, the SWAR byte test, the 64-bit exclusive
// scan of u32 lengths (one span of kScan64Span per workgroup, then the span sums) and the flush of an LDS image to its
// 16-byte aligned place in memory.  Included by every kernel file that uses one of them.
#pragma once
#include "fqg_device.h"

namespace fqg {

// ---- wavefront helpers --------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t rl64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}

// 0x80 in every byte of x that equals c
__device__ __forceinline__ uint64_t bytes_eq(uint64_t x, uint8_t c) {
  const uint64_t y = x ^ (0x0101010101010101ull * c);
  const uint64_t t = ((y & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | y;
  return ~(t | 0x7F7F7F7F7F7F7F7Full);
}

typedef uint32_t bc_u32x4 __attribute__((ext_vector_type(4)));

// ---- 64-bit exclusive scan of u32 lengths: 2048 per workgroup ---------------------------------
constexpr int kScan64Span = kBlock * 8;
typedef unsigned long long bc_u64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void scan64_a_body(const uint32_t* __restrict__ in, uint64_t n,
                                              unsigned long long* __restrict__ local,
                                              unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long s_w[kBlock / kWave];
  const uint64_t first = (uint64_t)blockIdx.x * kScan64Span + threadIdx.x * 8;
  // a span that lies inside the array (all but the last one), arrays on 16-byte addresses: the lane's eight lengths in two
  // loads, its eight offsets in four stores
  const bool whole = ((uint64_t)blockIdx.x + 1) * kScan64Span <= n && (((uintptr_t)in | (uintptr_t)local) & 15u) == 0;
  unsigned long long v[8], sum = 0;
  if (whole) {
    const bc_u32x4 a = *reinterpret_cast<const bc_u32x4*>(in + first), b = *reinterpret_cast<const bc_u32x4*>(in + first + 4);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
#pragma unroll
    for (int i = 0; i < 8; ++i) sum += v[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = first + i < n ? in[first + i] : 0u;
      sum += v[i];
    }
  }
  unsigned long long incl = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(incl, d, 64);
    if ((int)(threadIdx.x & 63) >= d) incl += o;
  }
  if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = incl;
  __syncthreads();
  unsigned long long before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) {
    if (w < (int)(threadIdx.x >> 6)) before += s_w[w];
    all += s_w[w];
  }
  unsigned long long run = before + incl - sum;
  if (whole) {
    unsigned long long o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      o[i] = run;
      run += v[i];
    }
#pragma unroll
    for (int i = 0; i < 8; i += 2) *reinterpret_cast<bc_u64x2*>(local + first + i) = bc_u64x2{o[i], o[i + 1]};
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (first + i < n) local[first + i] = run;
      run += v[i];
    }
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = all;
}
// The arrays of up to kScan64Streams scans that run as ONE launch pair (blockIdx.y picks the stream): a launch costs more
// than the scan of a few million lengths.  A single scan fills entry 0.
constexpr int kScan64Streams = 6;
struct Scan64 {
  const uint32_t* in[kScan64Streams];
  unsigned long long* local[kScan64Streams];  // exclusive prefix inside a span of kScan64Span
  unsigned long long* sums[kScan64Streams];   // the span sums, then (k_scan64_b) their exclusive prefix
  unsigned long long* total;                  // [streams]
};
__global__ __launch_bounds__(kBlock) void k_scan64_a(Scan64 t, uint64_t n) {  // grid (spans, streams)
  scan64_a_body(t.in[blockIdx.y], n, t.local[blockIdx.y], t.sums[blockIdx.y]);
}

// one workgroup: exclusive prefix over the span sums, total into *total
// (2048 sums per round - eight per thread, a wavefront scan by shuffles, one exchange through LDS: the scan of the
// 97 656 span sums of 200 M lengths took 0.49 ms as 382 rounds of a 256-wide scan with sixteen barriers each)
__device__ __forceinline__ void scan64_b_body(unsigned long long* __restrict__ sums, uint64_t nb,
                                              unsigned long long* __restrict__ total) {
  __shared__ unsigned long long s_w[kBlock / kWave];
  unsigned long long carry = 0;  // (the same in every thread)
  for (uint64_t base = 0; base < nb; base += kScan64Span) {
    const uint64_t first = base + threadIdx.x * 8;
    unsigned long long v[8], sum = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = first + i < nb ? sums[first + i] : 0ull;
      sum += v[i];
    }
    unsigned long long incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_up(incl, d, 64);
      if ((int)(threadIdx.x & 63) >= d) incl += o;
    }
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = incl;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) {
      if (w < (int)(threadIdx.x >> 6)) before += s_w[w];
      all += s_w[w];
    }
    unsigned long long run = carry + before + incl - sum;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (first + i < nb) sums[first + i] = run;
      run += v[i];
    }
    carry += all;
    __syncthreads();  // (s_w is written again in the next round)
  }
  if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(kBlock) void k_scan64_b(Scan64 t, uint64_t nb) {  // grid (1, streams)
  scan64_b_body(t.sums[blockIdx.y], nb, t.total + blockIdx.y);
}

// ---- an LDS image to memory ------------------------------------------------------------------
__device__ __forceinline__ void emit_flush(const uint8_t* __restrict__ buf, uint32_t skew, uint32_t len,
                                           uint8_t* __restrict__ dst, int lane) {
  // buf[skew .. skew+len) -> dst[0 .. len), with (dst - skew) 16-byte aligned
  uint8_t* g0 = dst - skew;
  const uint32_t end = skew + len;
  const uint32_t first_full = (skew + 15u) & ~15u, last_full = end & ~15u;
  for (uint32_t i = skew + lane; i < (first_full < end ? first_full : end); i += kWave) g0[i] = buf[i];
  typedef uint32_t fl_u32x4 __attribute__((ext_vector_type(4)));
  uint32_t u = first_full + 16u * lane;
  for (; u + 3u * 16u * kWave + 16u <= last_full; u += 4u * 16u * kWave) {  // four LDS reads in flight per lane
    fl_u32x4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const fl_u32x4*>(buf + u + (uint32_t)q * 16u * kWave);
#pragma unroll
    for (int q = 0; q < 4; ++q) __builtin_nontemporal_store(v[q], reinterpret_cast<fl_u32x4*>(g0 + u + (uint32_t)q * 16u * kWave));
  }
  for (; u + 16u <= last_full; u += 16u * kWave)
    __builtin_nontemporal_store(*reinterpret_cast<const fl_u32x4*>(buf + u), reinterpret_cast<fl_u32x4*>(g0 + u));
  if (last_full >= first_full)
    for (uint32_t i = last_full + lane; i < end; i += kWave) g0[i] = buf[i];
}

}  // namespace fqg
