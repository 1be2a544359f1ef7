// The exact order statistic of a row of doubles (compare.hip: the percentiles of the resampled statistics; decay.hip: the quartiles of a row's decay
// times): an 8-bit radix select on the order-preserving 64-bit key of a double, most significant byte first, by one workgroup of 256 threads.  A pass
// counts the byte of the elements that share the prefix found so far (256 LDS counters; integer atomics, whose result has no order), a scan finds the
// byte at which the count passes the rank.  After eight passes the key is the element: exact for any length, no copy of the row.
#pragma once
#include "common.h"

namespace buddy {
constexpr int SEL_T = 256;                    // threads of a workgroup that selects: one per counter

// exclusive prefix of one unsigned per thread over the workgroup (thread order); ``ws`` holds the wave totals
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned (&ws)[SEL_T / 64], int tid, unsigned* total) {
  const int lane = tid & 63, wave = tid >> 6;
  unsigned inc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  __syncthreads();                            // the previous use of ws has been read
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  unsigned before = 0, all = 0;
  for (int w = 0; w < SEL_T / 64; ++w) {
    if (w < wave) before += ws[w];
    all += ws[w];
  }
  if (total) *total = all;
  return before + inc - v;
}

// the order-preserving key of a double: negative values complemented, the others with the sign bit set (-0 sorts below +0)
__device__ __forceinline__ unsigned long long key_of(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double value_of(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}

// the element of rank ``rank`` (0-based, ascending) of row[0 .. R - 1], in every thread; SKIP_NAN: of its elements that are not NaN (the rank must be
// below their number).  Every thread of the workgroup must call it (barriers); hist, ws and pick are free again when it returns
template <bool SKIP_NAN>
__device__ __forceinline__ double radix_select(const double* __restrict__ row, int R, unsigned rank, unsigned (&hist)[256], unsigned (&ws)[SEL_T / 64],
                                               unsigned (&pick)[2], int tid) {
  unsigned long long prefix = 0;              // the bytes found so far, in place
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    hist[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < R; i += SEL_T) {
      const double x = row[i];
      if (SKIP_NAN && x != x) continue;
      const unsigned long long k = key_of(x);
      if (pass == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned mine = hist[tid];
    const unsigned before = block_excl_scan(mine, ws, tid, nullptr);
    if (rank >= before && rank < before + mine) { pick[0] = (unsigned)tid; pick[1] = rank - before; }
    __syncthreads();
    prefix |= (unsigned long long)pick[0] << shift;
    rank = pick[1];
    __syncthreads();                          // pick and hist are free for the next pass
  }
  return value_of(prefix);
}
}  // namespace buddy
