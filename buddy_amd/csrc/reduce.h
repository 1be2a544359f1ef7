// The fixed-order sums and the frame and tile counts of the evaluation kernels (metrics.hip, spectral.hip, align.hip, acoustics.hip; capi.hip takes
// frames_of for its checks).  Private to them: nothing on the sampler's or the trainer's path includes this header.
//
// Every sum here has one association whatever the batch: a wave adds lanes l and l ^ off for off = 32, 16, 8, 4, 2, 1, a workgroup then adds its wave
// totals in wave order.  Lane 0 of this butterfly adds the same pairs in the same order as lane 0 of a __shfl_down tree (at every step its partner is
// lane off, whose value was built from the lanes below 2 off in both forms), so the one form gives the bits of the tree the files had before.
//
// NOT folded in, on purpose: level.hip's block_sum is a halving tree over 256 LDS entries (another association: other bits), and optim.hip's
// block_sum_256 / block_sum_256_u64 are the trainer's sums, the u64 one exact by construction.
#pragma once
#include "common.h"

namespace buddy {
// full frames of ``frame`` samples at hop ``hop`` in ``len`` samples; int in the kernels, long long in the host checks
template <typename T>
__host__ __device__ __forceinline__ T frames_of(T len, int frame, int hop) { return len >= frame ? (len - frame) / hop + 1 : 0; }

inline unsigned tiles_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ double wave_sum(double v) {       // the sum lands in every lane: butterfly, the same order in every lane
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// K sums over a workgroup of NW waves (a call names K, NW comes with the LDS array); they land in every thread.  ``lds`` may be reused by the next
// call: the leading barrier covers it
template <int K, int NW>
__device__ __forceinline__ void block_sum(double (&v)[K], double (&lds)[NW][K], int tid) {
#pragma unroll
  for (int q = 0; q < K; ++q) v[q] = wave_sum(v[q]);
  __syncthreads();                            // the previous use of lds has been read
  if ((tid & 63) == 0)
#pragma unroll
    for (int q = 0; q < K; ++q) lds[tid >> 6][q] = v[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < K; ++q) {
    double s = lds[0][q];
    for (int w = 1; w < NW; ++w) s += lds[w][q];
    v[q] = s;
  }
}

// the maximum over a workgroup of NW waves, in every thread: the same butterfly and the same wave order (a maximum has one value in any order; the
// fixed order keeps a NaN's path fixed too).  ``lds`` may be reused by the next call: the leading barrier covers it
template <int NW>
__device__ __forceinline__ double block_max(double v, double (&lds)[NW], int tid) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  __syncthreads();                            // the previous use of lds has been read
  if ((tid & 63) == 0) lds[tid >> 6] = v;
  __syncthreads();
  double s = lds[0];
  for (int w = 1; w < NW; ++w) s = fmax(s, lds[w]);
  return s;
}
}  // namespace buddy
