// Batched rational polyphase resampler: any-rate recordings -> the model's rate and back (buddy_amd/utils/resample.py; no reference
// counterpart, the reference's loaders assert samplerate == fs).  For x (B, Lin) and an odd-length FIR h of Nh taps, centre c = (Nh-1)/2:
//
//   y[b][n] = sum over m in [0, Lin) with 0 <= n*down - m*up + c < Nh  of  x[b][m] * h[n*down - m*up + c],   n in [0, Lout)
//
// (zero-stuff by `up`, filter, keep every `down`-th sample, zero extension at both ends).  Output n reads the polyphase branch
// h[(n*down + c) mod up + k*up] against the inputs m in [ceil((n*down - c)/up), floor((n*down + c)/up)].
//
// One workgroup produces RS_TILE consecutive outputs of one row.  The inputs that tile needs form one contiguous span; it is staged in LDS
// in segments of RS_SEG samples (one segment for every audio ratio at this tile; a very long filter or a large down/up takes several), each
// staged once and read by all outputs whose range crosses it.  The taps stay in global memory and are served by L2: neighbouring outputs
// sit on different branches (their tap indices differ by `down`), so a tile of RS_TILE outputs reads RS_TILE * Nh/up taps with no reuse
// inside the tile when up >= RS_TILE -- a copy in LDS would be read once per word staged, and the largest audio bank (160/441: 21 169 taps,
// 85 KB) would pin one workgroup per CU to do it.  In L2 the bank is fetched from HBM once and shared by every workgroup.
// fp32 accumulation in ascending m.  Runs twice per file, outside the sampling loop; written for clarity.
#include "common.h"

namespace buddy {
namespace {
constexpr int RS_NT = 256;          // threads per workgroup
constexpr int RS_PER = 4;           // outputs per thread
constexpr int RS_TILE = RS_NT * RS_PER;
constexpr int RS_SEG = 8192;        // staged input samples per pass (32 KB of LDS)

__device__ __forceinline__ long long floordiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0
__device__ __forceinline__ long long ceildiv(long long a, long long b) { return a > 0 ? (a + b - 1) / b : -((-a) / b); }    // b > 0

__global__ __launch_bounds__(RS_NT) void resample_kernel(const float* __restrict__ x, const float* __restrict__ h, float* __restrict__ y, long long Lin,
                                                         long long Lout, int Nh, int up, int down, long long tiles) {
  __shared__ float xs[RS_SEG];
  const int tid = threadIdx.x;
  const long long row = blockIdx.x / tiles, n0 = (blockIdx.x % tiles) * RS_TILE;
  const long long c = (Nh - 1) / 2;
  const float* xr = x + row * Lin;
  float* yr = y + row * Lout;
  const long long n_last = (n0 + RS_TILE < Lout ? n0 + RS_TILE : Lout) - 1;
  // the tile's input span, clipped to the signal
  long long t_lo = ceildiv(n0 * down - c, up), t_hi = floordiv(n_last * down + c, up);
  if (t_lo < 0) t_lo = 0;
  if (t_hi > Lin - 1) t_hi = Lin - 1;
  long long lo[RS_PER], hi[RS_PER];
  float acc[RS_PER];
#pragma unroll
  for (int j = 0; j < RS_PER; ++j) {
    const long long n = n0 + tid + (long long)j * RS_NT;
    acc[j] = 0.f;
    lo[j] = ceildiv(n * down - c, up);
    hi[j] = floordiv(n * down + c, up);
    if (lo[j] < t_lo) lo[j] = t_lo;
    if (hi[j] > t_hi) hi[j] = t_hi;
    if (n >= Lout) hi[j] = lo[j] - 1;            // past the end: empty range, and no store below
  }
  for (long long s0 = t_lo; s0 <= t_hi; s0 += RS_SEG) {       // uniform over the workgroup
    const long long s1 = s0 + RS_SEG - 1 < t_hi ? s0 + RS_SEG - 1 : t_hi;
    for (long long m = s0 + tid; m <= s1; m += RS_NT) xs[m - s0] = xr[m];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RS_PER; ++j) {
      const long long a = lo[j] > s0 ? lo[j] : s0, b = hi[j] < s1 ? hi[j] : s1;
      if (a > b) continue;
      const long long n = n0 + tid + (long long)j * RS_NT;
      int k = (int)(n * down - a * up + c);      // in [0, Nh) for every m in [lo, hi]; falls by `up` per input sample
      const float* xp = xs + (a - s0);
      const int cnt = (int)(b - a + 1);
      float s = acc[j];
      for (int i = 0; i < cnt; ++i, k -= up) s = fmaf(xp[i], h[k], s);
      acc[j] = s;
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < RS_PER; ++j) {
    const long long n = n0 + tid + (long long)j * RS_NT;
    if (n < Lout) yr[n] = acc[j];
  }
}
}  // namespace

long long resample_tiles(long long Lout) { return (Lout + RS_TILE - 1) / RS_TILE; }

void launch_resample(const float* x, int B, long long Lin, const float* h, int Nh, int up, int down, float* y, long long Lout, hipStream_t st) {
  const long long tiles = resample_tiles(Lout);
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(tiles * B)), dim3(RS_NT), 0, st, x, h, y, Lin, Lout, Nh, up, down, tiles);
}

}  // namespace buddy
