// Diffuse noise fields by plane-wave superposition (buddy_amd/utils/noise.py; Habets & Gannot 2007; no reference counterpart):
//   out[b][d][i] = scale * sum_n sum_k taps[b][n][d][k] * s_{b,n}[i + P - first[b][n][d] - k],   s_{b,n}[j] = 0 outside 0 <= j < L + 2 P,
// with s_{b,n} the kind-0 normals of buddy_philox_fill for (keys[b], purpose, draw0 + n, j): they are generated here, where they are consumed, and
// never stored (at B = 8, N = 512, L = 64 000 they would be about 1 GB).
//
//   noise_bank    one workgroup of NZ_T threads per (item b, tile of NZ_T output samples), one output sample per thread, D accumulators in double.
//                 The waves go through LDS NZ_NC at a time: their tap rows and first lags are staged, then for each wave a window of NZ_SW source
//                 samples is generated from Philox into LDS as doubles (one block of four normals per thread and pass), then every thread walks
//                 waves ascending, microphones, taps ascending.  So the terms of a sample are added in the order (n, k) ascending whatever the
//                 chunking, the batch or the grid: no atomics, and a row's bits do not depend on B.
//
// A wave's window starts at the four-aligned sample at or below i0 + P - fmax - (W - 1), fmax the largest first lag of its D rows, and covers every
// row whose first lag lies within NZ_SPAN of fmax: real geometries (|tau| <= 64 samples) always do.  A row further away -- a first lag no geometry
// produces -- still follows the definition: its samples are generated one by one from Philox with the range test (slow, and uniform over the
// workgroup, so no divergence).  Window entries outside 0 <= j < L + 2 P are stored as zeros, so the fast path needs no test.
#include "../../include/buddy_hip.h"
#include "common.h"
#include "net.h"
#include "philox.h"

#include <cmath>

using namespace buddy;

namespace {

constexpr int NZ_T = 256;                     // threads per workgroup = output samples per tile (buddy_noise_tile)
constexpr int NZ_MAXW = 80;                   // taps per filter at most (buddy_noise_max_taps) = 2 Hw of the fractional-delay kernel
constexpr int NZ_MAXD = 8;                    // microphones at most
constexpr int NZ_NC = 4;                      // waves per LDS chunk
constexpr int NZ_SPAN = 128;                  // first lags of one wave's rows this far below the largest share its window (2 M, M = 64)
constexpr int NZ_SW = ((NZ_T + NZ_MAXW - 1 + NZ_SPAN + 3 + 3) / 4) * 4;      // window: tile + taps - 1 + span + the alignment slack, in blocks of 4

// LDS: NZ_NC * NZ_SW * 8 = 14 976 B of sources + NZ_NC * NZ_MAXD * NZ_MAXW * 8 = 20 480 B of taps + 128 B of lags = 35.6 KB: four workgroups per CU
template <int D>
__global__ __launch_bounds__(NZ_T) void noise_bank_kernel(const double* __restrict__ taps, const int* __restrict__ first, const uint32_t* __restrict__ keys,
                                                          uint32_t purpose, uint32_t draw0, float* __restrict__ out, int N, int W, int P, long long L, double scale) {
  __shared__ double s_src[NZ_NC][NZ_SW];
  __shared__ double s_tap[NZ_NC * NZ_MAXD * NZ_MAXW];
  __shared__ int s_first[NZ_NC * NZ_MAXD];
  const int tid = threadIdx.x, b = blockIdx.y;
  const long long i0 = (long long)blockIdx.x * NZ_T, i = i0 + tid;
  const long long S = L + 2LL * P;                                      // source samples per wave
  const uint32_t k0 = keys[2 * b], k1 = keys[2 * b + 1];
  constexpr int NBLK = NZ_SW / 4;
  double acc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) acc[d] = 0.0;

  for (int c0 = 0; c0 < N; c0 += NZ_NC) {
    const int nc = min(NZ_NC, N - c0);
    // ---- the chunk's tap rows and first lags: (nc, D, W) and (nc, D) are contiguous in (B, N, D, W) and (B, N, D) ----
    const long long row0 = ((long long)b * N + c0) * D;
    for (int e = tid; e < nc * D * W; e += NZ_T) s_tap[e] = taps[row0 * W + e];
    if (tid < nc * D) s_first[tid] = first[row0 + tid];
    __syncthreads();
    // ---- the chunk's source windows, one Philox block of four normals per thread and pass ----
    for (int e = tid; e < nc * NBLK; e += NZ_T) {
      const int w = e / NBLK, q = e - w * NBLK;
      long long fmax = s_first[w * D];
#pragma unroll
      for (int d = 1; d < D; ++d) fmax = max(fmax, (long long)s_first[w * D + d]);
      const long long j0 = (((i0 + P - fmax - (W - 1)) >> 2) + q) * 4;  // arithmetic shift: rounds towards minus infinity
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (j0 + 3 >= 0 && j0 < S) normals4(philox4x32_10((uint32_t)(j0 >> 2), draw0 + (uint32_t)(c0 + w), purpose, 0u, k0, k1), z);
#pragma unroll
      for (int j = 0; j < 4; ++j) s_src[w][4 * q + j] = (j0 + j >= 0 && j0 + j < S) ? (double)z[j] : 0.0;
    }
    __syncthreads();
    // ---- waves ascending, taps ascending ----
    for (int w = 0; w < nc; ++w) {
      long long fmax = s_first[w * D];
#pragma unroll
      for (int d = 1; d < D; ++d) fmax = max(fmax, (long long)s_first[w * D + d]);
      const long long wstart = ((i0 + P - fmax - (W - 1)) >> 2) * 4;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const long long f = s_first[w * D + d];
        const double* tp = s_tap + (w * D + d) * W;
        if (fmax - f <= NZ_SPAN) {                                      // uniform over the workgroup
          const double* sp = &s_src[w][(int)(i + P - f - wstart)];      // in 0 .. NZ_SW - 1 for every k: see NZ_SW
          double a = acc[d];
#pragma unroll 8
          for (int k = 0; k < W; ++k) a += tp[k] * sp[-k];
          acc[d] = a;
        } else {
          double a = acc[d];
          for (int k = 0; k < W; ++k) {
            const long long j = i + P - f - k;
            double v = 0.0;
            if (j >= 0 && j < S) {
              float z[4];
              normals4(philox4x32_10((uint32_t)(j >> 2), draw0 + (uint32_t)(c0 + w), purpose, 0u, k0, k1), z);
              v = (double)z[j & 3];
            }
            a += tp[k] * v;
          }
          acc[d] = a;
        }
      }
    }
    __syncthreads();                          // the chunk has been read before the next one overwrites it
  }
  if (i < L) {
#pragma unroll
    for (int d = 0; d < D; ++d) out[((long long)b * D + d) * L + i] = (float)(scale * acc[d]);
  }
}

template <int D>
void launch_d(const double* taps, const int* first, const uint32_t* keys, uint32_t purpose, uint32_t draw0, float* out, int B, int N, int W, int P, long long L,
              double scale, hipStream_t st) {
  const unsigned tiles = (unsigned)((L + NZ_T - 1) / NZ_T);
  hipLaunchKernelGGL(noise_bank_kernel<D>, dim3(tiles, (unsigned)B), dim3(NZ_T), 0, st, taps, first, keys, purpose, draw0, out, N, W, P, L, scale);
}

}  // namespace

extern "C" {

int buddy_noise_tile(void) { return NZ_T; }
int buddy_noise_max_taps(void) { return NZ_MAXW; }

int buddy_noise_bank(const double* taps, const int* first, const unsigned* keys, unsigned purpose, unsigned draw0, float* out, int B, int D, int N, int W, int P,
                     long long L, double scale, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_noise_bank: ") + why); return BUDDY_ERR_ARG; };
  if (!taps || !first || !keys || !out) return bad("null pointer");
  if (D < 1 || D > NZ_MAXD) return bad("D must be in 1..8");
  if (N < 1 || N > 4096) return bad("N must be in 1..4096");
  if (W < 1 || W > NZ_MAXW) return bad("W must be in 1..buddy_noise_max_taps()");
  if (P < 0 || P > 4096) return bad("P must be in 0..4096");
  if (B < 1 || L < 1) return bad("B and L must be >= 1");
  if (B > 65535) return bad("B above 65535");
  if (L > (1LL << 33)) return bad("L above 2^33 (a draw's sample index has 34 bits)");
  if (!std::isfinite(scale)) return bad("scale must be finite");
  hipStream_t st = (hipStream_t)stream;
  switch (D) {       // one instantiation per microphone count keeps the accumulators in registers
    case 1: launch_d<1>(taps, first, keys, purpose, draw0, out, B, N, W, P, L, scale, st); break;
    case 2: launch_d<2>(taps, first, keys, purpose, draw0, out, B, N, W, P, L, scale, st); break;
    case 3: launch_d<3>(taps, first, keys, purpose, draw0, out, B, N, W, P, L, scale, st); break;
    case 4: launch_d<4>(taps, first, keys, purpose, draw0, out, B, N, W, P, L, scale, st); break;
    case 5: launch_d<5>(taps, first, keys, purpose, draw0, out, B, N, W, P, L, scale, st); break;
    case 6: launch_d<6>(taps, first, keys, purpose, draw0, out, B, N, W, P, L, scale, st); break;
    case 7: launch_d<7>(taps, first, keys, purpose, draw0, out, B, N, W, P, L, scale, st); break;
    default: launch_d<8>(taps, first, keys, purpose, draw0, out, B, N, W, P, L, scale, st); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string("buddy_noise_bank: kernel launch: ") + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

}  // extern "C"
