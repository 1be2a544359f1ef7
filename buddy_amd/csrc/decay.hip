// Blind decay time of single signals (buddy_amd/utils/decay.py; no reference counterpart: the reference scores nothing).  Definitions in DESIGN.md
// section 30 (the free-decay-region family: Prego, de Lima, Netto & Lee 2012; Loellmann et al. 2010, restated there with every constant fixed).
// Kernels behind the C entries of include/buddy_hip.h:
//
//   decay_energies   E[b][band][m] = sum of |X[k]|^2 over the band's bins, X the 512-point transform of fft512.h of frame m (hop 128)   one wave per frame
//   decay_regions    S = the sum of K consecutive E, its maximum, and for every frame at which a run of steps down starts the run's
//                    length and the decay time of its least-squares slope                                                                one workgroup per (row, band)
//   decay_select     the number of kept regions of a (row, band) and the lower median and the quartiles of their decay times            one workgroup per (row, band, rank)
//
// Rows are ragged inside a common stride; lengths and frame counts are device arrays, checked by the C entries.  Nothing behind a row's end is read,
// nothing outside the declared extents is written.  Every sum runs in a fixed order in double and there are no floating-point atomics (the select
// counts with integer LDS atomics, whose result has no order), so a row's result does not depend on its batch.  All of it runs once per tester
// mode, after sampling: latency-bound, written for clarity.
//
// decay_regions writes DENSE output: T[m] is the decay time of the region that starts at frame m, NaN where none does, so a region list's order is its
// frame order with no slot counter.  A workgroup walks its row in tiles of DK_TILE frames; a tile's S, one frame before it and DK_HALO frames behind it
// lie in LDS.  Thread i decides whether a region starts at frame base + i (a step down here and none one frame earlier) and then walks the region
// itself; S beyond the LDS window is summed from E in global memory by the same function that filled the window, so it has the same bits.
#include "common.h"
#include "fft512.h"
#include "reduce.h"
#include "select.h"

namespace buddy {
namespace {
constexpr int DK_HOP = 128;                   // frames of FFT_N = 512 samples at this hop, at 16 kHz
constexpr int DK_FS = 16000;
constexpr int DK_MAXB = 8, DK_MAXK = 8;
constexpr int DK_NBIN = FFT_N / 2 + 1;
constexpr int DK_TILE = 256, DK_HALO = 256;
constexpr int DK_WIN = 1 + DK_TILE + DK_HALO; // S of frames base - 1 .. base + DK_TILE + DK_HALO - 1

struct DkBands { int lo[DK_MAXB], hi[DK_MAXB]; };

__global__ __launch_bounds__(FFT_NT) void decay_energies_kernel(const float* __restrict__ x, const int* __restrict__ lens, long long ld, DkBands bands, int NB,
                                                                double* __restrict__ E, long long ldm, int* __restrict__ frames) {
  __shared__ FftLds s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
  const int M = frames_of(lens[b], FFT_N, DK_HOP);
  if (blockIdx.x == 0 && tid == 0) frames[b] = M;
  const long long f = (long long)blockIdx.x * FFT_NW + wv;
  fft_tables(s, tid, FFT_N);
  frame_load(s, wv, lane, f < M ? x + (long long)b * ld + f * DK_HOP : nullptr, FFT_N);     // the last sample read is (M - 1) hop + 511 < lens[b]
  const float2* X = frame_fft(s, wv, lane);
  if (f >= M || lane >= NB) return;
  double acc = 0.0;                           // lane = band: its bins in ascending order, one accumulator
  for (int k = bands.lo[lane]; k < bands.hi[lane]; ++k) {
    const double re = (double)X[k].x, im = (double)X[k].y;
    acc += re * re + im * im;                 // the squares of fp32 values are exact in double
  }
  E[((long long)b * NB + lane) * ldm + f] = acc;
}

// S[m] = (((E[m] + E[m + 1]) + E[m + 2]) + ...) + E[m + K - 1], m + K <= frames
__device__ __forceinline__ double smoothed(const double* __restrict__ Er, int m, int K) {
  double v = Er[m];
  for (int i = 1; i < K; ++i) v = __dadd_rn(v, Er[m + i]);
  return v;
}

__global__ __launch_bounds__(DK_TILE) void decay_regions_kernel(const double* __restrict__ E, const int* __restrict__ frames, int NB, long long ldm, int K,
                                                                int lmin, double q, double floor_rel, double* __restrict__ T, int* __restrict__ len) {
  __shared__ double sS[DK_WIN];
  __shared__ double red[DK_TILE / 64];
  const int tid = threadIdx.x, band = blockIdx.x, b = blockIdx.y;
  const int M = frames[b];
  const long long row = ((long long)b * NB + band) * ldm;
  const double* Er = E + row;
  const int Ms = M >= K ? M - K + 1 : 0;      // S[0 .. Ms - 1]
  double mx = 0.0;
  for (int m = tid; m < Ms; m += DK_TILE) mx = fmax(mx, smoothed(Er, m, K));
  mx = block_max(mx, red, tid);
  const double floor = __dmul_rn(floor_rel, mx);
  const double nan = __builtin_nan("");
  for (int base = 0; base < M; base += DK_TILE) {
    __syncthreads();                          // the previous tile has been walked
    for (int i = tid; i < DK_WIN; i += DK_TILE) {
      const int m = base - 1 + i;
      sS[i] = (m >= 0 && m < Ms) ? smoothed(Er, m, K) : 0.0;
    }
    __syncthreads();
    const int m0 = base + tid;
    if (m0 >= M) continue;                    // the barriers above are reached by every thread: the loop bound is uniform
    auto S = [&](int m) {                     // base - 1 <= m < Ms
      const int i = m - base + 1;
      return i < DK_WIN ? sS[i] : smoothed(Er, m, K);
    };
    auto step = [&](int m) {                  // 0 <= m, m + 1 < Ms: frame m steps down
      const double a = S(m), c = S(m + 1);
      return c < a && c > floor;
    };
    double t = nan;
    int n = 0;
    if (m0 + 1 < Ms && step(m0) && !(m0 > 0 && step(m0 - 1))) {
      const double s0 = S(m0);
      double prev = s0, sj = 0.0, sjj = 0.0, sd = 0.0, sjd = 0.0;      // the terms of j = 0 are all zero
      int m1 = m0;
      while (m1 + 1 < Ms) {
        const double c = S(m1 + 1);
        if (!(c < prev && c > floor)) break;
        ++m1;
        const double j = (double)(m1 - m0), d = __dmul_rn(10.0, log10(c / s0));
        sj = __dadd_rn(sj, j);
        sjj = __dadd_rn(sjj, __dmul_rn(j, j));
        sd = __dadd_rn(sd, d);
        sjd = __dadd_rn(sjd, __dmul_rn(j, d));
        prev = c;
      }
      const int cnt = m1 - m0 + 1;
      if (cnt >= lmin && s0 > floor && prev <= __dmul_rn(s0, q)) {
        const double nn = (double)cnt;
        const double num = __dsub_rn(__dmul_rn(nn, sjd), __dmul_rn(sj, sd)), den = __dsub_rn(__dmul_rn(nn, sjj), __dmul_rn(sj, sj));
        const double slope = num / den;
        if (slope < 0.0) {                    // a run of steps down has a negative slope; checked all the same
          t = __dmul_rn(-60.0 / slope, (double)DK_HOP) / (double)DK_FS;
          n = cnt;
        }
      }
    }
    T[row + m0] = t;
    len[row + m0] = n;
  }
}

__global__ __launch_bounds__(SEL_T) void decay_select_kernel(const double* __restrict__ T, const int* __restrict__ frames, int NB, long long ldm,
                                                             double* __restrict__ out, int* __restrict__ counts) {
  __shared__ unsigned hist[256];
  __shared__ unsigned ws[SEL_T / 64];
  __shared__ unsigned pick[2];
  const int rb = blockIdx.x, which = blockIdx.y, tid = threadIdx.x;
  const int M = frames[rb / NB];
  const double* row = T + (long long)rb * ldm;
  unsigned mine = 0, n = 0;
  for (int m = tid; m < M; m += SEL_T) mine += row[m] == row[m] ? 1u : 0u;
  block_excl_scan(mine, ws, tid, &n);
  if (which == 0 && tid == 0) counts[rb] = (int)n;
  double v = __builtin_nan("");
  if (n > 0) {                                // uniform over the workgroup
    const unsigned rank = which == 0 ? (n - 1) / 2 : which == 1 ? (n - 1) / 4 : 3 * (n - 1) / 4;
    v = radix_select<true>(row, M, rank, hist, ws, pick, tid);
  }
  if (tid == 0) out[(long long)rb * 3 + which] = v;
}
}  // namespace

int decay_regions_tile() { return DK_TILE; }
int decay_frame() { return FFT_N; }
int decay_hop() { return DK_HOP; }
int decay_bins() { return DK_NBIN; }

void launch_decay_energies(const float* x, const int* lens, int B, long long ld, long long max_frames, const int* lo, const int* hi, int NB, double* E, long long ldm,
                           int* frames, hipStream_t st) {
  DkBands bands;
  for (int i = 0; i < DK_MAXB; ++i) { bands.lo[i] = i < NB ? lo[i] : 0; bands.hi[i] = i < NB ? hi[i] : 0; }
  const unsigned tiles = max_frames >= 1 ? tiles_of(max_frames, FFT_NW) : 1u;       // a call without a full frame still writes the frame counts
  hipLaunchKernelGGL(decay_energies_kernel, dim3(tiles, (unsigned)B), dim3(FFT_NT), 0, st, x, lens, ld, bands, NB, E, ldm, frames);
}

void launch_decay_regions(const double* E, const int* frames, int B, int NB, long long ldm, int K, int lmin, double q, double floor_rel, double* T, int* len,
                          hipStream_t st) {
  hipLaunchKernelGGL(decay_regions_kernel, dim3((unsigned)NB, (unsigned)B), dim3(DK_TILE), 0, st, E, frames, NB, ldm, K, lmin, q, floor_rel, T, len);
}

void launch_decay_select(const double* T, const int* frames, int B, int NB, long long ldm, double* out, int* counts, hipStream_t st) {
  hipLaunchKernelGGL(decay_select_kernel, dim3((unsigned)(B * NB), 3u), dim3(SEL_T), 0, st, T, frames, NB, ldm, out, counts);
}

}  // namespace buddy
