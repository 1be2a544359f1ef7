// Spectral-envelope distortion of a paired run (buddy_amd/utils/spectral.py; no reference counterpart).  Definitions in DESIGN.md section 21: cepstral
// distance, log-likelihood ratio and frequency-weighted segmental SNR per pair (estimate e, clean reference x) at 16 kHz.  Kernels behind the C
// entries of include/buddy_hip.h:
//
//   frame_spectra    |X[k]|, k = 0..256, fp32, of every full windowed frame: the 512-point LDS FFT of fft512.h           one wave per frame
//   cepstra          25 real-cepstrum coefficients of both signals from given spectra, double, cosine table in LDS        one wave per frame
//   cd_rows          coefficient means over the frames, the frame distances, their mean                                   one workgroup per row
//   fwseg_frames     23 mel-band magnitudes of both signals, band SNRs by comparison, the weighted frame value            one wave per frame
//   llr_frames       2 x (order + 1) lag sums of the windowed frames, Levinson-Durbin, the quadratic forms, double        one wave per frame
//   mean_rows        sum and count of the counted frame values of a row (fwSegSNR, LLR)                                   one workgroup per row
//
// Rows are ragged inside a common stride; lengths and frame counts are device arrays, checked by the C entries.  Nothing behind a row's end is read,
// nothing outside the declared extents is written.  Every reduction runs in a fixed order (strided partial sums, wave shuffles, one LDS exchange;
// per-frame values go through a workspace and are summed by one workgroup per row): no atomics, and a row's result does not depend on its batch.
// All of it runs once per tester mode, after sampling: latency-bound, written for clarity.
//
// The frame FFT lives in fft512.h, the sums (wave_sum, block_sum) and the frame and tile counts (frames_of, tiles_of) in reduce.h.
#include "common.h"
#include "fft512.h"
#include "reduce.h"

namespace buddy {
namespace {
constexpr int SP_NT = FFT_NT;                 // threads per workgroup (4 waves)
constexpr int SP_NW = FFT_NW;
constexpr int NBIN = FFT_N / 2 + 1;           // 257
constexpr int NCEP = 25;                      // cepstral coefficients 0..24
constexpr int MAXORD = 16;
constexpr double DB_PER_NEPER = 4.342944819032518;           // 10 / ln 10

// ---- magnitude spectra -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_NT) void frame_spectra_kernel(const float* __restrict__ x, const int* __restrict__ lens, long long ld, int frame, int hop,
                                                              float* __restrict__ S, long long ldf) {
  __shared__ FftLds s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
  const int F = frames_of(lens[b], frame, hop);
  const long long f = (long long)blockIdx.x * SP_NW + wv;
  fft_tables(s, tid, frame);
  frame_load(s, wv, lane, f < F ? x + (long long)b * ld + f * hop : nullptr, frame);       // the last sample read is (F - 1) hop + frame - 1 < lens[b]
  const float2* X = frame_fft(s, wv, lane);
  if (f >= F) return;
  float* o = S + ((long long)b * ldf + f) * NBIN;
  for (int k = lane; k < NBIN; k += 64) o[k] = (float)sqrt((double)X[k].x * (double)X[k].x + (double)X[k].y * (double)X[k].y);
}

// ---- cepstral distance -------------------------------------------------------------------------------------------------------------------
// c[n] = (1/512) sum_{k = 0..511} L[k] cos(2 pi k n / 512) with L[512 - k] = L[k]: (L[0] + (-1)^n L[256] + 2 sum_{k = 1..255} L[k] cos(2 pi k n / 512)) / 512
__global__ __launch_bounds__(SP_NT) void cepstra_kernel(const float* __restrict__ X, const float* __restrict__ E, const int* __restrict__ frames, long long ldf,
                                                        const double* __restrict__ gain, const double* __restrict__ delta, double* __restrict__ ws, long long ldw) {
  __shared__ double ctab[FFT_N];
  __shared__ double L[SP_NW][2][NBIN];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
  for (int i = tid; i < FFT_N; i += SP_NT) ctab[i] = cospi(2.0 * (double)i / (double)FFT_N);
  const int F = frames[b];
  const long long f = (long long)blockIdx.x * SP_NW + wv;
  const bool live = f < F;
  if (live) {
    const double g = gain[b], d = delta[b];
    const float* xp = X + ((long long)b * ldf + f) * NBIN;
    const float* ep = E + ((long long)b * ldf + f) * NBIN;
    for (int k = lane; k < NBIN; k += 64) {
      const double xv = (double)xp[k], ev = g * (double)ep[k];
      L[wv][0][k] = 0.5 * log(xv * xv + d);
      L[wv][1][k] = 0.5 * log(ev * ev + d);
    }
  }
  __syncthreads();
  if (!live) return;
  double* o = ws + ((long long)b * ldw + f) * (2 * NCEP);
  for (int q = 0; q < 2; ++q) {
    const double* Lq = L[wv][q];
    for (int n = 0; n < NCEP; ++n) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = lane + 64 * i;                          // 0..255; bin 0 is taken with the edge terms
        if (k >= 1) acc += Lq[k] * ctab[(k * n) & (FFT_N - 1)];
      }
      acc = wave_sum(acc);
      if (lane == 0) o[q * NCEP + n] = (Lq[0] + ((n & 1) ? -Lq[FFT_N / 2] : Lq[FFT_N / 2]) + 2.0 * acc) / (double)FFT_N;
    }
  }
}

__global__ __launch_bounds__(SP_NT) void cd_rows_kernel(const double* __restrict__ ws, long long ldw, const int* __restrict__ frames, const double* __restrict__ delta,
                                                        double* __restrict__ out, int* __restrict__ flags) {
  __shared__ double red[SP_NW][5];
  __shared__ double mean[2 * NCEP];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int F = frames[b];
  const double* c = ws + (long long)b * ldw * (2 * NCEP);
  for (int q0 = 0; q0 < 2 * NCEP; q0 += 5) {                 // the means of the 50 coefficients, five at a time
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int f = tid; f < F; f += SP_NT)
#pragma unroll
      for (int q = 0; q < 5; ++q) v[q] += c[(long long)f * (2 * NCEP) + q0 + q];
    block_sum<5>(v, red, tid);
    if (tid == 0)
#pragma unroll
      for (int q = 0; q < 5; ++q) mean[q0 + q] = v[q] / (double)F;
  }
  __syncthreads();
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int f = tid; f < F; f += SP_NT) {
    const double* cf = c + (long long)f * (2 * NCEP);
    double acc = 0.0;
    for (int n = 0; n < NCEP; ++n) {
      const double dc = (cf[n] - mean[n]) - (cf[NCEP + n] - mean[NCEP + n]);
      acc += (n ? 2.0 : 1.0) * dc * dc;
    }
    s[0] += fmin(fmax(DB_PER_NEPER * sqrt(acc), 0.0), 10.0);
  }
  block_sum<5>(s, red, tid);
  if (tid != 0) return;
  const bool ok = F >= 1 && delta[b] > 0.0;   // no full frame, or a clean signal without power (a NaN floor compares false)
  out[b] = ok ? s[0] / (double)F : __builtin_nan("");
  flags[b] = ok ? 1 : 0;
}

// ---- frequency-weighted segmental SNR ----------------------------------------------------------------------------------------------------
// lane j < J owns band j: X_j = sum_k M[j][k] |X[k]|, E_j = sum_k M[j][k] g |E[k]|, k ascending, double
__global__ __launch_bounds__(SP_NT) void fwseg_frames_kernel(const float* __restrict__ X, const float* __restrict__ E, const int* __restrict__ frames, long long ldf,
                                                             const double* __restrict__ gain, const double* __restrict__ M, int J, double* __restrict__ ws,
                                                             long long ldw) {
  __shared__ double sx[SP_NW][NBIN], se[SP_NW][NBIN];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
  const int F = frames[b];
  const long long f = (long long)blockIdx.x * SP_NW + wv;
  const bool live = f < F;
  if (live) {
    const double g = gain[b];
    const float* xp = X + ((long long)b * ldf + f) * NBIN;
    const float* ep = E + ((long long)b * ldf + f) * NBIN;
    for (int k = lane; k < NBIN; k += 64) { sx[wv][k] = (double)xp[k]; se[wv][k] = g * (double)ep[k]; }
  }
  __syncthreads();
  if (!live) return;
  double w = 0.0, ws_ = 0.0;
  if (lane < J) {
    const double* Mj = M + (long long)lane * NBIN;
    double xj = 0.0, ej = 0.0;
    for (int k = 0; k < NBIN; ++k) { xj += Mj[k] * sx[wv][k]; ej += Mj[k] * se[wv][k]; }
    const double num = xj * xj, den = (xj - ej) * (xj - ej);
    double snr;
    if (den <= num * 3.1622776601683794e-4) snr = 35.0;       // 10^-3.5: the band SNR is at least 35 dB
    else if (num <= den * 0.1) snr = -10.0;
    else snr = 10.0 * log10(num / den);
    w = pow(xj, 0.2);
    ws_ = w * snr;
  }
  w = wave_sum(w);
  ws_ = wave_sum(ws_);
  if (lane == 0) {
    const bool counted = w > 0.0;
    ws[((long long)b * ldw + f) * 2 + 0] = counted ? ws_ / w : 0.0;
    ws[((long long)b * ldw + f) * 2 + 1] = counted ? 1.0 : 0.0;
  }
}

// ---- log-likelihood ratio ----------------------------------------------------------------------------------------------------------------
// Levinson-Durbin on r[0..p] (r[0] > 0): a[0] = 1, a[1..p] the coefficients of the prediction-error filter.  The recursion stops where the error is
// no longer positive (the remaining coefficients stay zero)
__device__ void levinson(const double* r, int p, double* a) {
  double tmp[MAXORD + 1];
  a[0] = 1.0;
  for (int i = 1; i <= p; ++i) a[i] = 0.0;
  double err = r[0];
  for (int i = 1; i <= p; ++i) {
    if (!(err > 0.0)) break;
    double acc = r[i];
    for (int j = 1; j < i; ++j) acc += a[j] * r[i - j];
    const double k = -acc / err;
    for (int j = 1; j < i; ++j) tmp[j] = a[j] + k * a[i - j];
    for (int j = 1; j < i; ++j) a[j] = tmp[j];
    a[i] = k;
    err *= 1.0 - k * k;
  }
}

__device__ double toeplitz_form(const double* a, const double* r, int p) {       // a R a^T, R[i][j] = r[|i - j|], rows in order
  double s = 0.0;
  for (int i = 0; i <= p; ++i) {
    double t = 0.0;
    for (int j = 0; j <= p; ++j) t += a[j] * r[i > j ? i - j : j - i];
    s += a[i] * t;
  }
  return s;
}

__global__ __launch_bounds__(SP_NT) void llr_frames_kernel(const float* __restrict__ e, const float* __restrict__ x, const int* __restrict__ lens, long long ld,
                                                           int frame, int hop, int order, double* __restrict__ ws, long long ldw) {
  __shared__ double sig[SP_NW][2][FFT_N];
  __shared__ double r[SP_NW][2][MAXORD + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.y;
  const int F = frames_of(lens[b], frame, hop);
  const long long f = (long long)blockIdx.x * SP_NW + wv;
  const bool live = f < F;                    // wave-uniform
  if (live) {
    const float* xf = x + (long long)b * ld + f * hop;        // the last sample read is (F - 1) hop + frame - 1 < lens[b]
    const float* ef = e + (long long)b * ld + f * hop;
    for (int i = lane; i < frame; i += 64) {
      const double w = fft_window_d(i, frame);
      sig[wv][0][i] = w * (double)xf[i];
      sig[wv][1][i] = w * (double)ef[i];
    }
  }
  __syncthreads();
  if (!live) return;                          // from here on a wave works on its own part of the LDS
  for (int q = 0; q < 2; ++q)
    for (int k = 0; k <= order; ++k) {
      double acc = 0.0;
      for (int i = lane; i + k < frame; i += 64) acc += sig[wv][q][i] * sig[wv][q][i + k];
      acc = wave_sum(acc);
      if (lane == 0) r[wv][q][k] = acc;
    }
  if (lane != 0) return;
  double* rx = r[wv][0];
  double* re = r[wv][1];
  const bool counted = rx[0] > 0.0 && re[0] > 0.0;
  double v = 0.0;
  if (counted) {
    rx[0] *= 1.0 + 1e-9;
    re[0] *= 1.0 + 1e-9;
    double ax[MAXORD + 1], ae[MAXORD + 1];
    levinson(rx, order, ax);
    levinson(re, order, ae);
    v = fmin(fmax(log(toeplitz_form(ae, rx, order) / toeplitz_form(ax, rx, order)), 0.0), 2.0);
  }
  ws[((long long)b * ldw + f) * 2 + 0] = v;
  ws[((long long)b * ldw + f) * 2 + 1] = counted ? 1.0 : 0.0;
}

// ws (B, ldw, 2): value and counted (0 or 1) of each frame -> the mean over the counted frames and their number
__global__ __launch_bounds__(SP_NT) void mean_rows_kernel(const double* __restrict__ ws, long long ldw, const int* __restrict__ frames, const int* __restrict__ lens,
                                                          int frame, int hop, double* __restrict__ out, int* __restrict__ counts, int* __restrict__ flags) {
  __shared__ double red[SP_NW][2];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int F = frames ? frames[b] : frames_of(lens[b], frame, hop);
  double v[2] = {0.0, 0.0};
  for (int f = tid; f < F; f += SP_NT) {
    const double c = ws[((long long)b * ldw + f) * 2 + 1];
    if (c > 0.0) { v[0] += ws[((long long)b * ldw + f) * 2 + 0]; v[1] += c; }
  }
  block_sum<2>(v, red, tid);
  if (tid != 0) return;
  const bool ok = v[1] > 0.0;
  out[b] = ok ? v[0] / v[1] : __builtin_nan("");
  counts[b] = (int)v[1];
  flags[b] = ok ? 1 : 0;
}

}  // namespace

int spectral_bins() { return NBIN; }
int spectral_cepstra() { return NCEP; }
int spectral_max_order() { return MAXORD; }

void launch_frame_spectra(const float* x, const int* lens, int B, long long ld, long long max_frames, int frame, int hop, float* S, long long ldf, hipStream_t st) {
  if (max_frames < 1) return;
  hipLaunchKernelGGL(frame_spectra_kernel, dim3(tiles_of(max_frames, SP_NW), (unsigned)B), dim3(SP_NT), 0, st, x, lens, ld, frame, hop, S, ldf);
}

void launch_cepstral_distance(const float* X, const float* E, const int* frames, int B, long long ldf, int max_frames, const double* g, const double* d, double* out,
                              int* flags, double* ws, hipStream_t st) {
  const long long ldw = max_frames > 1 ? max_frames : 1;
  if (max_frames >= 1) hipLaunchKernelGGL(cepstra_kernel, dim3(tiles_of(max_frames, SP_NW), (unsigned)B), dim3(SP_NT), 0, st, X, E, frames, ldf, g, d, ws, ldw);
  hipLaunchKernelGGL(cd_rows_kernel, dim3((unsigned)B), dim3(SP_NT), 0, st, (const double*)ws, ldw, frames, d, out, flags);
}

void launch_fwsegsnr(const float* X, const float* E, const int* frames, int B, long long ldf, int max_frames, const double* g, const double* M, int J, double* out,
                     int* counts, int* flags, double* ws, hipStream_t st) {
  const long long ldw = max_frames > 1 ? max_frames : 1;
  if (max_frames >= 1)
    hipLaunchKernelGGL(fwseg_frames_kernel, dim3(tiles_of(max_frames, SP_NW), (unsigned)B), dim3(SP_NT), 0, st, X, E, frames, ldf, g, M, J, ws, ldw);
  hipLaunchKernelGGL(mean_rows_kernel, dim3((unsigned)B), dim3(SP_NT), 0, st, (const double*)ws, ldw, frames, (const int*)nullptr, 0, 1, out, counts, flags);
}

void launch_llr(const float* e, const float* x, const int* lens, int B, long long ld, long long max_frames, int frame, int hop, int order, double* out, int* counts,
                int* flags, double* ws, hipStream_t st) {
  const long long ldw = max_frames > 1 ? max_frames : 1;
  if (max_frames >= 1)
    hipLaunchKernelGGL(llr_frames_kernel, dim3(tiles_of(max_frames, SP_NW), (unsigned)B), dim3(SP_NT), 0, st, e, x, lens, ld, frame, hop, order, ws, ldw);
  hipLaunchKernelGGL(mean_rows_kernel, dim3((unsigned)B), dim3(SP_NT), 0, st, (const double*)ws, ldw, (const int*)nullptr, lens, frame, hop, out, counts, flags);
}

}  // namespace buddy
