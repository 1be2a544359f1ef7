// The frame FFT of the evaluation kernels (metrics.hip, spectral.hip): a radix-2 Stockham transform of 512 complex points in LDS, one wave per
// transform, 4 butterflies per lane and stage, two buffers of 512 float2 per wave, four waves per workgroup.  Reads of a stage are consecutive
// 8-byte words (conflict-free); the writes of the first stages have a stride of 2 Ns words and run at half rate (2-way conflicts), which nine stages
// of four instructions do not repay removing.  The stages are separated by workgroup barriers, so every wave of a workgroup runs the transform, also
// when its frame lies past the row's end (its input is then zero and nothing is stored).
//
// The frame is `frame` <= 512 samples under the window w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / (frame + 1)), the interior of a Hann window of frame + 2
// points, zero-padded to 512.  The window is rounded to fp32 from double and the product w x is one fp32 multiplication.
#pragma once
#include "common.h"

namespace buddy {
constexpr int FFT_NT = 256;                   // threads per workgroup of a kernel that runs the transform
constexpr int FFT_NW = FFT_NT / 64;           // waves, one transform each
constexpr int FFT_N = 512;

__device__ __forceinline__ double fft_window_d(int i, int frame) { return 0.5 - 0.5 * cospi(2.0 * (double)(i + 1) / (double)(frame + 1)); }

struct FftLds {
  float2 buf[FFT_NW][2][FFT_N];               // 32 KB
  float2 tw[FFT_N / 2];                       // exp(-2 pi i t / 512)
  float win[FFT_N];                           // the first `frame` values are set
};

__device__ __forceinline__ void fft_tables(FftLds& s, int tid, int frame) {      // 256 threads: one twiddle each and the window, from double
  double sn, cs;
  sincospi(-2.0 * (double)tid / (double)FFT_N, &sn, &cs);
  s.tw[tid] = make_float2((float)cs, (float)sn);
  for (int i = tid; i < frame; i += FFT_NT) s.win[i] = (float)fft_window_d(i, frame);
  __syncthreads();
}

// the windowed frame at xf (nullptr: zeros), zero-padded to 512, into buffer 0 of wave wv
__device__ __forceinline__ void frame_load(FftLds& s, int wv, int lane, const float* xf, int frame) {
#pragma unroll
  for (int i = 0; i < FFT_N / 64; ++i) {
    const int n = lane + 64 * i;
    s.buf[wv][0][n] = make_float2(xf && n < frame ? __fmul_rn(s.win[n], xf[n]) : 0.f, 0.f);
  }
}

// in: buffer 0 of wave wv, written by this wave.  Returns the buffer that holds the spectrum in natural order (nine stages: buffer 1).  Every wave of
// the workgroup must call it (barriers); the result may be read after it returns
__device__ __forceinline__ const float2* frame_fft(FftLds& s, int wv, int lane) {
  int cur = 0;
  for (int Ns = 1; Ns < FFT_N; Ns <<= 1, cur ^= 1) {
    __syncthreads();
    const float2* in = s.buf[wv][cur];
    float2* out = s.buf[wv][cur ^ 1];
    const int tstep = (FFT_N / 2) / Ns;
#pragma unroll
    for (int i = 0; i < FFT_N / 2 / 64; ++i) {
      const int j = lane + 64 * i, k = j & (Ns - 1);
      const float2 w = s.tw[k * tstep], v0 = in[j], u = in[j + FFT_N / 2];
      const float2 v1 = make_float2(u.x * w.x - u.y * w.y, u.x * w.y + u.y * w.x);
      const int j0 = ((j - k) << 1) + k;
      out[j0] = make_float2(v0.x + v1.x, v0.y + v1.y);
      out[j0 + Ns] = make_float2(v0.x - v1.x, v0.y - v1.y);
    }
  }
  __syncthreads();
  return s.buf[wv][cur];
}
}  // namespace buddy
