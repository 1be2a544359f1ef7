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

// the windowed frame of 512 samples row[start .. start + 511] of a row of len samples, zeros where the index leaves [0, len), into buffer 0 of wave
// wv (denoise.hip: frames that overhang both ends of the row; the tables must have been made for frame = 512).  live = false: zeros
__device__ __forceinline__ void frame_load_clipped(FftLds& s, int wv, int lane, const float* row, long long start, long long len, bool live) {
#pragma unroll
  for (int i = 0; i < FFT_N / 64; ++i) {
    const int n = lane + 64 * i;
    const long long j = start + n;
    s.buf[wv][0][n] = make_float2(live && j >= 0 && j < len ? __fmul_rn(s.win[n], row[j]) : 0.f, 0.f);
  }
}

// the conjugate of the Hermitian spectrum Z[k] = g[k] Y[k], k = 0..256, Z[512 - k] = conj(Z[k]), into buffer 0 of wave wv: frame_fft of it is
// 512 conj(z), z the inverse transform of Z, so Re(result) / 512 is the real signal (the imaginary parts of bins 0 and 256 fall out of the real part,
// as in any real inverse transform).  Each product is one fp32 multiplication.  Y, g null: zeros
__device__ __forceinline__ void spectrum_load_hermitian(FftLds& s, int wv, int lane, const float2* Y, const float* g) {
#pragma unroll
  for (int i = 0; i < FFT_N / 64; ++i) {
    const int n = lane + 64 * i, k = n <= FFT_N / 2 ? n : FFT_N - n;     // every lane writes its own eight points
    float2 v = make_float2(0.f, 0.f);
    if (Y) {
      const float2 y = Y[k];
      const float re = __fmul_rn(g[k], y.x), im = __fmul_rn(g[k], y.y);
      v = make_float2(re, n <= FFT_N / 2 ? -im : im);
    }
    s.buf[wv][0][n] = v;
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
