// Noise power tracker and spectral post-filter of noisy recordings (buddy_amd/utils/denoise.py; Gerkmann & Hendriks 2012,
// Ephraim & Malah 1984 / 1985; no reference counterpart).  Frames of N = 512 samples at hop H = 128 that overhang both ends of the row by P = N - H
// samples, so that every sample lies in exactly four frames: T(L) = (L - 1 + P) / H + 1, frame t covers samples t H - P .. t H - P + 511, zeros
// outside the row.  Kernels behind the C entries at the end of this file (declared in include/buddy_hip.h):
//
//   spectra       Y[b][t][k], k = 0..256, float2: the 512-point LDS transform of fft512.h of the windowed frame               one wave per frame
//   gains         the tracker and the gain rule: G, sigma^2 (B, ldt, 257) fp32 from Y, the row floor phi and the rule        one thread per (row, bin)
//   inverse       x^_t = Re(inverse transform of G[t] Y[t]) into a workspace (B, ldt, 512) fp32, through the same transform    one wave per frame
//   overlap       out[n] = sum_t w x^_t / sum_t w^2 over the four frames of sample n, t ascending, double, rounded once         one thread per sample
//   stats         snr_est_db, noise_db, att_db and the flag word of a row                                                      one workgroup per row
//
// The only fp32 stages are the window product, the product G Y and the two transforms; the tracker, the overlap-add and every sum are double.
//
// gains is LATENCY-BOUND BY CONSTRUCTION: the recursion over the frames is nonlinear (the speech presence probability feeds the noise power that
// the next frame's probability is formed from), so it cannot be scanned; the parallelism is 257 B threads and T dependent steps of a few dozen
// double operations, one exp and -- for the log-spectral-amplitude rule -- one exponential integral each.  Workgroups are one wave of 64 bins, so
// that a batch of B rows spreads over 5 B compute units, and the bins of the next four frames are loaded while the current four are worked on.
// No rate is claimed for it; it runs once per file.
//
// Rows are ragged inside a common stride; lengths are a device array, checked by the C entries.  Nothing behind a row's end is read, nothing
// outside the declared extents is written, every sum has a fixed order, there are no atomics, and a row's bits do not depend on its batch.
#include "../../include/buddy_hip.h"
#include "common.h"
#include "net.h"
#include "fft512.h"
#include "reduce.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace buddy;

namespace {

constexpr int DN_N = FFT_N, DN_H = 128, DN_P = DN_N - DN_H;
constexpr int DN_BINS = FFT_N / 2 + 1;        // 257
constexpr int DN_GT = 64;                     // threads per workgroup of the tracker: one wave
constexpr int DN_PF = 4;                      // frames loaded ahead
constexpr int DN_ZERO = 1, DN_SHORT = 2, DN_NO_SPEECH = 4;
constexpr double DN_XI1 = 31.622776601683793;                 // 10^1.5: the a-priori SNR under the speech hypothesis
constexpr double DN_XI_MIN = 0.0031622776601683794;           // 10^-2.5
constexpr double DN_EULER = 0.5772156649015328606;

template <typename T>
__host__ __device__ __forceinline__ T dn_frames(T len) { return (len - 1 + DN_P) / DN_H + 1; }

__device__ __forceinline__ double dn_power(float2 y) { return (double)y.x * (double)y.x + (double)y.y * (double)y.y; }

// ---- spectra -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FFT_NT) void dn_spectra_kernel(const float* __restrict__ x, const int* __restrict__ lens, long long ld, float2* __restrict__ Y,
                                                            long long ldt) {
  __shared__ FftLds s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
  const long long L = lens[b], T = dn_frames(L);
  const long long t = (long long)blockIdx.x * FFT_NW + wv;
  fft_tables(s, tid, DN_N);
  frame_load_clipped(s, wv, lane, x + (long long)b * ld, t * DN_H - DN_P, L, t < T);        // reads indices in [0, L) only
  const float2* X = frame_fft(s, wv, lane);
  if (t >= T) return;
  float2* o = Y + ((long long)b * ldt + t) * DN_BINS;
  for (int k = lane; k < DN_BINS; k += 64) o[k] = X[k];
}

// ---- tracker and gain rule ---------------------------------------------------------------------------------------------------------------------
// E1(x) = int_x^inf exp(-u) / u du, x > 0, double: the power series -gamma - ln x - sum_{n >= 1} (-x)^n / (n n!) below 1, the continued fraction
// exp(-x) / (x + 1 - 1 / (x + 3 - 4 / (x + 5 - ...))) by the modified Lentz recurrence from 1 on
__device__ double dn_expint_e1(double x) {
  if (x < 1.0) {
    double sum = 0.0, term = 1.0;
    for (int n = 1; n <= 40; ++n) {
      term *= -x / (double)n;
      const double d = term / (double)n;
      sum += d;
      if (fabs(d) <= 1e-17 * fabs(sum)) break;
    }
    return -DN_EULER - log(x) - sum;
  }
  double bq = x + 1.0, c = 1e300, d = 1.0 / bq, h = d;
  for (int i = 1; i <= 300; ++i) {
    const double an = -(double)i * (double)i;
    bq += 2.0;
    d = 1.0 / (an * d + bq);
    c = bq + an / c;
    const double del = c * d;
    h *= del;
    if (fabs(del - 1.0) <= 3e-16) break;
  }
  return h * exp(-x);
}

struct DnState { double sig, pbar, a2; };

// one frame of one bin: DESIGN.md section 27, steps 1..9
__device__ __forceinline__ void dn_step(DnState& st, double pw, double phi, int rule, double gmin, float* g_out, float* s_out) {
  double p = 1.0 / (1.0 + (1.0 + DN_XI1) * exp(-(pw / st.sig) * (DN_XI1 / (1.0 + DN_XI1))));
  st.pbar = 0.9 * st.pbar + 0.1 * p;
  if (st.pbar > 0.99) p = fmin(p, 0.99);
  st.sig = fmax(0.8 * st.sig + 0.2 * (p * st.sig + (1.0 - p) * pw), phi);
  const double gam = fmin(fmax(pw / st.sig, 1e-6), 1e3);
  const double xi = fmax(0.98 * st.a2 / st.sig + 0.02 * fmax(gam - 1.0, 0.0), DN_XI_MIN);
  const double a = xi / (1.0 + xi);
  double g = a;
  if (rule == 1) g = fmin(a * exp(0.5 * dn_expint_e1(a * gam)), 1.0);
  g = fmax(g, gmin);
  st.a2 = g * g * pw;
  *g_out = (float)g;
  *s_out = (float)st.sig;
}

__global__ __launch_bounds__(DN_GT) void dn_gains_kernel(const float2* __restrict__ Y, const int* __restrict__ lens, const double* __restrict__ phi, int rule,
                                                         double gmin, float* __restrict__ G, float* __restrict__ S2, long long ldt) {
  const int b = blockIdx.y, k = blockIdx.x * DN_GT + threadIdx.x;
  if (k >= DN_BINS) return;
  const long long L = lens[b], T = dn_frames(L);
  const float2* y = Y + (long long)b * ldt * DN_BINS + k;
  float* g = G + (long long)b * ldt * DN_BINS + k;
  float* s2 = S2 + (long long)b * ldt * DN_BINS + k;
  const double ph = phi[b];
  if (!(ph > 0.0)) {                                           // an all-zero row: unit gain, no noise
    for (long long t = 0; t < T; ++t) { g[t * DN_BINS] = 1.f; s2[t * DN_BINS] = 0.f; }
    return;
  }
  // the start: the mean power of the first full frames (t >= 3), at most 8 of them; of all frames where none is full
  const long long full = frames_of(L, DN_N, DN_H);
  const long long t0 = full ? DN_P / DN_H : 0, n0 = full ? (full < 8 ? full : 8) : T;
  double acc = 0.0;
  for (long long t = t0; t < t0 + n0; ++t) acc += dn_power(y[t * DN_BINS]);
  DnState st = {fmax(acc / (double)n0, ph), 0.5, 0.0};
  float2 cur[DN_PF], nxt[DN_PF];
#pragma unroll
  for (int j = 0; j < DN_PF; ++j) cur[j] = j < T ? y[(long long)j * DN_BINS] : make_float2(0.f, 0.f);
  for (long long t = 0; t < T; t += DN_PF) {
#pragma unroll
    for (int j = 0; j < DN_PF; ++j) nxt[j] = t + DN_PF + j < T ? y[(t + DN_PF + j) * DN_BINS] : make_float2(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < DN_PF; ++j)
      if (t + j < T) dn_step(st, dn_power(cur[j]), ph, rule, gmin, g + (t + j) * DN_BINS, s2 + (t + j) * DN_BINS);
#pragma unroll
    for (int j = 0; j < DN_PF; ++j) cur[j] = nxt[j];
  }
}

// ---- synthesis ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FFT_NT) void dn_inverse_kernel(const float2* __restrict__ Y, const float* __restrict__ G, const int* __restrict__ lens, long long ldt,
                                                            float* __restrict__ ws) {
  __shared__ FftLds s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
  const long long T = dn_frames((long long)lens[b]);
  const long long t = (long long)blockIdx.x * FFT_NW + wv;
  const bool live = t < T;
  fft_tables(s, tid, DN_N);
  const long long at = ((long long)b * ldt + t) * DN_BINS;
  spectrum_load_hermitian(s, wv, lane, live ? Y + at : nullptr, live ? G + at : nullptr);
  const float2* X = frame_fft(s, wv, lane);
  if (!live) return;
  float* o = ws + ((long long)b * ldt + t) * DN_N;
#pragma unroll
  for (int i = 0; i < DN_N / 64; ++i) o[lane + 64 * i] = X[lane + 64 * i].x * (1.f / (float)DN_N);
}

__global__ __launch_bounds__(256) void dn_overlap_kernel(const float* __restrict__ ws, const int* __restrict__ lens, long long ldt, float* __restrict__ out,
                                                         long long ld) {
  __shared__ double w[DN_N];
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int i = tid; i < DN_N; i += 256) w[i] = fft_window_d(i, DN_N);
  __syncthreads();
  const long long n = (long long)blockIdx.x * 256 + tid;
  if (n >= lens[b]) return;
  const long long thi = (n + DN_P) / DN_H;                     // the last frame that covers n; thi - 3 >= 0 is the first, thi <= T - 1
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int j = 3; j >= 0; --j) {                               // t ascending
    const long long t = thi - j;
    const int i = (int)(n - (t * DN_H - DN_P));                // 0..511
    num += w[i] * (double)ws[((long long)b * ldt + t) * DN_N + i];
    den += w[i] * w[i];
  }
  out[(long long)b * ld + n] = (float)(num / den);
}

// ---- row statistics ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dn_stats_kernel(const float* __restrict__ x, const float* __restrict__ out, const int* __restrict__ lens, long long ld,
                                                       const float2* __restrict__ Y, const float* __restrict__ S2, long long ldt, double* __restrict__ stats) {
  __shared__ double red[4][4];
  const int tid = threadIdx.x, b = blockIdx.x;
  const long long L = lens[b], T = dn_frames(L), cells = T * DN_BINS;
  const float2* y = Y + (long long)b * ldt * DN_BINS;
  const float* s2 = S2 + (long long)b * ldt * DN_BINS;
  double v[4] = {0.0, 0.0, 0.0, 0.0};         // sum max(|Y|^2 - sigma^2, 0), sum sigma^2, sum x^2, sum out^2
  for (long long i = tid; i < cells; i += 256) {
    const double sg = (double)s2[i];
    v[0] += fmax(dn_power(y[i]) - sg, 0.0);
    v[1] += sg;
  }
  const float* xr = x + (long long)b * ld;
  const float* orow = out + (long long)b * ld;
  for (long long i = tid; i < L; i += 256) {
    const double xv = (double)xr[i], ov = (double)orow[i];
    v[2] += xv * xv;
    v[3] += ov * ov;
  }
  block_sum<4>(v, red, tid);
  if (tid != 0) return;
  double w2 = 0.0;
  for (int i = 0; i < DN_N; ++i) { const double w = fft_window_d(i, DN_N); w2 += w * w; }
  int flags = 0;
  if (L < DN_N) flags |= DN_SHORT;
  double* o = stats + 4LL * b;
  if (!(v[2] > 0.0)) {
    flags |= DN_ZERO;
    o[0] = o[1] = o[2] = __builtin_nan("");
  } else {
    if (!(v[0] > 0.0)) flags |= DN_NO_SPEECH;
    o[0] = 10.0 * log10(v[0] / v[1]);         // -inf with NO_SPEECH
    o[1] = 10.0 * log10(v[1] / (double)cells / w2);
    o[2] = 10.0 * log10(v[2] / v[3]);         // +inf where the output is silent
  }
  o[3] = (double)flags;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------
// a small device array copied to the host once (after the work queued on the stream), so that a bad value is refused before anything is launched;
// on a host without a HIP device no device pointer exists and the array is read where it lies
template <typename T>
int fetch(const T* dev, int n, std::vector<T>& host, void* stream, const char* who) {
  host.resize(n);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    std::memcpy(host.data(), dev, sizeof(T) * (size_t)n);
    return BUDDY_OK;
  }
  hipError_t e = hipMemcpyAsync(host.data(), dev, sizeof(T) * (size_t)n, hipMemcpyDefault, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) { set_error(std::string(who) + ": reading a device array: " + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

// B, the lengths (each in 1..2^30), the sample stride where the entry has one (ld = -1: none) and the frame stride; *longest, *most: the longest row, its frames
int check(const char* who, const int* lens, int B, long long ld, long long ldt, void* stream, long long* longest, long long* most) {
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (B < 1 || B > 65535) return bad("B must be in 1..65535");
  std::vector<int> len;
  if (int rc = fetch(lens, B, len, stream, who)) return rc;
  *longest = 0;
  for (int b = 0; b < B; ++b) {
    if (len[b] < 1 || len[b] > (1 << 30)) return bad("every length must be in 1..2^30");
    *longest = len[b] > *longest ? len[b] : *longest;
  }
  *most = dn_frames(*longest);
  if (ld >= 0 && ld < *longest) return bad("the row stride is smaller than the longest row");
  if (ldt < *most) return bad("ldt is smaller than the frames of the longest row");
  return BUDDY_OK;
}

int finish(const char* who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string(who) + ": kernel launch: " + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

}  // namespace

extern "C" {

long long buddy_denoise_frames(long long L) { return L >= 1 && L <= (1LL << 30) ? dn_frames(L) : -1; }

int buddy_denoise_spectra(const float* x, const int* lens, int B, long long ld, float* Y, long long ldt, void* stream) {
  const char* who = "buddy_denoise_spectra";
  if (!x || !lens || !Y) { set_error(std::string(who) + ": null pointer"); return BUDDY_ERR_ARG; }
  long long longest, most;
  if (int rc = check(who, lens, B, ld, ldt, stream, &longest, &most)) return rc;
  hipLaunchKernelGGL(dn_spectra_kernel, dim3(tiles_of(most, FFT_NW), (unsigned)B), dim3(FFT_NT), 0, (hipStream_t)stream, x, lens, ld, (float2*)Y, ldt);
  return finish(who);
}

int buddy_denoise_gains(const float* Y, const int* lens, const double* phi, int B, long long ldt, int rule, double g_min, float* G, float* sigma2, void* stream) {
  const char* who = "buddy_denoise_gains";
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (!Y || !lens || !phi || !G || !sigma2) return bad("null pointer");
  if (rule != 0 && rule != 1) return bad("the gain rule must be 0 (wiener) or 1 (lsa)");
  if (!(g_min > 0.0) || !(g_min <= 1.0)) return bad("g_min must be in (0, 1]");
  long long longest, most;
  if (int rc = check(who, lens, B, -1, ldt, stream, &longest, &most)) return rc;
  std::vector<double> ph;
  if (int rc = fetch(phi, B, ph, stream, who)) return rc;
  for (int b = 0; b < B; ++b)
    if (!std::isfinite(ph[b]) || ph[b] < 0.0) return bad("every phi[b] must be finite and >= 0 (0: an all-zero row)");
  hipLaunchKernelGGL(dn_gains_kernel, dim3(tiles_of(DN_BINS, DN_GT), (unsigned)B), dim3(DN_GT), 0, (hipStream_t)stream, (const float2*)Y, lens, phi, rule, g_min, G,
                     sigma2, ldt);
  return finish(who);
}

long long buddy_denoise_synthesis_workspace(int B, long long ldt) {
  if (B < 1 || B > 65535 || ldt < 1 || ldt > (1LL << 24)) return -1;
  return 4LL * B * ldt * DN_N;
}

int buddy_denoise_synthesis(const float* Y, const float* G, const int* lens, int B, long long ldt, float* out, long long ld, void* ws, long long ws_bytes,
                            void* stream) {
  const char* who = "buddy_denoise_synthesis";
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (!Y || !G || !lens || !out || !ws) return bad("null pointer");
  long long longest, most;
  if (int rc = check(who, lens, B, ld, ldt, stream, &longest, &most)) return rc;
  const long long need = buddy_denoise_synthesis_workspace(B, ldt);
  if (need < 0 || ws_bytes < need) return bad("the workspace is smaller than buddy_denoise_synthesis_workspace(B, ldt)");
  hipLaunchKernelGGL(dn_inverse_kernel, dim3(tiles_of(most, FFT_NW), (unsigned)B), dim3(FFT_NT), 0, (hipStream_t)stream, (const float2*)Y, G, lens, ldt, (float*)ws);
  hipLaunchKernelGGL(dn_overlap_kernel, dim3(tiles_of(longest, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, (const float*)ws, lens, ldt, out, ld);
  return finish(who);
}

int buddy_denoise_stats(const float* x, const float* out, const int* lens, int B, long long ld, const float* Y, const float* sigma2, long long ldt, double* stats,
                        void* stream) {
  const char* who = "buddy_denoise_stats";
  if (!x || !out || !lens || !Y || !sigma2 || !stats) { set_error(std::string(who) + ": null pointer"); return BUDDY_ERR_ARG; }
  long long longest, most;
  if (int rc = check(who, lens, B, ld, ldt, stream, &longest, &most)) return rc;
  hipLaunchKernelGGL(dn_stats_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, x, out, lens, ld, (const float2*)Y, sigma2, ldt, stats);
  return finish(who);
}

}  // extern "C"
