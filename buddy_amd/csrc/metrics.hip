// Objective evaluation of a paired run (buddy_amd/utils/metrics.py; no reference counterpart: the reference writes its wavs and stops there).
// Definitions in DESIGN.md section 17: SI-SDR, STOI (Taal et al. 2011), ESTOI (Jensen & Taal 2016) and the log-spectral distance, per pair
// (estimate e, clean reference x).  Kernels behind the C entries of include/buddy_hip.h:
//
//   pair_moments     means, zero-mean ||e||^2, ||x||^2, <e,x> and SI-SDR in double                     one workgroup per row
//   frame_energy     E[f] = 20 log10(||w x_f|| + eps) of the clean rows, double                          one wave per frame
//   select_scan      per-row maximum, keep mask E[f] > max - 40, exclusive scan -> src[j], K            one workgroup per row
//   gather_ola       rebuilt signals: each output sample sums the at most two kept frames covering it   one thread per sample
//   band_spectra     512-point LDS FFT of a windowed 256-sample frame, third-octave band norms          one wave per frame
//   stoi_segments    the 15 x 30 segment scores in double; stoi_finalize sums them in a fixed order     one wave per (row, segment)
//   frame_power      sum_k |X[k]|^2, k = 0..256, from the windowed frame by Parseval (the LSD floor)     one wave per frame
//   lsd_frames       rms over k of 10 log10((P + d) / (Q + d)); lsd_finalize: the mean over frames      one wave per frame
//
// Rows are ragged inside a common stride; the lengths are device arrays, checked by the C entries.  Nothing behind lens[b] is read, nothing
// outside the declared extents is written.  Every reduction runs in a fixed order (strided partial sums, wave shuffles, one LDS exchange; per-frame
// and per-segment values go through a workspace and are summed by one workgroup per row): no atomics, and a row's result does not depend on
// its batch.  All of it runs once per tester mode, after sampling: latency-bound, written for clarity.
//
// The frame FFT (frame_fft) lives in fft512.h, the sums (wave_sum, block_sum) and the frame and tile counts in reduce.h; spectral.hip uses both too.
#include "common.h"
#include "fft512.h"
#include "reduce.h"

namespace buddy {
namespace {
constexpr int MT_NT = FFT_NT;                 // threads per workgroup (4 waves)
constexpr int MT_NW = FFT_NW;
constexpr int MT_PER = 4;
constexpr int MT_TILE = MT_NT * MT_PER;       // samples per step of the row reductions (buddy_metrics_tile)
constexpr int FR = 256, HOP = 128, NFFT = FFT_N, NBIN = NFFT / 2 + 1, SEG = 30;
constexpr double ST_EPS = 2.220446049250313e-16;          // 2^-52
constexpr int MAXJ = 32;

__device__ __forceinline__ int frames_of(int len) { return buddy::frames_of(len, FR, HOP); }
__device__ __forceinline__ double window_d(int i) { return fft_window_d(i, FR); }            // interior of a 258-point Hann window

// ---- SI-SDR ------------------------------------------------------------------------------------------------------------------------------
// three passes over the row: means; zero-mean moments; with a = <e,x> / max(||x||^2, 1e-30) the target and residual energies, element by element
// as utils.metrics.si_sdr forms them (no fused multiply-add: the residual of a nearly perfect estimate is a difference of nearly equal numbers)
__global__ __launch_bounds__(MT_NT) void pair_moments_kernel(const float* __restrict__ e, const float* __restrict__ x, const int* __restrict__ lens, long long ld,
                                                             double* __restrict__ out, int* __restrict__ flags) {
  __shared__ double red[MT_NW][3];
  const int tid = threadIdx.x, b = blockIdx.x, L = lens[b];
  const float* er = e + (long long)b * ld;
  const float* xr = x + (long long)b * ld;
  double s[3] = {0.0, 0.0, 0.0};
  for (int n = tid; n < L; n += MT_NT) { s[0] += (double)er[n]; s[1] += (double)xr[n]; }
  block_sum<3>(s, red, tid);
  const double me = s[0] / (double)L, mx = s[1] / (double)L;
  double m[3] = {0.0, 0.0, 0.0};
  for (int n = tid; n < L; n += MT_NT) {
    const double ec = __dsub_rn((double)er[n], me), xc = __dsub_rn((double)xr[n], mx);
    m[0] = __dadd_rn(m[0], __dmul_rn(ec, ec));
    m[1] = __dadd_rn(m[1], __dmul_rn(xc, xc));
    m[2] = __dadd_rn(m[2], __dmul_rn(ec, xc));
  }
  block_sum<3>(m, red, tid);
  const double a = m[2] / fmax(m[1], 1e-30);
  double r[3] = {0.0, 0.0, 0.0};
  for (int n = tid; n < L; n += MT_NT) {
    const double ec = __dsub_rn((double)er[n], me), xc = __dsub_rn((double)xr[n], mx);
    const double t = __dmul_rn(a, xc), d = __dsub_rn(t, ec);
    r[0] = __dadd_rn(r[0], __dmul_rn(t, t));
    r[1] = __dadd_rn(r[1], __dmul_rn(d, d));
  }
  block_sum<3>(r, red, tid);
  if (tid != 0) return;
  out[(long long)b * 4 + 0] = m[0];
  out[(long long)b * 4 + 1] = m[1];
  out[(long long)b * 4 + 2] = m[2];
  out[(long long)b * 4 + 3] = 10.0 * log10(r[0] / fmax(r[1], 1e-30));
  flags[b] = (m[1] > 0.0 && L >= 2) ? 1 : 0;
}

// ---- silent-frame removal ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_NT) void frame_energy_kernel(const float* __restrict__ x, const int* __restrict__ lens, long long ld, double* __restrict__ en,
                                                             long long ldf) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int F = frames_of(lens[b]);
  const long long f = (long long)blockIdx.x * MT_NW + (threadIdx.x >> 6);
  if (f >= F) return;                         // wave-uniform; no barrier below
  const float* xf = x + (long long)b * ld + f * HOP;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < FR / 64; ++i) {
    const int n = lane + 64 * i;
    const double v = window_d(n) * (double)xf[n];
    s += v * v;
  }
  s = wave_sum(s);
  if (lane == 0) en[(long long)b * ldf + f] = 20.0 * log10(sqrt(s) + ST_EPS);
}

__global__ __launch_bounds__(MT_NT) void select_scan_kernel(const double* __restrict__ en, const int* __restrict__ lens, long long ldf, int* __restrict__ src,
                                                            int* __restrict__ K, int* __restrict__ Fo, int* __restrict__ lens_out) {
  __shared__ double smax[MT_NW];
  __shared__ int wtot[2][MT_NW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  const int F = frames_of(lens[b]);
  const double* er = en + (long long)b * ldf;
  int* sr = src + (long long)b * ldf;
  double mx = -INFINITY;
  for (int f = tid; f < F; f += MT_NT) mx = fmax(mx, er[f]);
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
  if (lane == 0) smax[wv] = mx;
  __syncthreads();
  mx = smax[0];
  for (int w = 1; w < MT_NW; ++w) mx = fmax(mx, smax[w]);
  const double thr = mx - 40.0;
  int carry = 0, parity = 0;                  // kept frames before this tile
  for (int f0 = 0; f0 < F; f0 += MT_NT, parity ^= 1) {
    const int f = f0 + tid;
    const bool keep = f < F && er[f] > thr;
    const unsigned long long mask = __ballot(keep);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[parity][wv] = __popcll(mask);
    __syncthreads();                          // two buffers by tile parity: the barrier of tile t + 1 separates the reads of tile t from the writes of t + 2
    int pre = carry, tot = 0;
    for (int w = 0; w < MT_NW; ++w) {
      const int t = wtot[parity][w];
      if (w < wv) pre += t;
      tot += t;
    }
    if (keep) sr[pre + before] = f;           // pre + before < K <= F <= ldf
    carry += tot;
  }
  if (tid == 0) {
    K[b] = carry;
    Fo[b] = F;
    lens_out[b] = carry > 0 ? (carry - 1) * HOP + FR : 0;
  }
}

__global__ __launch_bounds__(MT_NT) void gather_ola_kernel(const float* __restrict__ x, const float* __restrict__ e, long long ld, const int* __restrict__ src,
                                                           long long ldf, const int* __restrict__ K, float* __restrict__ xo, float* __restrict__ eo, long long ldo) {
  const int b = blockIdx.y, k = K[b];
  const long long n = (long long)blockIdx.x * MT_NT + threadIdx.x;
  if (k < 1 || n >= (long long)(k - 1) * HOP + FR) return;
  const int* sr = src + (long long)b * ldf;
  const float* xr = x + (long long)b * ld;
  const float* er = e + (long long)b * ld;
  const long long j1 = n / HOP;               // the later of the two frames covering n; the earlier is j1 - 1
  float ax = 0.f, ae = 0.f;
  bool first = true;
  for (long long j = j1 - 1; j <= j1; ++j) {
    if (j < 0 || j >= k) continue;
    const int i = (int)(n - j * HOP);         // in [0, 256)
    const float w = (float)window_d(i);
    const long long m = (long long)sr[j] * HOP + i;           // < (F - 1) * 128 + 256 <= lens[b]
    const float px = __fmul_rn(w, xr[m]), pe = __fmul_rn(w, er[m]);
    ax = first ? px : __fadd_rn(ax, px);
    ae = first ? pe : __fadd_rn(ae, pe);
    first = false;
  }
  xo[(long long)b * ldo + n] = ax;
  eo[(long long)b * ldo + n] = ae;
}

// ---- the frame FFT: fft512.h, here with frames of 256 samples ------------------------------------------------------------------------------------
struct Bands { int J; int lo[MAXJ]; int hi[MAXJ]; };        // bins [lo, hi) within 0..257, checked by the C entry

__global__ __launch_bounds__(MT_NT) void band_spectra_kernel(const float* __restrict__ x, const int* __restrict__ lens, long long ld, Bands bands,
                                                             float* __restrict__ out, long long ldm) {
  __shared__ FftLds s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
  const int M = frames_of(lens[b]);
  const long long m = (long long)blockIdx.x * MT_NW + wv;
  fft_tables(s, tid, FR);
  frame_load(s, wv, lane, m < M ? x + (long long)b * ld + m * HOP : nullptr, FR);
  const float2* X = frame_fft(s, wv, lane);
  if (m >= M || lane >= bands.J) return;
  double acc = 0.0;
  for (int k = bands.lo[lane]; k < bands.hi[lane]; ++k) acc += (double)X[k].x * (double)X[k].x + (double)X[k].y * (double)X[k].y;
  out[((long long)b * bands.J + lane) * ldm + m] = (float)sqrt(acc);
}

// ---- STOI / ESTOI ------------------------------------------------------------------------------------------------------------------------
// one wave per (row, segment): lane j < J owns band row j (30 values, serial, double), lane n < 30 owns column n of the row-normalised block
__global__ __launch_bounds__(64) void stoi_segments_kernel(const float* __restrict__ X, const float* __restrict__ Y, const int* __restrict__ lens_m, int J,
                                                           long long ldm, double* __restrict__ ws, long long lds_) {
  __shared__ double xr[MAXJ][SEG], yr[MAXJ][SEG];
  __shared__ double part[64];
  const int lane = threadIdx.x, b = blockIdx.y, sg = blockIdx.x;
  const int S = lens_m[b] - (SEG - 1);
  if (sg >= S) return;                        // uniform over the workgroup
  const double clip = 1.0 + 5.623413251903491;               // 1 + 10^(15/20)
  double corr = 0.0;
  if (lane < J) {
    const float* xp = X + ((long long)b * J + lane) * ldm + sg;
    const float* yp = Y + ((long long)b * J + lane) * ldm + sg;
    double xv[SEG], yv[SEG], sx = 0.0, sy = 0.0, mxv = 0.0, myv = 0.0;
#pragma unroll
    for (int n = 0; n < SEG; ++n) {
      xv[n] = (double)xp[n]; yv[n] = (double)yp[n];
      sx += xv[n] * xv[n]; sy += yv[n] * yv[n];
      mxv += xv[n]; myv += yv[n];
    }
    mxv /= (double)SEG; myv /= (double)SEG;
    // ESTOI rows: mean removed, divided by (norm + eps)
    double nx = 0.0, ny = 0.0;
#pragma unroll
    for (int n = 0; n < SEG; ++n) { const double dx = xv[n] - mxv, dy = yv[n] - myv; nx += dx * dx; ny += dy * dy; }
    nx = sqrt(nx) + ST_EPS; ny = sqrt(ny) + ST_EPS;
#pragma unroll
    for (int n = 0; n < SEG; ++n) { xr[lane][n] = (xv[n] - mxv) / nx; yr[lane][n] = (yv[n] - myv) / ny; }
    // STOI row: scale, clip, correlate
    const double c = sqrt(sx) / (sqrt(sy) + ST_EPS);
    double myc = 0.0;
#pragma unroll
    for (int n = 0; n < SEG; ++n) { yv[n] = fmin(c * yv[n], xv[n] * clip); myc += yv[n]; }
    myc /= (double)SEG;
    double nyc = 0.0;
#pragma unroll
    for (int n = 0; n < SEG; ++n) { const double dy = yv[n] - myc; nyc += dy * dy; }
    nyc = sqrt(nyc) + ST_EPS;
#pragma unroll
    for (int n = 0; n < SEG; ++n) corr += ((xv[n] - mxv) / nx) * ((yv[n] - myc) / nyc);
  }
  part[lane] = corr;
  __syncthreads();
  double stoi = 0.0;
  if (lane == 0)
    for (int j = 0; j < J; ++j) stoi += part[j];
  __syncthreads();
  double col = 0.0;
  if (lane < SEG) {
    double mx = 0.0, my = 0.0;
    for (int j = 0; j < J; ++j) { mx += xr[j][lane]; my += yr[j][lane]; }
    mx /= (double)J; my /= (double)J;
    double nx = 0.0, ny = 0.0;
    for (int j = 0; j < J; ++j) { const double dx = xr[j][lane] - mx, dy = yr[j][lane] - my; nx += dx * dx; ny += dy * dy; }
    nx = sqrt(nx) + ST_EPS; ny = sqrt(ny) + ST_EPS;
    for (int j = 0; j < J; ++j) col += ((xr[j][lane] - mx) / nx) * ((yr[j][lane] - my) / ny);
  }
  part[lane] = col;
  __syncthreads();
  if (lane == 0) {
    double estoi = 0.0;
    for (int n = 0; n < SEG; ++n) estoi += part[n];
    ws[((long long)b * 2 + 0) * lds_ + sg] = stoi;
    ws[((long long)b * 2 + 1) * lds_ + sg] = estoi;
  }
}

__global__ __launch_bounds__(MT_NT) void stoi_finalize_kernel(const double* __restrict__ ws, long long lds_, const int* __restrict__ lens_m, int J,
                                                              double* __restrict__ out, int* __restrict__ flags) {
  __shared__ double red[MT_NW][2];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int S = lens_m[b] - (SEG - 1);
  double v[2] = {0.0, 0.0};
  for (int i = tid; i < S; i += MT_NT) { v[0] += ws[((long long)b * 2 + 0) * lds_ + i]; v[1] += ws[((long long)b * 2 + 1) * lds_ + i]; }
  block_sum<2>(v, red, tid);
  if (tid != 0) return;
  const bool ok = S >= 1;
  out[(long long)b * 2 + 0] = ok ? v[0] / ((double)J * (double)S) : __builtin_nan("");
  out[(long long)b * 2 + 1] = ok ? v[1] / ((double)SEG * (double)S) : __builtin_nan("");
  flags[b] = ok ? 1 : 0;
}

// ---- LSD ---------------------------------------------------------------------------------------------------------------------------------
// sum over k = 0..256 of |X[k]|^2 of the windowed frame f (the fp32 products the FFT reads), by Parseval:
// (512 sum f^2 + (sum f)^2 + (sum (-1)^n f)^2) / 2, in double
__global__ __launch_bounds__(MT_NT) void frame_power_kernel(const float* __restrict__ x, const int* __restrict__ lens, long long ld, double* __restrict__ ws,
                                                            long long ldw) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int M = frames_of(lens[b]);
  const long long m = (long long)blockIdx.x * MT_NW + (threadIdx.x >> 6);
  if (m >= M) return;                         // wave-uniform; no barrier below
  const float* xf = x + (long long)b * ld + m * HOP;
  double s2 = 0.0, s1 = 0.0, sa = 0.0;
#pragma unroll
  for (int i = 0; i < FR / 64; ++i) {
    const int n = lane + 64 * i;
    const double v = (double)__fmul_rn((float)window_d(n), xf[n]);
    s2 += v * v; s1 += v; sa += (n & 1) ? -v : v;
  }
  s2 = wave_sum(s2); s1 = wave_sum(s1); sa = wave_sum(sa);
  if (lane == 0) ws[(long long)b * ldw + m] = 0.5 * ((double)NFFT * s2 + s1 * s1 + sa * sa);
}

__global__ __launch_bounds__(MT_NT) void power_finalize_kernel(const double* __restrict__ ws, long long ldw, const int* __restrict__ lens, double* __restrict__ mean_p) {
  __shared__ double red[MT_NW][1];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int M = frames_of(lens[b]);
  double v[1] = {0.0};
  for (int i = tid; i < M; i += MT_NT) v[0] += ws[(long long)b * ldw + i];
  block_sum<1>(v, red, tid);
  if (tid == 0) mean_p[b] = M >= 1 ? v[0] / ((double)NBIN * (double)M) : __builtin_nan("");
}

__global__ __launch_bounds__(MT_NT) void lsd_frames_kernel(const float* __restrict__ e, const float* __restrict__ x, const int* __restrict__ lens, long long ld,
                                                           const double* __restrict__ gain, const double* __restrict__ delta, double* __restrict__ ws,
                                                           long long ldw) {
  __shared__ FftLds s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
  const int M = frames_of(lens[b]);
  const long long m = (long long)blockIdx.x * MT_NW + wv;
  const bool live = m < M;
  fft_tables(s, tid, FR);
  frame_load(s, wv, lane, live ? x + (long long)b * ld + m * HOP : nullptr, FR);
  const float2* X = frame_fft(s, wv, lane);
  double P[NBIN / 64 + 1];                    // bins lane + 64 i, i < 4, and bin 256 in lane 0
#pragma unroll
  for (int i = 0; i <= NBIN / 64; ++i) {
    const int k = lane + 64 * i;
    P[i] = k < NBIN ? (double)X[k].x * (double)X[k].x + (double)X[k].y * (double)X[k].y : 0.0;
  }
  __syncthreads();                            // the spectrum has been read: buffer 0 is free for the second frame
  frame_load(s, wv, lane, live ? e + (long long)b * ld + m * HOP : nullptr, FR);
  const float2* E = frame_fft(s, wv, lane);
  if (!live) return;
  const double g = gain[b], d = delta[b], g2 = g * g;
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i <= NBIN / 64; ++i) {
    const int k = lane + 64 * i;
    if (k < NBIN) {
      const double Q = g2 * ((double)E[k].x * (double)E[k].x + (double)E[k].y * (double)E[k].y);
      const double t = 10.0 * log10((P[i] + d) / (Q + d));
      acc += t * t;
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) ws[(long long)b * ldw + m] = sqrt(acc / (double)NBIN);
}

__global__ __launch_bounds__(MT_NT) void lsd_finalize_kernel(const double* __restrict__ ws, long long ldw, const int* __restrict__ lens, const double* __restrict__ delta,
                                                             double* __restrict__ out, int* __restrict__ flags) {
  __shared__ double red[MT_NW][1];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int M = frames_of(lens[b]);
  double v[1] = {0.0};
  for (int i = tid; i < M; i += MT_NT) v[0] += ws[(long long)b * ldw + i];
  block_sum<1>(v, red, tid);
  if (tid != 0) return;
  const bool ok = M >= 1 && delta[b] > 0.0;   // no full frame, or a clean signal without power (a NaN floor compares false)
  out[b] = ok ? v[0] / (double)M : __builtin_nan("");
  flags[b] = ok ? 1 : 0;
}

}  // namespace

int metrics_tile() { return MT_TILE; }
long long metrics_frames(long long len) { return frames_of(len, FR, HOP); }

void launch_pair_moments(const float* e, const float* x, const int* lens, int B, long long ld, double* out, int* flags, hipStream_t st) {
  hipLaunchKernelGGL(pair_moments_kernel, dim3((unsigned)B), dim3(MT_NT), 0, st, e, x, lens, ld, out, flags);
}

void launch_stoi_select(const float* x, const float* e, const int* lens, int B, long long ld, int max_len, float* xo, float* eo, long long ldo, int* lens_out,
                        int* K, int* F, int* src, long long ldf, double* ws, hipStream_t st) {
  const long long maxF = metrics_frames(max_len);
  if (maxF > 0) hipLaunchKernelGGL(frame_energy_kernel, dim3(tiles_of(maxF, MT_NW), (unsigned)B), dim3(MT_NT), 0, st, x, lens, ld, ws, ldf);
  hipLaunchKernelGGL(select_scan_kernel, dim3((unsigned)B), dim3(MT_NT), 0, st, (const double*)ws, lens, ldf, src, K, F, lens_out);
  if (maxF > 0)
    hipLaunchKernelGGL(gather_ola_kernel, dim3(tiles_of((maxF - 1) * HOP + FR, MT_NT), (unsigned)B), dim3(MT_NT), 0, st, x, e, ld, (const int*)src, ldf,
                       (const int*)K, xo, eo, ldo);
}

void launch_band_spectra(const float* x, const int* lens, int B, long long ld, int max_len, const int* lo, const int* hi, int J, float* out, long long ldm,
                         hipStream_t st) {
  const long long maxM = metrics_frames(max_len);
  if (maxM < 1) return;
  Bands bands;
  bands.J = J;
  for (int j = 0; j < MAXJ; ++j) { bands.lo[j] = j < J ? lo[j] : 0; bands.hi[j] = j < J ? hi[j] : 0; }
  hipLaunchKernelGGL(band_spectra_kernel, dim3(tiles_of(maxM, MT_NW), (unsigned)B), dim3(MT_NT), 0, st, x, lens, ld, bands, out, ldm);
}

void launch_stoi_scores(const float* X, const float* Y, const int* lens_m, int B, int J, long long ldm, int max_m, double* out, int* flags, double* ws,
                        hipStream_t st) {
  const long long maxS = (long long)max_m - (SEG - 1), lds_ = maxS > 1 ? maxS : 1;
  if (maxS >= 1) hipLaunchKernelGGL(stoi_segments_kernel, dim3((unsigned)maxS, (unsigned)B), dim3(64), 0, st, X, Y, lens_m, J, ldm, ws, lds_);
  hipLaunchKernelGGL(stoi_finalize_kernel, dim3((unsigned)B), dim3(MT_NT), 0, st, (const double*)ws, lds_, lens_m, J, out, flags);
}

void launch_frame_power(const float* x, const int* lens, int B, long long ld, int max_len, double* mean_p, double* ws, hipStream_t st) {
  const long long maxM = metrics_frames(max_len), ldw = maxM > 1 ? maxM : 1;
  if (maxM >= 1) hipLaunchKernelGGL(frame_power_kernel, dim3(tiles_of(maxM, MT_NW), (unsigned)B), dim3(MT_NT), 0, st, x, lens, ld, ws, ldw);
  hipLaunchKernelGGL(power_finalize_kernel, dim3((unsigned)B), dim3(MT_NT), 0, st, (const double*)ws, ldw, lens, mean_p);
}

void launch_lsd(const float* e, const float* x, const int* lens, int B, long long ld, int max_len, const double* gain, const double* delta, double* out, int* flags,
                double* ws, hipStream_t st) {
  const long long maxM = metrics_frames(max_len), ldw = maxM > 1 ? maxM : 1;
  if (maxM >= 1) hipLaunchKernelGGL(lsd_frames_kernel, dim3(tiles_of(maxM, MT_NW), (unsigned)B), dim3(MT_NT), 0, st, e, x, lens, ld, gain, delta, ws, ldw);
  hipLaunchKernelGGL(lsd_finalize_kernel, dim3((unsigned)B), dim3(MT_NT), 0, st, (const double*)ws, ldw, lens, delta, out, flags);
}

}  // namespace buddy
