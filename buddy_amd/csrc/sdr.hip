// Projection SDR of (estimate, clean) pairs over filter lengths (buddy_amd/utils/sdr.py; no reference counterpart).  Definitions in DESIGN.md section
// 31: the estimate e is projected onto the clean signal x and its delayed copies 0..m - 1 (the BSS-Eval SDR of Vincent et al. 2006 for one source);
// what the projection explains is target, the rest distortion.  Kernels behind the C entries of include/buddy_hip.h:
//
//   sdr_partial    sums of e[t + k] x[t] and x[t + k] x[t] over one chunk of SD_T samples for one tile of SD_LT lags k >= 0, and the chunk's sum of
//                  e[t]^2 (lag tile 0 only), into the workspace                                                      one workgroup per (chunk, lag tile, row)
//   sdr_reduce     d[k], r[k] and ee = the chunks' sums in ascending chunk order                                       one thread per sum
//   sdr_solve      the symmetric Levinson recursion on (r, d) up to order N, p_m and SDR_m at the orders asked         one workgroup per row
//
// sdr_partial is of the family of align.hip's xcorr_partial (same chunk, lag tile, register window and LDS padding; read its header for the bank
// arithmetic) but shares no code with it: no means are removed, the lags are 0..N - 1 and not -K..K, and two correlations are taken against one staged
// x chunk, the halo array being filled twice.  Every product and sum is a double operation on the exact fp32 inputs: a direct correlation, no FFT.  The
// order is fixed (no atomics): within a chunk a lane sums its samples ascending, the four waves are added in wave order, the chunks in chunk order.
//
// sdr_solve keeps r, d, the forward vector f (T_n f = e_1) and the solution h as doubles in LDS (4 N doubles: 64 KiB at N = 2048, requested as dynamic
// LDS).  It is N dependent steps of one workgroup reduction and one pairwise update each: latency-bound by construction, no rate is claimed for it.
#include "common.h"
#include "reduce.h"                           // block_sum, tiles_of

namespace buddy {
namespace {
constexpr int SD_NT = 256;                    // threads per workgroup (4 waves)
constexpr int SD_NW = SD_NT / 64;
constexpr int SD_R = 8;                       // adjacent lags per lane = samples per step
constexpr int SD_LT = 64 * SD_R;              // lags per tile (buddy_sdr_lag_tile)
constexpr int SD_TW = 512;                    // samples per wave
constexpr int SD_T = SD_NW * SD_TW;           // samples per chunk (buddy_sdr_tile)
constexpr int SD_NH = SD_T + SD_LT;           // values of the shifted signal a workgroup stages
constexpr int SD_MAXN = 2048;                 // the largest order
constexpr int SD_MAXJ = 8;                    // the most orders reported

struct SdrOrders { int m[SD_MAXJ]; };

__device__ __forceinline__ int pad8(int i) { return i + (i >> 3); }

// H[pad8(i)] = row[m0 + i] for i < SD_NH, zero behind the row's end (m0 >= 0; m0 + i < 2^30 + 2^11 + SD_NH)
__device__ __forceinline__ void stage_shifted(const float* __restrict__ row, int n, int m0, double* H, int tid) {
  for (int i = tid; i < SD_NH; i += SD_NT) {
    const int m = m0 + i;
    H[pad8(i)] = m < n ? (double)row[m] : 0.0;
  }
}

// po[i] = sum over the chunk's samples t of H[t + i] X[t], i < nk <= SD_LT.  ``live``: samples of the chunk inside the row.  Called by the whole
// workgroup with X and H staged and a barrier behind them; H is overwritten (the exchange between the waves) and free again on return
__device__ __forceinline__ void tile_sums(const double* X, double* H, int live_chunk, int tid, double* __restrict__ po, int nk) {
  const int lane = tid & 63, wv = tid >> 6;
  double acc[SD_R], w[2 * SD_R];
#pragma unroll
  for (int j = 0; j < SD_R; ++j) acc[j] = 0.0;
  const int m_lo = wv * SD_TW;
  const int live = live_chunk - m_lo;         // samples of this wave inside the row (wave-uniform); X is zero behind them
  const int steps = live <= 0 ? 0 : (live >= SD_TW ? SD_TW / SD_R : (live + SD_R - 1) / SD_R);
  const double* hp = H + pad8(m_lo + SD_R * lane);            // 8 (q) -> 9 q: the 8 values of one group are adjacent
#pragma unroll
  for (int i = 0; i < SD_R; ++i) w[i] = hp[i];
  for (int s = 0; s < steps; ++s) {
    const double* hh = hp + (SD_R + 1) * (s + 1);             // logical m_lo + 8 lane + 8 (s + 1) + i <= SD_T + SD_LT - 1
    const double* xp = X + m_lo + SD_R * s;
    double xv[SD_R];
#pragma unroll
    for (int i = 0; i < SD_R; ++i) { w[SD_R + i] = hh[i]; xv[i] = xp[i]; }
#pragma unroll
    for (int i = 0; i < SD_R; ++i)
#pragma unroll
      for (int j = 0; j < SD_R; ++j) acc[j] = fma(w[i + j], xv[i], acc[j]);
#pragma unroll
    for (int i = 0; i < SD_R; ++i) w[i] = w[SD_R + i];
  }
  __syncthreads();                            // every wave has read H
  double* red = H;                            // [SD_NW][SD_LT]
#pragma unroll
  for (int j = 0; j < SD_R; ++j) red[wv * SD_LT + SD_R * lane + j] = acc[j];
  __syncthreads();
  for (int i = tid; i < nk; i += SD_NT) {
    double s = red[i];
    for (int q = 1; q < SD_NW; ++q) s += red[q * SD_LT + i];
    po[i] = s;
  }
  __syncthreads();                            // red has been read: H may be staged again
}

// part (B, nchunks, 2 N + 1): per chunk d[0..N), r[0..N), ee
__global__ __launch_bounds__(SD_NT) void sdr_partial_kernel(const float* __restrict__ e, const float* __restrict__ x, const int* __restrict__ lens, long long ld,
                                                            int N, double* __restrict__ part, long long nchunks) {
  __shared__ double X[SD_T];
  __shared__ double H[SD_NH + SD_NH / 8];     // padded: pad8()
  __shared__ double red[SD_NW][1];
  const int tid = threadIdx.x;
  const int c = blockIdx.x, lt = blockIdx.y, b = blockIdx.z, n = lens[b];
  const int c0 = c * SD_T;
  if (c0 >= n) return;                        // uniform over the workgroup; sdr_reduce reads the chunks below ceil(n / SD_T) only
  const int k0 = lt * SD_LT, nk = N - k0 < SD_LT ? N - k0 : SD_LT;
  const float* er = e + (long long)b * ld;
  const float* xr = x + (long long)b * ld;
  double* po = part + ((long long)b * nchunks + c) * (2LL * N + 1);
  for (int i = tid; i < SD_T; i += SD_NT) {
    const int m = c0 + i;
    X[i] = m < n ? (double)xr[m] : 0.0;
  }
  stage_shifted(er, n, c0 + k0, H, tid);
  __syncthreads();
  if (lt == 0) {                              // uniform: the first SD_T values of H are the chunk of e itself
    double s[1] = {0.0};
    for (int i = tid; i < SD_T; i += SD_NT) { const double v = H[pad8(i)]; s[0] = fma(v, v, s[0]); }
    block_sum<1>(s, red, tid);
    if (tid == 0) po[2LL * N] = s[0];
  }
  tile_sums(X, H, n - c0, tid, po + k0, nk);
  stage_shifted(xr, n, c0 + k0, H, tid);
  __syncthreads();
  tile_sums(X, H, n - c0, tid, po + N + k0, nk);
}

__global__ __launch_bounds__(SD_NT) void sdr_reduce_kernel(const double* __restrict__ part, long long nchunks, const int* __restrict__ lens, int N,
                                                           double* __restrict__ r, double* __restrict__ d, double* __restrict__ ee) {
  const int b = blockIdx.y, nl = 2 * N + 1;
  const int ki = blockIdx.x * SD_NT + threadIdx.x;
  if (ki >= nl) return;
  const int nc = (lens[b] + SD_T - 1) / SD_T;
  const double* p = part + (long long)b * nchunks * nl + ki;
  double s = 0.0;
  for (int c = 0; c < nc; ++c) s += p[(long long)c * nl];
  if (ki < N) d[(long long)b * N + ki] = s;
  else if (ki < 2 * N) r[(long long)b * N + ki - N] = s;
  else ee[b] = s;
}

// dynamic LDS: R, D, F, Hs (N doubles each), then the two reduction arrays
__global__ __launch_bounds__(SD_NT) void sdr_solve_kernel(const double* __restrict__ r, const double* __restrict__ d, const double* __restrict__ ee,
                                                          const int* __restrict__ lens, int N, SdrOrders ord, int J, double loading, double* __restrict__ sdr,
                                                          double* __restrict__ p, int* __restrict__ flags, double* __restrict__ hout) {
  extern __shared__ double sd_smem[];
  double* R = sd_smem;
  double* D = R + N;
  double* F = D + N;
  double* Hs = F + N;
  double (&red2)[SD_NW][2] = *reinterpret_cast<double (*)[SD_NW][2]>(Hs + N);
  double (&red1)[SD_NW][1] = *reinterpret_cast<double (*)[SD_NW][1]>(Hs + N + 2 * SD_NW);
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int i = tid; i < N; i += SD_NT) {
    R[i] = r[(long long)b * N + i];
    D[i] = d[(long long)b * N + i];
    F[i] = 0.0;
    Hs[i] = 0.0;
  }
  __syncthreads();
  const double e2 = ee[b], t0 = R[0] * (1.0 + loading);
  // fp32 inputs cannot overflow a double sum: r[0] and ee are finite exactly when every input is
  bool ok = lens[b] >= 2 && R[0] > 0.0 && e2 > 0.0 && isfinite(R[0]) && isfinite(e2);
  if (tid == 0 && ok) { F[0] = 1.0 / t0; Hs[0] = D[0] / t0; }
  __syncthreads();
  double* so = sdr + (long long)b * J;
  double* pp = p + (long long)b * J;
  int fl = 0, j = 0;
  if (ok)
    for (int n = 1;; ++n) {                   // F and Hs hold the vectors of order n; every branch below is uniform over the workgroup
      if (j < J && ord.m[j] == n) {
        double s[1] = {0.0};
        for (int i = tid; i < n; i += SD_NT) s[0] = fma(Hs[i], D[i], s[0]);
        block_sum<1>(s, red1, tid);
        const double pm = s[0], res = e2 - pm;
        if (!(pm > 0.0)) ok = false;
        if (res < 4.0 * loading * e2) fl |= 2;
        if (tid == 0) { pp[j] = pm; so[j] = 10.0 * log10(pm / fmax(res, 1e-12 * e2)); }
        ++j;
      }
      if (n == N) break;
      double s[2] = {0.0, 0.0};
      for (int i = tid; i < n; i += SD_NT) {
        const double rv = R[n - i];           // n - i >= 1: the loading sits on r[0], which the start alone uses
        s[0] = fma(rv, F[i], s[0]);
        s[1] = fma(rv, Hs[i], s[1]);
      }
      block_sum<2>(s, red2, tid);             // its barriers stand between these reads of F, Hs and the writes below
      const double ef = s[0], piv = 1.0 - ef * ef;
      if (!(piv > 0.0)) { ok = false; break; }
      if (piv < 0x1p-26) fl |= 4;
      const double g = D[n] - s[1];
      for (int i = tid; 2 * i <= n; i += SD_NT) {             // the pair (i, n - i) belongs to one thread: in place.  F[n] = Hs[n] = 0 on entry
        const int k = n - i;
        const double a = F[i], c = F[k];
        const double na = (a - ef * c) / piv, nc = (c - ef * a) / piv;
        F[i] = na;
        Hs[i] = fma(g, nc, Hs[i]);
        if (k != i) { F[k] = nc; Hs[k] = fma(g, na, Hs[k]); }
      }
      __syncthreads();
    }
  ok = ok && j == J;
  if (tid == 0) {
    flags[b] = (ok ? 1 : 0) | fl;
    if (!ok)
      for (int q = 0; q < J; ++q) { so[q] = __builtin_nan(""); pp[q] = __builtin_nan(""); }
  }
  if (hout) {
    __syncthreads();
    for (int i = tid; i < N; i += SD_NT) hout[(long long)b * N + i] = ok ? Hs[i] : 0.0;
  }
}
}  // namespace

int sdr_tile() { return SD_T; }
int sdr_lag_tile() { return SD_LT; }
int sdr_max_order() { return SD_MAXN; }
int sdr_max_orders() { return SD_MAXJ; }

long long sdr_products_workspace_doubles(int B, long long max_len, int N) {
  return (long long)B * ((max_len + SD_T - 1) / SD_T) * (2LL * N + 1);
}

void launch_sdr_products(const float* e, const float* x, const int* lens, int B, long long ld, int max_len, int N, double* r, double* d, double* ee, double* ws,
                         hipStream_t st) {
  const long long nc = ((long long)max_len + SD_T - 1) / SD_T;
  hipLaunchKernelGGL(sdr_partial_kernel, dim3((unsigned)nc, tiles_of(N, SD_LT), (unsigned)B), dim3(SD_NT), 0, st, e, x, lens, ld, N, ws, nc);
  hipLaunchKernelGGL(sdr_reduce_kernel, dim3(tiles_of(2LL * N + 1, SD_NT), (unsigned)B), dim3(SD_NT), 0, st, (const double*)ws, nc, lens, N, r, d, ee);
}

int launch_sdr_solve(const double* r, const double* d, const double* ee, const int* lens, int B, int N, const int* orders, int J, double loading, double* sdr,
                     double* p, int* flags, double* h, hipStream_t st) {
  SdrOrders ord;
  for (int q = 0; q < SD_MAXJ; ++q) ord.m[q] = q < J ? orders[q] : 0;
  const size_t lds = (4 * (size_t)N + 3 * SD_NW) * sizeof(double);
  if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)sdr_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return 1;
  hipLaunchKernelGGL(sdr_solve_kernel, dim3((unsigned)B), dim3(SD_NT), lds, st, r, d, ee, lens, N, ord, J, loading, sdr, p, flags, h);
  return 0;
}

}  // namespace buddy
