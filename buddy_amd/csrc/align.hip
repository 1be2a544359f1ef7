// Time alignment of a pair before it is scored (buddy_amd/utils/metrics.py align; no reference counterpart).  Definitions in DESIGN.md section 19:
// one integer lag per pair (estimate e, clean reference x) from a windowed cross-correlation of the zero-mean signals, and the pair trimmed to its
// overlap.  Kernels behind the C entries of include/buddy_hip.h:
//
//   xcorr_stats      means, zero-mean ||e||^2 and ||x||^2, "defined" (n >= 2, both energies > 0, every input finite)      one workgroup per row
//   xcorr_partial    sums of e~[m + k] x~[m] over one chunk of AL_T samples for one tile of AL_LT lags, into the workspace  one workgroup per
//                                                                                                                         (chunk, lag tile, row)
//   xcorr_reduce     r[k] = the chunks' sums in ascending chunk order                                                    one thread per lag
//   xcorr_peak       the lag of the largest |r[k]| under the tie rule, rho, frac and the flags                           one workgroup per row
//   align_pair       both rows shifted to their overlap, zeros behind it                                                 one thread per output sample
//
// The correlation is direct, not an FFT: every product and every sum is a double operation on the exact fp32 inputs, so r[k] obeys the bound of
// a length-n inner product whatever the order of the terms.  The order is fixed all the same (no atomics): within a chunk a lane sums its samples
// ascending, the four waves of a workgroup are added in wave order, the chunks in chunk order -- a row's r does not depend on its batch.
//
// xcorr_partial: the x~ chunk (AL_T doubles) and the e~ chunk with its halo (AL_T + AL_LT doubles) are staged in LDS, the means subtracted on the way
// in and zeros outside the row.  Wave w owns the samples [w AL_TW, (w + 1) AL_TW) of the chunk, lane l the AL_R = 8 adjacent lags k0 + 8 l + j.  A lane
// keeps a window of 16 e~ values in registers; a step of 8 samples loads 8 new e~ values and 8 x~ values (the same address in every lane: a broadcast)
// for 64 fused multiply-adds.  Lanes read e~ at a stride of 8 doubles, which would put a 32-lane group on 4 banks of 64; the e~ array therefore keeps
// one unused double behind every 8 (index i lives at i + i / 8): the stride becomes 18 dwords and the 32 lanes of a group cover all 64 banks once.
#include "common.h"
#include "reduce.h"                           // block_sum

namespace buddy {
namespace {
constexpr int AL_NT = 256;                    // threads per workgroup (4 waves)
constexpr int AL_NW = AL_NT / 64;
constexpr int AL_R = 8;                       // adjacent lags per lane = samples per step
constexpr int AL_LT = 64 * AL_R;              // lags per tile (buddy_align_lag_tile)
constexpr int AL_TW = 512;                    // samples per wave
constexpr int AL_T = AL_NW * AL_TW;           // samples per chunk (buddy_align_tile)
constexpr int AL_NE = AL_T + AL_LT;           // e~ values a workgroup stages
constexpr int AL_STATS = 5;                   // doubles per row: mean e, mean x, ||e~||^2, ||x~||^2, defined (1 or 0)

__device__ __forceinline__ int pad8(int i) { return i + (i >> 3); }

__global__ __launch_bounds__(AL_NT) void xcorr_stats_kernel(const float* __restrict__ e, const float* __restrict__ x, const int* __restrict__ lens, long long ld,
                                                            double* __restrict__ stats) {
  __shared__ double red[AL_NW][2];
  const int tid = threadIdx.x, b = blockIdx.x, n = lens[b];
  const float* er = e + (long long)b * ld;
  const float* xr = x + (long long)b * ld;
  double s[2] = {0.0, 0.0};
  for (int m = tid; m < n; m += AL_NT) { s[0] += (double)er[m]; s[1] += (double)xr[m]; }
  block_sum<2>(s, red, tid);
  const double me = s[0] / (double)n, mx = s[1] / (double)n;
  double q[2] = {0.0, 0.0};
  for (int m = tid; m < n; m += AL_NT) {
    const double ec = __dsub_rn((double)er[m], me), xc = __dsub_rn((double)xr[m], mx);
    q[0] = fma(ec, ec, q[0]);
    q[1] = fma(xc, xc, q[1]);
  }
  block_sum<2>(q, red, tid);
  if (tid != 0) return;
  double* o = stats + (long long)b * AL_STATS;
  // fp32 inputs cannot overflow a double sum: the sums are finite exactly when every input is
  const bool ok = n >= 2 && isfinite(s[0]) && isfinite(s[1]) && q[0] > 0.0 && q[1] > 0.0;
  o[0] = me; o[1] = mx; o[2] = q[0]; o[3] = q[1]; o[4] = ok ? 1.0 : 0.0;
}

__global__ __launch_bounds__(AL_NT) void xcorr_partial_kernel(const float* __restrict__ e, const float* __restrict__ x, const int* __restrict__ lens, long long ld,
                                                              int K, const double* __restrict__ stats, double* __restrict__ part, long long nchunks) {
  __shared__ double X[AL_T];
  __shared__ double E[AL_NE + AL_NE / 8];     // padded: pad8(); reused for the exchange between the waves (AL_NW * AL_LT doubles fit)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x, lt = blockIdx.y, b = blockIdx.z, n = lens[b];
  const int c0 = c * AL_T;
  if (c0 >= n) return;                        // uniform over the workgroup; xcorr_reduce reads the chunks below ceil(n / AL_T) only
  const int nl = 2 * K + 1, k0 = -K + lt * AL_LT;
  const float* er = e + (long long)b * ld;
  const float* xr = x + (long long)b * ld;
  const double me = stats[(long long)b * AL_STATS + 0], mx = stats[(long long)b * AL_STATS + 1];
  for (int i = tid; i < AL_T; i += AL_NT) {
    const int m = c0 + i;
    X[i] = m < n ? __dsub_rn((double)xr[m], mx) : 0.0;
  }
  for (int i = tid; i < AL_NE; i += AL_NT) {
    const int m = c0 + k0 + i;                // |c0 + k0 + i| < 2^30 + 2^16 + 2^12
    E[pad8(i)] = (m >= 0 && m < n) ? __dsub_rn((double)er[m], me) : 0.0;
  }
  __syncthreads();
  double acc[AL_R], w[2 * AL_R];
#pragma unroll
  for (int j = 0; j < AL_R; ++j) acc[j] = 0.0;
  const int m_lo = wv * AL_TW;
  const int live = n - c0 - m_lo;             // samples of this wave inside the row (wave-uniform)
  const int steps = live <= 0 ? 0 : (live >= AL_TW ? AL_TW / AL_R : (live + AL_R - 1) / AL_R);
  const double* ep = E + pad8(m_lo + AL_R * lane);            // 8 (q) -> 9 q: the 8 values of one group are adjacent
#pragma unroll
  for (int i = 0; i < AL_R; ++i) w[i] = ep[i];
  for (int s = 0; s < steps; ++s) {
    const double* eh = ep + (AL_R + 1) * (s + 1);             // logical m_lo + 8 lane + 8 (s + 1) + i <= AL_T + AL_LT - 1
    const double* xp = X + m_lo + AL_R * s;
    double xv[AL_R];
#pragma unroll
    for (int i = 0; i < AL_R; ++i) { w[AL_R + i] = eh[i]; xv[i] = xp[i]; }
#pragma unroll
    for (int i = 0; i < AL_R; ++i)
#pragma unroll
      for (int j = 0; j < AL_R; ++j) acc[j] = fma(w[i + j], xv[i], acc[j]);
#pragma unroll
    for (int i = 0; i < AL_R; ++i) w[i] = w[AL_R + i];
  }
  __syncthreads();                            // every wave has read E
  double* red = E;                            // [AL_NW][AL_LT]
#pragma unroll
  for (int j = 0; j < AL_R; ++j) red[wv * AL_LT + AL_R * lane + j] = acc[j];
  __syncthreads();
  double* po = part + ((long long)b * nchunks + c) * nl;
  for (int i = tid; i < AL_LT; i += AL_NT) {
    const int ki = lt * AL_LT + i;            // index of lag k0 + i in -K..K
    if (ki >= nl) break;
    double s = red[i];
    for (int q = 1; q < AL_NW; ++q) s += red[q * AL_LT + i];
    po[ki] = s;
  }
}

__global__ __launch_bounds__(AL_NT) void xcorr_reduce_kernel(const double* __restrict__ part, long long nchunks, const int* __restrict__ lens, int K,
                                                             double* __restrict__ r, double* __restrict__ r_out) {
  const int b = blockIdx.y, nl = 2 * K + 1;
  const int ki = blockIdx.x * AL_NT + threadIdx.x;
  if (ki >= nl) return;
  const int nc = (lens[b] + AL_T - 1) / AL_T;
  const double* p = part + (long long)b * nchunks * nl + ki;
  double s = 0.0;
  for (int c = 0; c < nc; ++c) s += p[(long long)c * nl];
  r[(long long)b * nl + ki] = s;
  if (r_out) r_out[(long long)b * nl + ki] = s;
}

// a beats b: larger |r|, then smaller |k|, then k >= 0 (a total order: the result does not depend on the order of the comparisons)
__device__ __forceinline__ bool beats(double va, int ka, double vb, int kb) {
  if (va != vb) return va > vb;
  const int aa = ka < 0 ? -ka : ka, ab = kb < 0 ? -kb : kb;
  if (aa != ab) return aa < ab;
  return ka > kb;
}

__global__ __launch_bounds__(AL_NT) void xcorr_peak_kernel(const double* __restrict__ r, const double* __restrict__ stats, int K, int* __restrict__ lag,
                                                           double* __restrict__ out, int* __restrict__ flags) {
  __shared__ double sv[AL_NT];
  __shared__ int sk[AL_NT];
  const int tid = threadIdx.x, b = blockIdx.x, nl = 2 * K + 1;
  const double* rr = r + (long long)b * nl;
  const double* st = stats + (long long)b * AL_STATS;
  const bool ok = st[4] != 0.0;
  double bv = -1.0;
  int bk = 0;
  if (ok)
    for (int i = tid; i < nl; i += AL_NT) {
      const double v = fabs(rr[i]);
      if (beats(v, i - K, bv, bk)) { bv = v; bk = i - K; }
    }
  sv[tid] = bv; sk[tid] = bk;
  __syncthreads();
  if (tid != 0) return;
  if (!ok) {
    lag[b] = 0; out[(long long)b * 2] = __builtin_nan(""); out[(long long)b * 2 + 1] = 0.0; flags[b] = 0;
    return;
  }
  for (int t = 1; t < AL_NT; ++t)
    if (beats(sv[t], sk[t], bv, bk)) { bv = sv[t]; bk = sk[t]; }
  const int d = bk;
  const double rho = rr[d + K] / sqrt(st[2] * st[3]);
  double frac = 0.0;
  if (d > -K && d < K) {
    const double a = fabs(rr[d + K - 1]), m = fabs(rr[d + K]), c = fabs(rr[d + K + 1]);
    const double den = __dadd_rn(__dsub_rn(a, __dmul_rn(2.0, m)), c);
    if (den < 0.0) frac = __dmul_rn(0.5, __dsub_rn(a, c)) / den;
  }
  lag[b] = d;
  out[(long long)b * 2] = rho;
  out[(long long)b * 2 + 1] = frac;
  flags[b] = 1 | ((K > 0 && (d == K || d == -K)) ? 2 : 0) | (rho < 0.0 ? 4 : 0);
}

__global__ __launch_bounds__(AL_NT) void align_pair_kernel(const float* __restrict__ e, const float* __restrict__ x, const int* __restrict__ lens,
                                                           const int* __restrict__ lag, long long ld, float* __restrict__ eo, float* __restrict__ xo, long long ldo,
                                                           int* __restrict__ lens_out) {
  const int b = blockIdx.y, d = lag[b];
  const int no = lens[b] - (d < 0 ? -d : d);  // >= 1, checked by the C entry
  const long long m = (long long)blockIdx.x * AL_NT + threadIdx.x;
  if (m == 0) lens_out[b] = no;
  if (m >= ldo) return;
  const bool in = m < no;
  eo[(long long)b * ldo + m] = in ? e[(long long)b * ld + m + (d > 0 ? d : 0)] : 0.f;     // m + |d| < lens[b]
  xo[(long long)b * ldo + m] = in ? x[(long long)b * ld + m + (d < 0 ? -d : 0)] : 0.f;
}
}  // namespace

int align_tile() { return AL_T; }
int align_lag_tile() { return AL_LT; }

long long xcorr_workspace_doubles(int B, long long max_len, int K) {
  const long long nl = 2LL * K + 1, nc = (max_len + AL_T - 1) / AL_T;
  return (long long)B * (AL_STATS + nl + nc * nl);
}

void launch_xcorr_lag(const float* e, const float* x, const int* lens, int B, long long ld, int max_len, int K, int* lag, double* out, int* flags, double* r_out,
                      double* ws, hipStream_t st) {
  const long long nl = 2LL * K + 1, nc = ((long long)max_len + AL_T - 1) / AL_T;
  double* stats = ws;
  double* r = stats + (long long)B * AL_STATS;
  double* part = r + (long long)B * nl;
  const unsigned lag_tiles = (unsigned)((nl + AL_LT - 1) / AL_LT);
  hipLaunchKernelGGL(xcorr_stats_kernel, dim3((unsigned)B), dim3(AL_NT), 0, st, e, x, lens, ld, stats);
  hipLaunchKernelGGL(xcorr_partial_kernel, dim3((unsigned)nc, lag_tiles, (unsigned)B), dim3(AL_NT), 0, st, e, x, lens, ld, K, (const double*)stats, part, nc);
  hipLaunchKernelGGL(xcorr_reduce_kernel, dim3((unsigned)((nl + AL_NT - 1) / AL_NT), (unsigned)B), dim3(AL_NT), 0, st, (const double*)part, nc, lens, K, r, r_out);
  hipLaunchKernelGGL(xcorr_peak_kernel, dim3((unsigned)B), dim3(AL_NT), 0, st, (const double*)r, (const double*)stats, K, lag, out, flags);
}

void launch_align_pair(const float* e, const float* x, const int* lens, const int* lag, int B, long long ld, float* eo, float* xo, long long ldo, int* lens_out,
                       hipStream_t st) {
  hipLaunchKernelGGL(align_pair_kernel, dim3((unsigned)((ldo + AL_NT - 1) / AL_NT), (unsigned)B), dim3(AL_NT), 0, st, e, x, lens, lag, ld, eo, xo, ldo, lens_out);
}

}  // namespace buddy
