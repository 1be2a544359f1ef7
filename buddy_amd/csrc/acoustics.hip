// Room-acoustic analysis of room impulse responses (buddy_amd/utils/acoustics.py; no reference counterpart: the reference writes its estimated
// RIRs to wav files and stops there).  Three kernels behind three C entries, definitions in DESIGN.md section 16 (ISO 3382-1):
//
//   row_argmax_abs   n0[b] = first index of max |h[b][n]| over n < lens[b]                       one workgroup per row
//   fir_bank         g[b][k][n] = sum_j bank[k][j] h[b][n - j + P], n in [0, lens[b] + P)         zero-phase band signals, tail of P kept
//   decay_metrics    Schroeder curve, EDT / T20 / T30 by least squares, C50, DRR, Ts              one workgroup per (row, band)
//
// Rows are ragged inside a common stride; the lengths are device arrays (arguments, lengths and strides are checked by the C entries, which
// fetch the lengths once).  All of it runs once per tester mode, after sampling: latency-bound, written for clarity.
#include "common.h"
#include "reduce.h"                           // block_sum

namespace buddy {
namespace {
constexpr int AC_NT = 256;                    // threads per workgroup (4 waves)
constexpr int AC_NW = AC_NT / 64;
constexpr int AC_PER = 4;                     // samples per thread and tile
constexpr int AC_TILE = AC_NT * AC_PER;       // the backward sweep's tile (buddy_decay_tile), the FIR's output tile

// ---- direct-path index ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AC_NT) void row_argmax_abs_kernel(const float* __restrict__ h, const int* __restrict__ lens, long long ldh, int* __restrict__ n0) {
  __shared__ float sv[AC_NW];
  __shared__ int si[AC_NW];
  const int tid = threadIdx.x, b = blockIdx.x, L = lens[b];
  const float* hr = h + (long long)b * ldh;
  float best = -1.f;                          // below every |v|: the first sample always wins over the start value (a NaN never does)
  int idx = 0;
  for (int n = tid; n < L; n += AC_NT) {      // ascending n per thread: a strict compare keeps the first index
    const float v = fabsf(hr[n]);
    if (v > best) { best = v; idx = n; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_down(best, off);
    const int oi = __shfl_down(idx, off);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = idx; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < AC_NW; ++w)
      if (sv[w] > best || (sv[w] == best && si[w] < idx)) { best = sv[w]; idx = si[w]; }
    n0[b] = idx;
  }
}

// ---- zero-phase FIR bank ---------------------------------------------------------------------------------------------------------------
// Output n of band k reads h[n - P .. n + P] against the taps in descending order; neighbouring threads read neighbouring samples and the
// same tap (uniform over the wave).  A zero tap is skipped: the bank's rows share one length and the short filters are zero-padded (the 4 kHz
// octave at 16 kHz has 33 taps of 1025), and band 0, a unit impulse, then copies h bit for bit.  fp32 accumulation in ascending input index.
__global__ __launch_bounds__(AC_NT) void fir_bank_kernel(const float* __restrict__ h, const int* __restrict__ lens, long long ldh, const float* __restrict__ bank,
                                                         int nb, int Nh, float* __restrict__ g, long long ldg) {
  const int tid = threadIdx.x, k = blockIdx.y, b = blockIdx.z;
  const int L = lens[b], P = (Nh - 1) / 2;
  const long long Lg = (long long)L + P, t0 = (long long)blockIdx.x * AC_TILE;
  if (t0 >= Lg) return;                                         // a tile past the end of this (short) row
  const float* hr = h + (long long)b * ldh;
  const float* w = bank + (long long)k * Nh;
  float* gr = g + ((long long)b * nb + k) * ldg;
  float acc[AC_PER];
#pragma unroll
  for (int i = 0; i < AC_PER; ++i) acc[i] = 0.f;
  // input index m = n - j + P: tap j meets sample n + P - j.  The tile's outputs n = t0 + tid + i * AC_NT need m in [0, L)
  const long long n_last = (t0 + AC_TILE < Lg ? t0 + AC_TILE : Lg) - 1;
  long long j_lo = t0 + P - (L - 1), j_hi = n_last + P;         // taps that meet a valid sample for at least one output of the tile
  if (j_lo < 0) j_lo = 0;
  if (j_hi > Nh - 1) j_hi = Nh - 1;
  for (long long j = j_hi; j >= j_lo; --j) {                    // descending tap = ascending input index
    const float wj = w[j];
    if (wj == 0.f) continue;                                    // uniform over the workgroup
#pragma unroll
    for (int i = 0; i < AC_PER; ++i) {
      const long long m = t0 + tid + (long long)i * AC_NT + P - j;
      if (m >= 0 && m < L) acc[i] = fmaf(hr[m], wj, acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < AC_PER; ++i) {
    const long long n = t0 + tid + (long long)i * AC_NT;
    if (n < Lg) gr[n] = acc[i];
  }
}

// ---- decay analysis -----------------------------------------------------------------------------------------------------------------
struct DecayRange { double lo, hi; };        // dB, lo <= D <= hi

__global__ __launch_bounds__(AC_NT) void decay_metrics_kernel(const float* __restrict__ g, const int* __restrict__ lens_g, const int* __restrict__ n0s, int nb,
                                                              long long ldg, int fs, int w_dir, int n50, double* __restrict__ out, int* __restrict__ flags,
                                                              float* __restrict__ edc_db) {
  __shared__ double red5[AC_NW][5];
  __shared__ double red[AC_NW][15];
  __shared__ double wave_tot[2][AC_NW];
  __shared__ int red_hi[AC_NW][3];
  __shared__ double s_total;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x / nb;
  const long long rowk = blockIdx.x;                            // = b * nb + k
  const int L = lens_g[b];
  int n0 = n0s[b];
  n0 = n0 < 0 ? 0 : (n0 > L - 1 ? L - 1 : n0);                  // a direct-path index outside the row is clamped, never followed
  const int ns = n0 - w_dir > 0 ? n0 - w_dir : 0;
  const long long n_dir = (long long)n0 + w_dir, n_early = (long long)ns + n50;      // direct part: n <= n_dir; early part: n < n_early
  const float* gr = g + rowk * ldg;
  float* er = edc_db ? edc_db + rowk * ldg : nullptr;

  // forward sweep from ns: early / late energy at the 50 ms split, direct / rest, first moment (in samples from ns)
  double f[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int n = ns + tid; n < L; n += AC_NT) {
    const double v = (double)gr[n], e = v * v;                  // exact: the square of an fp32 value has 48 bits
    if (n < n_early) f[0] += e; else f[1] += e;
    if (n <= n_dir) f[2] += e; else f[3] += e;
    f[4] += (double)(n - ns) * e;
  }
  block_sum<5>(f, red5, tid);
  if (tid == 0) s_total = f[0] + f[1];
  __syncthreads();
  const double total = s_total;                                 // E[ns]
  const bool live = total > 0.0;                                // an all-zero (or non-finite) row: every value NaN, every flag cleared
  if (er)
    for (int n = tid; n < ns; n += AC_NT) er[n] = __builtin_nanf("");      // the curve is not defined before the analysis start

  // backward sweep in tiles of AC_TILE samples from the end of the row: reversed index r = L - 1 - n, thread tid owns r = t0 + tid * AC_PER + i.
  // E[n] = carry (tail energy of the earlier tiles) + the block-wide inclusive scan of the tile: wave64 shuffles, then one LDS exchange of the
  // four wave totals per tile (two buffers by tile parity: the barrier of tile t + 1 separates the reads of tile t from the writes of t + 2)
  const DecayRange rg[3] = {{-10.0, 0.0}, {-25.0, -5.0}, {-35.0, -5.0}};
  double a[15];                                                 // per range: count, sum m, sum D, sum m^2, sum m D   (m = n - ns)
#pragma unroll
  for (int q = 0; q < 15; ++q) a[q] = 0.0;
  int n_hi[3] = {-1, -1, -1};                                   // last fitted sample per range
  double carry = 0.0;
  const int R = L - ns;                                         // samples swept
  int parity = 0;
  for (int t0 = 0; t0 < R; t0 += AC_TILE, parity ^= 1) {
    double e[AC_PER], ts = 0.0;
#pragma unroll
    for (int i = 0; i < AC_PER; ++i) {
      const int r = t0 + tid * AC_PER + i;
      double v = 0.0;
      if (r < R) v = (double)gr[L - 1 - r];
      e[i] = v * v;
      ts += e[i];
    }
    double inc = ts;                                            // inclusive scan over the wave
    for (int off = 1; off < 64; off <<= 1) {
      const double o = __shfl_up(inc, off);
      if (lane >= off) inc += o;
    }
    double excl = __shfl_up(inc, 1);                            // energy of the lanes before this one
    if (lane == 0) excl = 0.0;
    if (lane == 63) wave_tot[parity][wv] = inc;
    __syncthreads();
    double before = carry, tile_tot = 0.0;
#pragma unroll
    for (int w = 0; w < AC_NW; ++w) {
      const double wt = wave_tot[parity][w];
      if (w < wv) before += wt;
      tile_tot += wt;
    }
    double E = before + excl;                           // tail energy behind this thread's first sample
#pragma unroll
    for (int i = 0; i < AC_PER; ++i) {
      const int r = t0 + tid * AC_PER + i;
      E += e[i];
      if (r >= R) continue;
      const int n = L - 1 - r;
      // E[n] <= E[ns] in exact arithmetic; the two come from different summation orders, so the ratio is held at 1 (D <= 0, and D[ns] = 0)
      const double D = live ? 10.0 * log10(fmin(E / total, 1.0)) : __builtin_nan("");
      if (er) er[n] = (float)D;
      const double m = (double)(n - ns);
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (D >= rg[q].lo && D <= rg[q].hi) {
          a[5 * q] += 1.0; a[5 * q + 1] += m; a[5 * q + 2] += D; a[5 * q + 3] += m * m; a[5 * q + 4] += m * D;
          if (n > n_hi[q]) n_hi[q] = n;
        }
    }
    carry += tile_tot;
  }
  block_sum<15>(a, red, tid);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    int v = n_hi[q];
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_down(v, off); v = o > v ? o : v; }
    if (lane == 0) red_hi[wv][q] = v;
  }
  __syncthreads();
  if (tid != 0) return;

  const double nan = __builtin_nan("");
  double val[6] = {nan, nan, nan, nan, nan, nan};
  int fl = 0;
  if (live) {
    for (int q = 0; q < 3; ++q) {
      int nh = red_hi[0][q];
      for (int w = 1; w < AC_NW; ++w) nh = red_hi[w][q] > nh ? red_hi[w][q] : nh;
      const double c = a[5 * q], sm = a[5 * q + 1], sd = a[5 * q + 2], smm = a[5 * q + 3], smd = a[5 * q + 4];
      const double den = c * smm - sm * sm;
      if (c < 2.0 || !(den > 0.0)) continue;                    // fewer than two samples in the range
      const double s = (c * smd - sm * sd) / den * (double)fs;  // dB per second
      if (!(s < 0.0)) continue;                                 // no decay: NaN, flag cleared
      val[q] = -60.0 / s;
      fl |= 1 << q;
      // validity: the decay left between the last fitted sample and the end of the signal, at the fitted slope, is >= 10 dB
      if (-s * (double)(L - 1 - nh) / (double)fs >= 10.0) fl |= 1 << (6 + q);
    }
    if (f[1] > 0.0) { val[3] = 10.0 * log10(f[0] / f[1]); fl |= 1 << 3; }
    if (f[3] > 0.0) { val[4] = 10.0 * log10(f[2] / f[3]); fl |= 1 << 4; }
    val[5] = f[4] / total / (double)fs;
    fl |= 1 << 5;
  }
  for (int q = 0; q < 6; ++q) out[rowk * 6 + q] = val[q];
  flags[rowk] = fl;
}
}  // namespace

int decay_tile() { return AC_TILE; }

void launch_row_argmax_abs(const float* h, const int* lens, int B, long long ldh, int* n0, hipStream_t st) {
  hipLaunchKernelGGL(row_argmax_abs_kernel, dim3((unsigned)B), dim3(AC_NT), 0, st, h, lens, ldh, n0);
}

void launch_fir_bank(const float* h, const int* lens, int B, long long ldh, int max_len, const float* bank, int nb, int Nh, float* g, long long ldg, hipStream_t st) {
  const long long tiles = ((long long)max_len + (Nh - 1) / 2 + AC_TILE - 1) / AC_TILE;
  hipLaunchKernelGGL(fir_bank_kernel, dim3((unsigned)tiles, (unsigned)nb, (unsigned)B), dim3(AC_NT), 0, st, h, lens, ldh, bank, nb, Nh, g, ldg);
}

void launch_decay_metrics(const float* g, const int* lens_g, const int* n0, int B, int nb, long long ldg, int fs, double* out, int* flags, float* edc_db,
                          hipStream_t st) {
  const int w_dir = (int)(((long long)fs + 200) / 400), n50 = (int)(((long long)fs + 10) / 20);      // round(0.0025 fs), round(0.05 fs), halves up
  hipLaunchKernelGGL(decay_metrics_kernel, dim3((unsigned)(B * nb)), dim3(AC_NT), 0, st, g, lens_g, n0, nb, ldg, fs, w_dir, n50, out, flags, edc_db);
}

}  // namespace buddy
