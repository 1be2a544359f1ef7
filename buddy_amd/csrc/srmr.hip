// Speech-to-reverberation modulation energy ratio of single signals (buddy_amd/utils/srmr.py; no reference counterpart: the reference scores nothing).
// Definitions in DESIGN.md section 18 (Falk, Zheng & Chan 2010, restated there with every constant fixed).  Kernels behind the C entries of
// include/buddy_hip.h:
//
//   gammatone_env    env[j][n] = |sum_t g_j[t] x[n - t]|, a bank of complex FIR filters, fp32              one tile of one (row, channel) per workgroup
//   modulation       the eight second-order band-pass filters on each envelope and the windowed frame
//                    energies of their outputs, double; the filtered signals are never stored            one recursion per thread
//   srmr_scores      mean frame energies, the 90 % bandwidth, K* and the ratio, double                     one workgroup per row
//
// Rows are ragged inside a common stride; the lengths are device arrays, checked by the C entries.  Nothing behind lens[b] is read, nothing outside the
// declared extents is written.  Every sum runs in a fixed order, there are no atomics, and a row's result does not depend on its batch.
//
// gammatone_env is the one kernel here with an arithmetic load (4 * sum_j N_j flops per input sample).  A workgroup of 256 threads owns GT_TILE = 1024
// consecutive outputs of one (row, channel); thread i owns outputs 4 i .. 4 i + 3.  The tile's inputs and the ceil4(N_j) samples before them lie in LDS
// (zero before the row's start and behind its end).  The taps are walked four at a time, ascending: the four taps are wave-uniform loads, and the seven
// inputs that four outputs need under four taps are two aligned 16-byte LDS words, one of which is the previous step's: one ds_read_b128 per 32
// multiply-adds.  Consecutive lanes read consecutive 16-byte words, which is conflict-free.  Channel lengths differ 20-fold, so the launcher orders the
// grid by descending N_j: the long channels start first and the short ones fill the tail.
#include "common.h"

#include <algorithm>
#include <cstdint>

namespace buddy {
namespace {
constexpr int GT_NT = 256, GT_PER = 4, GT_TILE = GT_NT * GT_PER;
constexpr int GT_MAXN = 1536;                  // longest channel the LDS tile holds (a multiple of 4)
constexpr int SR_MAXJ = 32, SR_K = 8;
constexpr int MD_NT = 64, MD_CH = 8;           // one wave: 8 channels x 8 modulation bands
constexpr int MD_CHUNK = 256;                  // envelope samples per channel staged in LDS at a time
constexpr int MD_MAXW = 4096;

struct GtBank { int J; int off[SR_MAXJ + 1]; int order[SR_MAXJ]; };      // order: channels by descending tap count

__global__ __launch_bounds__(GT_NT) void gammatone_env_kernel(const float* __restrict__ x, const int* __restrict__ lens, long long ld, const float* __restrict__ gre,
                                                              const float* __restrict__ gim, GtBank bank, float* __restrict__ env, long long lde,
                                                              int vec_ok) {
  __shared__ __attribute__((aligned(16))) float xs[GT_MAXN + GT_TILE];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x, b = blockIdx.y, j = bank.order[blockIdx.z];      // z is the slowest grid axis: the longest channel first
  const int L = lens[b];
  const long long n0 = (long long)tile * GT_TILE;
  if (n0 >= L) return;                         // uniform over the workgroup
  const int N = bank.off[j + 1] - bank.off[j];
  const int halo = (N + 3) & ~3;               // samples staged before the tile: a multiple of 4, >= N
  const float* xr = x + (long long)b * ld;
  for (int i = tid; i < halo + GT_TILE; i += GT_NT) {
    const long long m = n0 - halo + i;
    xs[i] = (m >= 0 && m < L) ? xr[m] : 0.f;
  }
  __syncthreads();
  const float* gr = gre + bank.off[j];
  const float* gi = gim + bank.off[j];
  const float4* xs4 = reinterpret_cast<const float4*>(xs);
  // outputs o + i, i < 4, o = 4 tid (relative to the tile); with taps t0 .. t0 + 3 they read xs[base + i - q], base = halo + o - t0:
  // hi = xs[base .. base + 3], lo = xs[base - 4 .. base - 1]
  int w = (halo >> 2) + tid;                   // 16-byte word of base
  float4 hi = xs4[w];
  float ar[GT_PER] = {0.f, 0.f, 0.f, 0.f}, ai[GT_PER] = {0.f, 0.f, 0.f, 0.f};
  for (int t0 = 0; t0 < N; t0 += 4) {
    const float4 lo = xs4[--w];
    const float win[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool live = t0 + q < N;            // wave-uniform; a tap behind the last one counts as zero
      const float cr = live ? gr[t0 + q] : 0.f, ci = live ? gi[t0 + q] : 0.f;
#pragma unroll
      for (int i = 0; i < GT_PER; ++i) {
        ar[i] = __fmaf_rn(cr, win[4 + i - q], ar[i]);
        ai[i] = __fmaf_rn(ci, win[4 + i - q], ai[i]);
      }
    }
    hi = lo;
  }
  const long long n = n0 + 4 * tid;
  float* er = env + ((long long)b * bank.J + j) * lde + n;
  float v[GT_PER];
#pragma unroll
  for (int i = 0; i < GT_PER; ++i) v[i] = sqrtf(__fmaf_rn(ar[i], ar[i], __fmul_rn(ai[i], ai[i])));
  if (vec_ok && n + 3 < L) {
    *reinterpret_cast<float4*>(er) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < GT_PER; ++i)
      if (n + i < L) er[i] = v[i];
  }
}

// ---- modulation bank and frame energies --------------------------------------------------------------------------------------------------------
// lane = 8 c + k: channel j0 + c, band k.  y = b0 x + z1; z1 = b1 x - a1 y + z2; z2 = b2 x - a2 y (direct form II transposed, zero state, a0 = 1).
// Frames of W = 4 H samples at hop H: the samples of hop p lie in the frames p - 3 .. p, at the window offsets 3 H + r .. r; four running sums per lane,
// the oldest is a finished frame after each hop.  Only the (M + 3) hops that full frames cover are walked, so nothing at or behind lens[b] is read.
struct ModCoef { double c[SR_K][6]; };         // b0 b1 b2 a0 a1 a2, a0 = 1

__global__ __launch_bounds__(MD_NT) void modulation_kernel(const float* __restrict__ env, const int* __restrict__ lens, int J, long long lde, ModCoef coef, int K,
                                                           int W, int H, double* __restrict__ E, long long ldm, int* __restrict__ frames) {
  __shared__ double h2[MD_MAXW];               // squared window
  __shared__ __attribute__((aligned(16))) float es[MD_CH][MD_CHUNK + 4];      // rows 4 banks apart: the eight channels' 16-byte reads do not collide
  const int tid = threadIdx.x, c = tid >> 3, k = tid & 7, b = blockIdx.y;
  const int j0 = blockIdx.x * MD_CH, j = j0 + c;
  const int L = lens[b];
  const int M = L >= W ? (L - W) / H + 1 : 0;
  if (blockIdx.x == 0 && tid == 0) frames[b] = M;
  if (M < 1) return;                           // uniform over the workgroup
  for (int i = tid; i < W; i += MD_NT) {
    const double h = 0.54 - 0.46 * cospi(2.0 * (double)(i + 1) / (double)(W + 1));
    h2[i] = h * h;
  }
  const bool live = j < J && k < K;
  const int kk = k < K ? k : 0;
  const double b0 = coef.c[kk][0], b1 = coef.c[kk][1], b2 = coef.c[kk][2], a1 = coef.c[kk][4], a2 = coef.c[kk][5];
  double z1 = 0.0, z2 = 0.0, acc[4] = {0.0, 0.0, 0.0, 0.0};
  double* Er = E + (((long long)b * J + (live ? j : 0)) * K + kk) * ldm;
  const float4* es4 = reinterpret_cast<const float4*>(es[c]);
  for (int p = 0; p < M + 3; ++p) {
    for (int r0 = 0; r0 < H; r0 += MD_CHUNK) {
      __syncthreads();                         // the previous chunk has been read (and, the first time, h2 is written)
      for (int i = tid; i < MD_CH * MD_CHUNK; i += MD_NT) {
        const int cc = i / MD_CHUNK, ii = i % MD_CHUNK;
        es[cc][ii] = j0 + cc < J ? env[((long long)b * J + j0 + cc) * lde + (long long)p * H + r0 + ii] : 0.f;       // (p + 1) H <= (M + 3) H <= L
      }
      __syncthreads();
      for (int i4 = 0; i4 < MD_CHUNK / 4; ++i4) {
        const float4 e4 = es4[i4];
        const float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double xv = (double)ev[q];
          const double y = b0 * xv + z1;
          z1 = b1 * xv - a1 * y + z2;
          z2 = b2 * xv - a2 * y;
          const double y2 = y * y;
          const int r = r0 + 4 * i4 + q;
#pragma unroll
          for (int f = 0; f < 4; ++f) acc[f] += h2[f * H + r] * y2;
        }
      }
    }
    const int m = p - 3;                       // the frame that ended with this hop
    if (live && m >= 0) Er[m] = acc[3];
    acc[3] = acc[2]; acc[2] = acc[1]; acc[1] = acc[0]; acc[0] = 0.0;
  }
}

// ---- scores ------------------------------------------------------------------------------------------------------------------------------------
struct ScoreTab { double erb[SR_MAXJ]; double l[SR_K]; };

__global__ __launch_bounds__(256) void srmr_scores_kernel(const double* __restrict__ E, const int* __restrict__ frames, int J, long long ldm, ScoreTab tab,
                                                          double* __restrict__ out, double* __restrict__ Ebar, int* __restrict__ flags) {
  __shared__ double eb[SR_MAXJ * SR_K], A[SR_MAXJ];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int M = frames[b];
  const double nan = __builtin_nan("");
  if (tid < J * SR_K) {
    const double* Er = E + ((long long)b * J * SR_K + tid) * ldm;
    double s = 0.0;
    for (int m = 0; m < M; ++m) s += Er[m];
    s = M >= 1 ? s / (double)M : nan;
    eb[tid] = s;
    Ebar[(long long)b * J * SR_K + tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  double* o = out + (long long)b * 3;
  double total = 0.0;
  for (int j = 0; j < J; ++j) {
    double a = 0.0;
    for (int k = 0; k < SR_K; ++k) a += eb[j * SR_K + k];
    A[j] = a;
    total += a;
  }
  if (!(M >= 1 && total > 0.0)) {              // no full frame, or no energy (a NaN total compares false)
    o[0] = nan; o[1] = nan; o[2] = nan;
    flags[b] = 0;
    return;
  }
  const double thr = 0.9 * total;
  double run = 0.0, bw = tab.erb[J - 1];
  for (int j = 0; j < J; ++j) {                // channels in index order: ascending centre frequency is the caller's
    run += A[j];
    if (run > thr) { bw = tab.erb[j]; break; }
  }
  int ks = 5;
  for (int k = 5; k < SR_K; ++k) ks += bw >= tab.l[k] ? 1 : 0;
  double num = 0.0, den = 0.0;
  for (int j = 0; j < J; ++j) {
    for (int k = 0; k < 4; ++k) num += eb[j * SR_K + k];
    for (int k = 4; k < ks; ++k) den += eb[j * SR_K + k];
  }
  const bool ok = den > 0.0;
  o[0] = ok ? num / den : nan;
  o[1] = (double)ks;
  o[2] = bw;
  flags[b] = ok ? 1 : 0;
}
}  // namespace

int srmr_tile() { return GT_TILE; }
int srmr_max_taps() { return GT_MAXN; }
int modulation_chunk() { return MD_CHUNK; }
int modulation_max_window() { return MD_MAXW; }

void launch_gammatone_env(const float* x, const int* lens, int B, long long ld, int max_len, const float* gre, const float* gim, const int* tap_off, int J,
                          float* env, long long lde, hipStream_t st) {
  GtBank bank;
  bank.J = J;
  for (int j = 0; j <= SR_MAXJ; ++j) bank.off[j] = tap_off[j < J ? j : J];
  for (int j = 0; j < SR_MAXJ; ++j) bank.order[j] = j < J ? j : 0;
  std::stable_sort(bank.order, bank.order + J, [&](int a, int c) { return bank.off[a + 1] - bank.off[a] > bank.off[c + 1] - bank.off[c]; });
  const int tiles = (max_len + GT_TILE - 1) / GT_TILE;
  const int vec_ok = (lde % 4 == 0 && ((uintptr_t)env & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(gammatone_env_kernel, dim3((unsigned)tiles, (unsigned)B, (unsigned)J), dim3(GT_NT), 0, st, x, lens, ld, gre, gim, bank, env, lde, vec_ok);
}

void launch_modulation_energies(const float* env, const int* lens, int B, int J, long long lde, const double* coef, int K, int W, int H, double* E, long long ldm,
                                int* frames, hipStream_t st) {
  ModCoef c;
  for (int k = 0; k < SR_K; ++k)
    for (int q = 0; q < 6; ++q) c.c[k][q] = k < K ? coef[k * 6 + q] : 0.0;
  hipLaunchKernelGGL(modulation_kernel, dim3((unsigned)((J + MD_CH - 1) / MD_CH), (unsigned)B), dim3(MD_NT), 0, st, env, lens, J, lde, c, K, W, H, E, ldm, frames);
}

void launch_srmr_scores(const double* E, const int* frames, int B, int J, long long ldm, const double* erb, const double* l, double* out, double* Ebar, int* flags,
                        hipStream_t st) {
  ScoreTab tab;
  for (int j = 0; j < SR_MAXJ; ++j) tab.erb[j] = j < J ? erb[j] : 0.0;
  for (int k = 0; k < SR_K; ++k) tab.l[k] = l[k];
  hipLaunchKernelGGL(srmr_scores_kernel, dim3((unsigned)B), dim3(256), 0, st, E, frames, J, ldm, tab, out, Ebar, flags);
}

}  // namespace buddy
