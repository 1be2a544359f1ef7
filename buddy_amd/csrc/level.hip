// Active speech level of single signals, ITU-T P.56 method B as restated in DESIGN.md section 23 (buddy_amd/utils/level.py; no reference counterpart).
// Kernels behind the C entries of include/buddy_hip.h:
//
//   level_stats     sum and max |x| of every row (the mean and the peak are the caller's two divisions)            tile partials, then one workgroup per row
//   level_classes   the two-pole envelope q of |x - o| in double, one class byte k = #{j : q >= R 2^(j - 15)} per
//                   sample, and sq = sum (x - o)^2                                                                 three launches, below
//   level_counts    a[j] = #{i < n : some i' in [i - I, i] has k_i' >= j + 1}, int64                               four launches, below
//
// Rows are ragged inside a common stride; the lengths are device arrays, checked by the C entries.  Nothing at or behind lens[b] is read or written.
// Every floating-point sum runs in a fixed order, there are no atomics, and a row's result depends neither on B, nor on the grid, nor on the run.
//
// The envelope.  With a = 1 - g the state s = (p, q) moves by p' = g p + a v, q' = g q + a p': s' = M s + (a v, a^2 v), M = g [[1, 0], [a, 1]], and
// M^n = g^n [[1, 0], [n a, 1]].  A run of n samples is the affine map s -> M^n s + c, c its response from the zero state; since n is known from the
// position, c (two doubles) stands for the map, and two neighbouring runs compose as c = M^n2 c1 + c2.  A workgroup of 256 threads owns LV_TILE = 4096
// samples, thread t the LV_R = 16 samples behind 16 t:
//   1. level_env_kernel<false>: every thread runs its samples from the zero state; a Kogge-Stone scan (8 levels; at level k every left operand is
//      moved by the same M^(16 2^k), whose two numbers come from the host) composes them; the last thread leaves the tile's map, and the tile's
//      (x - o)^2 are summed thread by thread, then over a fixed tree.
//   2. level_chain_kernel: per row, serially over its tiles in ascending order: the state each tile starts from (M^4096 s + c) and sq[b].
//   3. level_env_kernel<true>: the same scan with the tile's state given to thread 0; every thread then runs its samples again from the state in
//      front of them and writes the class bytes.
// The per-sample arithmetic is that of the sequential recurrence; the scan adds the roundings of at most 255 compositions per tile (bound in section 23).
//
// The counts.  Thresholds ascend, so "active at j" is: i - last_j(i) <= I, last_j(i) = the latest i' <= i with k_i' > j.  That is a running maximum of
// indices -- integer, exact in any association -- and needs no halo, whatever I is:
//   1. level_hang_kernel<false>: per tile and j the last index with k > j.          2. level_last_chain_kernel: its exclusive running maximum over the
//   tiles of a row.          3. level_hang_kernel<true>: an exclusive maximum scan over the threads (wave shuffles, then the four waves through LDS),
//   every thread walks its 16 bytes and counts, the workgroup adds up.          4. level_count_sum_kernel: the tiles' counts, int64.
#include "common.h"

#include <cmath>

namespace buddy {
namespace {
constexpr int LV_NT = 256, LV_R = 16, LV_TILE = LV_NT * LV_R, LV_LEVELS = 8, LV_NJ = 16, LV_WAVES = LV_NT / 64;
constexpr int LV_NONE = -(1 << 30) - 2;        // "no such sample": i - LV_NONE > 2^30 >= the hangover the kernels use, for every i < 2^30

// g, a = 1 - g; G[k] = g^(16 2^k), NA[k] = (16 2^k) a G[k]: M^(16 2^k) = [[G, 0], [NA, G]].  k = 8 is a whole tile.
struct LvPow { double g, a, G[LV_LEVELS + 1], NA[LV_LEVELS + 1]; };

__device__ inline double block_sum(double v, double* red, int tid) {      // a fixed tree over the 256 threads
  red[tid] = v;
  __syncthreads();
  for (int d = LV_NT / 2; d > 0; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// ---- row statistics ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LV_NT) void level_stats_tile_kernel(const float* __restrict__ x, long long ldx, const int* __restrict__ lens, double* __restrict__ ws,
                                                                 int tiles) {
  __shared__ double red[LV_NT];
  const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y, n = lens[b];
  const long long n0 = (long long)tile * LV_TILE;
  if (n0 >= n) return;                         // uniform over the workgroup
  const float* xr = x + (long long)b * ldx;
  double s = 0.0, m = 0.0;
  for (int q = 0; q < LV_R; ++q) {
    const long long i = n0 + tid + (long long)q * LV_NT;
    if (i < n) {
      const double v = (double)xr[i];
      s += v;
      m = fmax(m, fabs(v));
    }
  }
  s = block_sum(s, red, tid);
  red[tid] = m;
  __syncthreads();
  for (int d = LV_NT / 2; d > 0; d >>= 1) {
    if (tid < d) red[tid] = fmax(red[tid], red[tid + d]);
    __syncthreads();
  }
  if (tid == 0) {
    double* w = ws + ((long long)b * tiles + tile) * 2;
    w[0] = s;
    w[1] = red[0];
  }
}

__global__ __launch_bounds__(LV_NT) void level_stats_row_kernel(const int* __restrict__ lens, const double* __restrict__ ws, int tiles, double* __restrict__ out) {
  __shared__ double red[LV_NT];
  const int tid = threadIdx.x, b = blockIdx.x, n = lens[b];
  const int rt = (n + LV_TILE - 1) / LV_TILE;
  const double* w = ws + (long long)b * tiles * 2;
  double s = 0.0, m = 0.0;
  for (int t = tid; t < rt; t += LV_NT) {
    s += w[2 * t];
    m = fmax(m, w[2 * t + 1]);
  }
  s = block_sum(s, red, tid);
  red[tid] = m;
  __syncthreads();
  for (int d = LV_NT / 2; d > 0; d >>= 1) {
    if (tid < d) red[tid] = fmax(red[tid], red[tid + d]);
    __syncthreads();
  }
  if (tid == 0) {
    out[2 * b] = s;
    out[2 * b + 1] = red[0];
  }
}

// ---- envelope and classes ----------------------------------------------------------------------------------------------------------------------
// ws_c (B, tiles, 3): the tile's map (cp, cq) and its sum of squares; ws_s (B, tiles, 2): the state the tile starts from
template <bool FINAL>
__global__ __launch_bounds__(LV_NT) void level_env_kernel(const float* __restrict__ x, long long ldx, const int* __restrict__ lens, const double* __restrict__ offset,
                                                          const double* __restrict__ ref, LvPow pw, double* __restrict__ ws_c, const double* __restrict__ ws_s,
                                                          int tiles, unsigned char* __restrict__ klass, long long ldk, int vec_x, int vec_k) {
  __shared__ double sp[2][LV_NT], sq[2][LV_NT];
  const int tid = threadIdx.x, tile = blockIdx.x, b = blockIdx.y, n = lens[b];
  const long long n0 = (long long)tile * LV_TILE;
  if (n0 >= n) return;                         // uniform over the workgroup
  const double o = offset ? offset[b] : 0.0;
  const long long s0 = n0 + (long long)tid * LV_R;
  const float* xr = x + (long long)b * ldx + s0;
  double v[LV_R];                              // x - o; zero behind the row's end
  if (vec_x && s0 + LV_R <= n) {
#pragma unroll
    for (int i4 = 0; i4 < LV_R / 4; ++i4) {
      const float4 f = reinterpret_cast<const float4*>(xr)[i4];
      v[4 * i4] = (double)f.x - o; v[4 * i4 + 1] = (double)f.y - o; v[4 * i4 + 2] = (double)f.z - o; v[4 * i4 + 3] = (double)f.w - o;
    }
  } else {
#pragma unroll
    for (int i = 0; i < LV_R; ++i) v[i] = s0 + i < n ? (double)xr[i] - o : 0.0;
  }
  double e2 = 0.0;
  if (!FINAL) {
#pragma unroll
    for (int i = 0; i < LV_R; ++i) e2 += v[i] * v[i];
  }
#pragma unroll
  for (int i = 0; i < LV_R; ++i) v[i] = fabs(v[i]);
  const long long slot = (long long)b * tiles + tile;
  double pin = 0.0, qin = 0.0;                 // the state in front of this thread's samples
  if (FINAL && tid == 0) { pin = ws_s[slot * 2]; qin = ws_s[slot * 2 + 1]; }
  double p = pin, q = qin;
#pragma unroll
  for (int i = 0; i < LV_R; ++i) {
    p = pw.g * p + pw.a * v[i];
    q = pw.g * q + pw.a * p;
  }
  int cur = 0;
  sp[0][tid] = p; sq[0][tid] = q;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < LV_LEVELS; ++k) {
    const int d = 1 << k;
    double P = sp[cur][tid], Q = sq[cur][tid];
    if (tid >= d) {
      const double lp = sp[cur][tid - d], lq = sq[cur][tid - d];
      Q = fma(pw.NA[k], lp, fma(pw.G[k], lq, Q));
      P = fma(pw.G[k], lp, P);
    }
    sp[cur ^ 1][tid] = P; sq[cur ^ 1][tid] = Q;
    __syncthreads();
    cur ^= 1;
  }
  if (!FINAL) {
    if (tid == LV_NT - 1) { ws_c[slot * 3] = sp[cur][tid]; ws_c[slot * 3 + 1] = sq[cur][tid]; }
    const double s = block_sum(e2, sp[cur ^ 1], tid);
    if (tid == 0) ws_c[slot * 3 + 2] = s;
    return;
  }
  if (tid > 0) { pin = sp[cur][tid - 1]; qin = sq[cur][tid - 1]; }
  const double c0 = ref[b] * 0x1p-15;          // c_j = R 2^(j - 15): exact scalings
  p = pin; q = qin;
  unsigned w[LV_R / 4];
#pragma unroll
  for (int i = 0; i < LV_R; ++i) {
    p = pw.g * p + pw.a * v[i];
    q = pw.g * q + pw.a * p;
    unsigned k = 0;
    double c = c0;
#pragma unroll
    for (int j = 0; j < LV_NJ; ++j) { k += q >= c ? 1u : 0u; c *= 2.0; }
    if (i % 4 == 0) w[i / 4] = k; else w[i / 4] |= k << (8 * (i % 4));
  }
  unsigned char* kr = klass + (long long)b * ldk + s0;
  if (vec_k && s0 + LV_R <= n) {
    *reinterpret_cast<uint4*>(kr) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int i = 0; i < LV_R; ++i)
      if (s0 + i < n) kr[i] = (unsigned char)((w[i / 4] >> (8 * (i % 4))) & 0xffu);
  }
}

// one wave per row: 64 tiles at a time through LDS, lane 0 walks them in ascending order
__global__ __launch_bounds__(64) void level_chain_kernel(const int* __restrict__ lens, LvPow pw, const double* __restrict__ ws_c, double* __restrict__ ws_s, int tiles,
                                                         double* __restrict__ sqo) {
  __shared__ double c[64][3], st[64][2];
  const int tid = threadIdx.x, b = blockIdx.x, n = lens[b];
  const int rt = (n + LV_TILE - 1) / LV_TILE;
  const double G = pw.G[LV_LEVELS], NA = pw.NA[LV_LEVELS];
  double p = 0.0, q = 0.0, s = 0.0;            // live in lane 0
  for (int t0 = 0; t0 < rt; t0 += 64) {
    const int m = rt - t0 < 64 ? rt - t0 : 64;
    if (tid < m) {
      const double* w = ws_c + ((long long)b * tiles + t0 + tid) * 3;
      c[tid][0] = w[0]; c[tid][1] = w[1]; c[tid][2] = w[2];
    }
    __syncthreads();
    if (tid == 0) {
      for (int t = 0; t < m; ++t) {
        st[t][0] = p; st[t][1] = q;
        s += c[t][2];
        const double qn = fma(NA, p, fma(G, q, c[t][1]));
        p = fma(G, p, c[t][0]);
        q = qn;
      }
    }
    __syncthreads();
    if (tid < m) {
      double* w = ws_s + ((long long)b * tiles + t0 + tid) * 2;
      w[0] = st[tid][0]; w[1] = st[tid][1];
    }
    __syncthreads();
  }
  if (tid == 0) sqo[b] = s;
}

// ---- hangover and counts -----------------------------------------------------------------------------------------------------------------------
// ws_l (B, tiles, 16): the last index with k > j inside the tile; ws_in (B, tiles, 16): the same over everything in front of the tile;
// ws_n (B, tiles, 16): the tile's counts
template <bool COUNT>
__global__ __launch_bounds__(LV_NT) void level_hang_kernel(const unsigned char* __restrict__ klass, long long ldk, const int* __restrict__ lens, unsigned hang,
                                                           int* __restrict__ ws_l, const int* __restrict__ ws_in, int* __restrict__ ws_n, int tiles, int vec_k) {
  __shared__ int wl[LV_WAVES][LV_NJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, b = blockIdx.y, n = lens[b];
  const long long n0 = (long long)tile * LV_TILE;
  if (n0 >= n) return;                         // uniform over the workgroup
  const int s0 = (int)n0 + tid * LV_R;         // n <= 2^30
  const unsigned char* kr = klass + (long long)b * ldk + s0;
  unsigned w[LV_R / 4] = {0u, 0u, 0u, 0u};
  if (vec_k && s0 + LV_R <= n) {
    const uint4 u = *reinterpret_cast<const uint4*>(kr);
    w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w;
  } else {
#pragma unroll
    for (int i = 0; i < LV_R; ++i)
      if (s0 + i < n) w[i / 4] |= (unsigned)kr[i] << (8 * (i % 4));
  }
  const int live = n - s0 < LV_R ? (n - s0 > 0 ? n - s0 : 0) : LV_R;      // samples of this thread inside the row
  int last[LV_NJ];
#pragma unroll
  for (int j = 0; j < LV_NJ; ++j) last[j] = LV_NONE;
#pragma unroll
  for (int i = 0; i < LV_R; ++i) {
    const int k = i < live ? (int)((w[i / 4] >> (8 * (i % 4))) & 0xffu) : 0;
#pragma unroll
    for (int j = 0; j < LV_NJ; ++j) last[j] = k > j ? s0 + i : last[j];
  }
  const long long slot = ((long long)b * tiles + tile) * LV_NJ;
  if (!COUNT) {
#pragma unroll
    for (int j = 0; j < LV_NJ; ++j) {
      int m = last[j];
      for (int d = 32; d > 0; d >>= 1) m = max(m, __shfl_xor(m, d, 64));
      if (lane == 0) wl[wave][j] = m;
    }
    __syncthreads();
    if (tid < LV_NJ) {
      int m = wl[0][tid];
      for (int q = 1; q < LV_WAVES; ++q) m = max(m, wl[q][tid]);
      ws_l[slot + tid] = m;
    }
    return;
  }
  int exc[LV_NJ];                              // the last index with k > j in front of this thread's samples
#pragma unroll
  for (int j = 0; j < LV_NJ; ++j) {
    int inc = last[j];
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d, 64);
      if (lane >= d) inc = max(inc, t);
    }
    const int t = __shfl_up(inc, 1, 64);
    exc[j] = lane > 0 ? t : LV_NONE;
    if (lane == 63) wl[wave][j] = inc;
  }
  __syncthreads();
  int cnt[LV_NJ];
#pragma unroll
  for (int j = 0; j < LV_NJ; ++j) {
    int m = max(exc[j], ws_in[slot + j]);
    for (int q = 0; q < LV_WAVES - 1; ++q) m = q < wave ? max(m, wl[q][j]) : m;
    exc[j] = m;
    cnt[j] = 0;
  }
#pragma unroll
  for (int i = 0; i < LV_R; ++i) {
    const int k = i < live ? (int)((w[i / 4] >> (8 * (i % 4))) & 0xffu) : 0;
#pragma unroll
    for (int j = 0; j < LV_NJ; ++j) {
      exc[j] = k > j ? s0 + i : exc[j];
      cnt[j] += (i < live && (unsigned)(s0 + i) - (unsigned)exc[j] <= hang) ? 1 : 0;
    }
  }
  __syncthreads();                             // wl is read no more
#pragma unroll
  for (int j = 0; j < LV_NJ; ++j) {
    int m = cnt[j];
    for (int d = 32; d > 0; d >>= 1) m += __shfl_xor(m, d, 64);
    if (lane == 0) wl[wave][j] = m;
  }
  __syncthreads();
  if (tid < LV_NJ) {
    int m = wl[0][tid];
    for (int q = 1; q < LV_WAVES; ++q) m += wl[q][tid];
    ws_n[slot + tid] = m;
  }
}

__global__ __launch_bounds__(LV_NJ) void level_last_chain_kernel(const int* __restrict__ lens, const int* __restrict__ ws_l, int* __restrict__ ws_in, int tiles) {
  const int j = threadIdx.x, b = blockIdx.x, n = lens[b];
  const int rt = (n + LV_TILE - 1) / LV_TILE;
  const long long base = (long long)b * tiles * LV_NJ + j;
  int run = LV_NONE;
#pragma unroll 8
  for (int t = 0; t < rt; ++t) {
    ws_in[base + (long long)t * LV_NJ] = run;
    run = max(run, ws_l[base + (long long)t * LV_NJ]);
  }
}

__global__ __launch_bounds__(LV_NJ) void level_count_sum_kernel(const int* __restrict__ lens, const int* __restrict__ ws_n, int tiles, long long* __restrict__ counts) {
  const int j = threadIdx.x, b = blockIdx.x, n = lens[b];
  const int rt = (n + LV_TILE - 1) / LV_TILE;
  const long long base = (long long)b * tiles * LV_NJ + j;
  long long s = 0;
#pragma unroll 8
  for (int t = 0; t < rt; ++t) s += ws_n[base + (long long)t * LV_NJ];
  counts[(long long)b * LV_NJ + j] = s;
}

int tiles_of(int max_len) { return max_len > 0 ? (max_len + LV_TILE - 1) / LV_TILE : 1; }
}  // namespace

int level_tile() { return LV_TILE; }
int level_counts_tile() { return LV_TILE; }
long long level_stats_ws_bytes(int B, long long max_len) { return 8LL * 2 * B * tiles_of((int)max_len); }
long long level_classes_ws_bytes(int B, long long max_len) { return 8LL * 5 * B * tiles_of((int)max_len); }
long long level_counts_ws_bytes(int B, long long max_len) { return 4LL * 3 * LV_NJ * B * tiles_of((int)max_len); }

void launch_level_stats(const float* x, long long ldx, const int* lens, int B, int max_len, double* out, void* ws, hipStream_t st) {
  const int tiles = tiles_of(max_len);
  if (max_len > 0)
    hipLaunchKernelGGL(level_stats_tile_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(LV_NT), 0, st, x, ldx, lens, (double*)ws, tiles);
  hipLaunchKernelGGL(level_stats_row_kernel, dim3((unsigned)B), dim3(LV_NT), 0, st, lens, (const double*)ws, tiles, out);
}

void launch_level_classes(const float* x, long long ldx, const int* lens, const double* offset, const double* ref, int B, int max_len, double g,
                          unsigned char* klass, long long ldk, double* sq, void* ws, hipStream_t st) {
  LvPow pw;
  pw.g = g;
  pw.a = 1.0 - g;
  for (int k = 0; k <= LV_LEVELS; ++k) {       // powers of the ROUNDED g the samples are run with, formed in extended precision and rounded once
    const long double nk = (long double)(LV_R << k), G = std::pow((long double)g, nk);
    pw.G[k] = (double)G;
    pw.NA[k] = (double)(nk * (long double)pw.a * G);
  }
  const int tiles = tiles_of(max_len);
  double* ws_c = (double*)ws;
  double* ws_s = ws_c + 3LL * B * tiles;
  const int vec_x = (ldx % 4 == 0 && ((uintptr_t)x & 15) == 0) ? 1 : 0;
  const int vec_k = (ldk % 16 == 0 && ((uintptr_t)klass & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)tiles, (unsigned)B);
  if (max_len > 0)
    hipLaunchKernelGGL(level_env_kernel<false>, grid, dim3(LV_NT), 0, st, x, ldx, lens, offset, ref, pw, ws_c, (const double*)ws_s, tiles, klass, ldk, vec_x, vec_k);
  hipLaunchKernelGGL(level_chain_kernel, dim3((unsigned)B), dim3(64), 0, st, lens, pw, (const double*)ws_c, ws_s, tiles, sq);
  if (max_len > 0)
    hipLaunchKernelGGL(level_env_kernel<true>, grid, dim3(LV_NT), 0, st, x, ldx, lens, offset, ref, pw, ws_c, (const double*)ws_s, tiles, klass, ldk, vec_x, vec_k);
}

void launch_level_counts(const unsigned char* klass, long long ldk, const int* lens, int B, int max_len, int hang, long long* counts, void* ws, hipStream_t st) {
  const int tiles = tiles_of(max_len);
  int* ws_l = (int*)ws;
  int* ws_in = ws_l + (long long)LV_NJ * B * tiles;
  int* ws_n = ws_in + (long long)LV_NJ * B * tiles;
  const unsigned h = hang > (1 << 30) ? (1u << 30) : (unsigned)hang;      // rows have at most 2^30 samples: a longer hangover reaches no further
  const int vec_k = (ldk % 16 == 0 && ((uintptr_t)klass & 15) == 0) ? 1 : 0;
  const dim3 grid((unsigned)tiles, (unsigned)B);
  if (max_len > 0) {
    hipLaunchKernelGGL(level_hang_kernel<false>, grid, dim3(LV_NT), 0, st, klass, ldk, lens, h, ws_l, (const int*)ws_in, ws_n, tiles, vec_k);
    hipLaunchKernelGGL(level_last_chain_kernel, dim3((unsigned)B), dim3(LV_NJ), 0, st, lens, (const int*)ws_l, ws_in, tiles);
    hipLaunchKernelGGL(level_hang_kernel<true>, grid, dim3(LV_NT), 0, st, klass, ldk, lens, h, ws_l, (const int*)ws_in, ws_n, tiles, vec_k);
  }
  hipLaunchKernelGGL(level_count_sum_kernel, dim3((unsigned)B), dim3(LV_NJ), 0, st, lens, (const int*)ws_n, tiles, counts);
}

}  // namespace buddy
