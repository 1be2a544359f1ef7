// Parameter gradients of the score network (training / fine-tuning): the reduction GEMMs over pixels that give the weight gradients of the
// 3x3 / 1x1 convolutions, NIN and Combine layers, the per-channel sums of the biases and GroupNorm affine parameters, and the backward of the
// time-embedding MLP.  Launched from the reverse tape walk of net.hip while each layer's output gradient exists.
//
// Weight gradient: G[n][k] = sum_m dY[m][n] * A[m][k] with m = pixel (K of the GEMM, ~1 M at B = 8), n = output channel, k = tap * Cin + c.
// A is never in HBM: the loader evaluates act(GroupNorm(x)) (and the box / nearest resampling of the down / up blocks) per element, from x,
// the statistics, gamma and beta, like the fused input transforms of the forward.  Exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32).
// (Exact means the products and their accumulation; the loader's normalisation and expf are fp32 evaluations.  Measured against float64 the whole
// kernel stays at or below 5.1e-7 of the abs-max, beside 8.6e-7 for torch's own fp32 autograd: tests/test_hip_param_grad_kernels.py.)
// Split-K over fixed pixel chunks: every workgroup writes its chunk's partial tile, a second pass sums the chunks in chunk order.  No atomics:
// the result is bit-identical from run to run.
#include "common.h"

namespace buddy {

namespace {
constexpr int WG_BN = 64, WG_BK = 256, WG_BP = 32, WG_NT = 256;
constexpr int WG_LY = WG_BN + 32, WG_LA = WG_BK + 32;   // LDS row strides = 32 mod 64 banks: the two lane halves (pixel rows r, r + 1) hit disjoint banks
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float silu_w(float z) { return z / (1.f + expf(-z)); }
__device__ __forceinline__ float dsilu_w(float z) { const float s = 1.f / (1.f + expf(-z)); return s * (1.f + z * (1.f - s)); }

__global__ __launch_bounds__(WG_NT) void wgrad_kernel(const WgY y, const WgA a, long long M, int N, int K, long long ppc, float* __restrict__ part) {
  __shared__ float Ys[WG_BP * WG_LY];
  __shared__ float As[WG_BP * WG_LA];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n0 = blockIdx.x * WG_BN, k0 = blockIdx.y * WG_BK;
  const long long m_begin = (long long)blockIdx.z * ppc;
  const long long m_end = m_begin + ppc < M ? m_begin + ppc : M;
  // the A column this thread loads: k = tap * Cin + c
  const int kk = k0 + tid;
  const bool k_ok = kk < K;
  const int tap = k_ok ? kk / a.Cin : 0, c = k_ok ? kk % a.Cin : 0;
  const int dy = a.taps == 9 ? tap / 3 - 1 : 0, dx = a.taps == 9 ? tap % 3 - 1 : 0;
  const float* src = a.x.p0; int ld = a.x.ld0, cs = c;
  if (a.x.p1 != nullptr && c >= a.x.C0) { src = a.x.p1; ld = a.x.ld1; cs = c - a.x.C0; }
  const bool gn = a.stats != nullptr;
  const float gm = gn && k_ok ? a.gamma[c] : 1.f, bt = gn && k_ok ? a.beta[c] : 0.f;
  const int g = gn ? c / (a.Cin / a.G) : 0;
  const int Hs = a.rs == 1 ? 2 * a.H : a.rs == 2 ? a.H / 2 : a.H, Ws = a.rs == 1 ? 2 * a.W : a.rs == 2 ? a.W / 2 : a.W;
  const int HW = a.H * a.W;
  // the dY column / rows this thread loads
  const int yn = n0 + (tid & 63);
  const bool n_ok = yn < N;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  for (long long ms = m_begin; ms < m_end; ms += WG_BP) {
#pragma unroll
    for (int j = 0; j < WG_BP / 4; ++j) {
      const int pr = (tid >> 6) + 4 * j;
      const long long m = ms + pr;
      float v = 0.f;
      if (m < m_end && n_ok) { const long long b = m / y.T, t = m - b * y.T; v = y.p[b * y.sb + t * y.sm + (long long)yn * y.sn]; }
      Ys[pr * WG_LY + (tid & 63)] = v;
    }
    {
      long long m = ms;
      int b = (int)(m / HW), rem = (int)(m - (long long)b * HW), yy = rem / a.W, xx = rem - yy * a.W;
      for (int pr = 0; pr < WG_BP; ++pr) {
        float v = 0.f;
        const int sy = yy + dy, sx = xx + dx;
        if (m < m_end && k_ok && (unsigned)sy < (unsigned)a.H && (unsigned)sx < (unsigned)a.W) {
          float mean = 0.f, rstd = 1.f;
          if (gn) { mean = a.stats[((long long)b * a.G + g) * 2]; rstd = a.stats[((long long)b * a.G + g) * 2 + 1]; }
          auto act = [&](float u) {
            if (gn) u = (u - mean) * rstd * gm + bt;
            return a.silu ? silu_w(u) : u;
          };
          if (a.rs == 0) {
            v = act(src[(((long long)b * Hs + sy) * Ws + sx) * ld + cs]);
          } else if (a.rs == 2) {
            v = act(src[(((long long)b * Hs + (sy >> 1)) * Ws + (sx >> 1)) * ld + cs]);
          } else {
            const float* q = src + (((long long)b * Hs + 2 * sy) * Ws + 2 * sx) * ld + cs;
            v = ((act(q[0]) + act(q[ld])) + (act(q[(long long)Ws * ld]) + act(q[(long long)Ws * ld + ld]))) * 0.25f;
          }
        }
        As[pr * WG_LA + tid] = v;
        ++m;
        if (++xx == a.W) { xx = 0; if (++yy == a.H) { yy = 0; ++b; } }
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int kp = 0; kp < WG_BP / 2; ++kp) {
      const int r = 2 * kp + (lane >> 5);
      const float y0 = Ys[r * WG_LY + (lane & 31)], y1 = Ys[r * WG_LY + 32 + (lane & 31)];
      const float a0 = As[r * WG_LA + wid * 64 + (lane & 31)], a1 = As[r * WG_LA + wid * 64 + 32 + (lane & 31)];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(y0, a0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(y0, a1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(y1, a0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(y1, a1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  // C/D map of the 32x32 tiles: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* P = part + (long long)blockIdx.z * N * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = k0 + wid * 64 + 32 * j + (lane & 31);
      if (col >= K) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = n0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < N) P[(long long)row * K + col] = acc[i][j][r];
      }
    }
}

// out (+)= alpha * sum over chunks (in chunk order) of part[chunk][n][k], written in the parameter's own layout
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int chunks, int N, int K, int Cin, int layout, float alpha,
                                                           float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * K) return;
  const int n = (int)(i / K), k = (int)(i % K);
  float s = 0.f;
  for (int ch = 0; ch < chunks; ++ch) s += part[(long long)ch * N * K + i];
  long long o;
  if (layout == 0) o = i;                                                    // [N][K]
  else if (layout == 2) o = (long long)k * N + n;                            // [K][N] (NIN W: (in, out))
  else {                                                                     // torch OIHW of a 3x3 conv: tap (dy, dx) is W[o][c][ky = dx][kx = dy]
    const int tap = k / Cin, c = k % Cin;
    o = (((long long)n * Cin + c) * 3 + tap % 3) * 3 + tap / 3;
  }
  out[o] += alpha * s;
}

// per-(utterance, chunk) column sums of dY: part[b][chunk][n]; 64 columns x 4 row lanes per workgroup, combined in a fixed order.  Accumulated in
// double: a bias gradient is a sum of ~10^5 terms that cancel heavily (the C -> 2 heads and output_layer: ~1e-3 relative error in fp32)
constexpr int CS_ROWS = 2048;
__global__ __launch_bounds__(256) void colsum_part_kernel(const WgY y, int N, int chunks, double* __restrict__ part) {
  __shared__ double red[4][64];
  const int b = blockIdx.z, ch = blockIdx.x, n = blockIdx.y * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  const long long t0 = (long long)ch * CS_ROWS, t1 = t0 + CS_ROWS < y.T ? t0 + CS_ROWS : y.T;
  double s = 0.0;
  if (n < N)
    for (long long t = t0 + q; t < t1; t += 4) s += (double)y.p[(long long)b * y.sb + t * y.sm + (long long)n * y.sn];
  red[q][threadIdx.x & 63] = s;
  __syncthreads();
  if (q == 0 && n < N) part[((long long)b * chunks + ch) * N + n] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
// bc != null: bc[b * ld_bc + n] = per-utterance sums (overwritten); out / out2 != null: (+)= alpha * the sum over utterances
__global__ __launch_bounds__(256) void colsum_final_kernel(const double* __restrict__ part, int B, int N, int chunks, float alpha, float* bc, int ld_bc,
                                                           float* out, float* out2) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double tot = 0.0;
  for (int b = 0; b < B; ++b) {
    double s = 0.0;
    for (int ch = 0; ch < chunks; ++ch) s += part[((long long)b * chunks + ch) * N + n];
    if (bc) bc[(long long)b * ld_bc + n] = (float)s;
    tot += s;
  }
  if (out) out[n] += (float)(alpha * tot);
  if (out2) out2[n] += (float)(alpha * tot);
}

// output_layer.bias: the column sums of the frame gradient (colsum_part_kernel's partials) against the inverse DFT's bin sums, in double; one
// workgroup, thread n takes the columns n, n + 256, ... and the 256 results are added in a fixed tree
__global__ __launch_bounds__(256) void basis_bias_final_kernel(const double* __restrict__ part, int B, int K, int chunks, const double* __restrict__ bsum,
                                                               float* out) {
  __shared__ double red[2][256];
  double a0 = 0.0, a1 = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) {
    double tot = 0.0;
    for (int b = 0; b < B; ++b)
      for (int ch = 0; ch < chunks; ++ch) tot += part[((long long)b * chunks + ch) * K + k];
    a0 += tot * bsum[k];
    a1 += tot * bsum[K + k];
  }
  red[0][threadIdx.x] = a0; red[1][threadIdx.x] = a1;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] += (float)red[0][0]; out[1] += (float)red[1][0]; }
}

// GroupNorm affine gradients: per channel sum dz * xhat and sum dz, dz = da_eff * act'(z), z = xhat * gamma + beta.  x at (H, W); da at (H, W)
// (da_mode 0), at (H/2, W/2) scaled by 1/4 (1: the box-downsample's adjoint) or at (2H, 2W) summed over the four children (2: nearest-upsample's)
// (accumulated in double, like the column sums)
constexpr int GN_ROWS = 1024;
__global__ __launch_bounds__(256) void gn_pgrad_part_kernel(const Src2 x, const float* stats, const float* gamma, const float* beta, int G, int silu,
                                                            const float* da, int da_mode, int B, int H, int W, int C, double* __restrict__ part) {
  __shared__ double red[4][64][2];
  const int ch = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  const long long HW = (long long)H * W, M = (long long)B * HW;
  const long long m0 = (long long)ch * GN_ROWS, m1 = m0 + GN_ROWS < M ? m0 + GN_ROWS : M;
  double sg = 0.0, sb = 0.0;
  if (c < C) {
    const int g = c / (C / G);
    const float gm = gamma[c], bt = beta[c];
    const float* src = x.p0; int ld = x.ld0, cs = c;
    if (x.p1 != nullptr && c >= x.C0) { src = x.p1; ld = x.ld1; cs = c - x.C0; }
    for (long long m = m0 + q; m < m1; m += 4) {
      const int b = (int)(m / HW);
      const long long p = m - (long long)b * HW;
      const int h = (int)(p / W), w = (int)(p % W);
      const float mean = stats[((long long)b * G + g) * 2], rstd = stats[((long long)b * G + g) * 2 + 1];
      const float xh = (src[m * ld + cs] - mean) * rstd;
      float d;
      if (da_mode == 0) d = da[m * C + c];
      else if (da_mode == 1) d = 0.25f * da[(((long long)b * (H >> 1) + (h >> 1)) * (W >> 1) + (w >> 1)) * C + c];
      else {
        const float* r = da + (((long long)b * 2 * H + 2 * h) * 2 * W + 2 * w) * C + c;
        d = (r[0] + r[C]) + (r[(long long)2 * W * C] + r[(long long)2 * W * C + C]);
      }
      if (silu) d *= dsilu_w(xh * gm + bt);
      sg += (double)d * xh; sb += d;
    }
  }
  red[q][threadIdx.x & 63][0] = sg; red[q][threadIdx.x & 63][1] = sb;
  __syncthreads();
  if (q == 0 && c < C) {
    const int l = threadIdx.x;
    part[((long long)ch * C + c) * 2] = (red[0][l][0] + red[1][l][0]) + (red[2][l][0] + red[3][l][0]);
    part[((long long)ch * C + c) * 2 + 1] = (red[0][l][1] + red[1][l][1]) + (red[2][l][1] + red[3][l][1]);
  }
}
__global__ __launch_bounds__(256) void gn_pgrad_final_kernel(const double* __restrict__ part, int chunks, int C, float* dgamma, float* dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double sg = 0.0, sb = 0.0;
  for (int ch = 0; ch < chunks; ++ch) { sg += part[((long long)ch * C + c) * 2]; sb += part[((long long)ch * C + c) * 2 + 1]; }
  dgamma[c] += (float)sg; dbeta[c] += (float)sb;
}

// Linear layer y[b][j] = sum_k act(x[b][k]) W[j][k] + bias[j] over a handful of utterances (the time embedding):
// gw[j][k] (+)= sum_b dy[b][j] act(x[b][k]); gb / gb2 (+)= sum_b dy[b][j]
__global__ __launch_bounds__(256) void linear_bwd_w_kernel(const float* dy, int ld_dy, const float* x, int silu_in, int B, int N, int K, float* gw,
                                                           float* gb, float* gb2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * K) return;
  const int j = (int)(i / K), k = (int)(i % K);
  float s = 0.f, sbias = 0.f;
  for (int b = 0; b < B; ++b) {
    float v = x[(long long)b * K + k];
    if (silu_in) v = silu_w(v);
    const float d = dy[(long long)b * ld_dy + j];
    s += d * v; sbias += d;
  }
  gw[i] += s;
  if (k == 0) { if (gb) gb[j] += sbias; if (gb2) gb2[j] += sbias; }
}
// dx[b][k] = act'(x[b][k]) * sum_j dy[b][j] W[j][k]   (act' = 1 without silu_in)
__global__ __launch_bounds__(256) void linear_bwd_x_kernel(const float* dy, const float* Wm, const float* x, int silu_in, int B, int N, int K, float* dx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i % K;
  float s = 0.f;
  for (int j = 0; j < N; ++j) s += dy[(long long)b * N + j] * Wm[(long long)j * K + k];
  dx[i] = silu_in ? s * dsilu_w(x[i]) : s;
}
}  // namespace

int wgrad_chunks(long long M, int N, int K) {
  const long long tiles = (long long)((N + WG_BN - 1) / WG_BN) * ((K + WG_BK - 1) / WG_BK);
  long long ch = (2048 + tiles - 1) / tiles;
  const long long cap = (32LL << 20) / ((long long)N * K);                   // partial tiles <= 128 MB
  if (ch > cap) ch = cap;
  if (ch > (M + 255) / 256) ch = (M + 255) / 256;                             // at least 256 pixels per chunk
  if (ch < 1) ch = 1;
  const long long ppc = ((M + ch - 1) / ch + WG_BP - 1) / WG_BP * WG_BP;
  return (int)((M + ppc - 1) / ppc);
}
long long wgrad_ws_floats(long long M, int N, int K) { return (long long)wgrad_chunks(M, N, K) * N * K; }

void launch_wgrad(const WgY& y, const WgA& a, long long M, int N, int layout, float alpha, float* ws, float* out, hipStream_t st) {
  const int K = a.taps * a.Cin;
  const int chunks = wgrad_chunks(M, N, K);
  const long long ppc = ((M + chunks - 1) / chunks + WG_BP - 1) / WG_BP * WG_BP;
  hipLaunchKernelGGL(wgrad_kernel, dim3((N + WG_BN - 1) / WG_BN, (K + WG_BK - 1) / WG_BK, chunks), dim3(WG_NT), 0, st, y, a, M, N, K, ppc, ws);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv((long long)N * K, 256)), dim3(256), 0, st, (const float*)ws, chunks, N, K, a.Cin, layout, alpha, out);
}

long long colsum_ws_floats(int B, long long T, int N) { return 2LL * B * ((T + CS_ROWS - 1) / CS_ROWS) * N; }   // doubles
long long basis_bias_ws_floats(int B, long long T, int K) { return colsum_ws_floats(B, T, K); }
void launch_basis_bias(const float* x, int K, int B, long long T, const double* bsum, float* ws, float* out, hipStream_t st) {
  WgY y; y.p = x; y.T = T; y.sb = T * K; y.sm = K; y.sn = 1;
  const int chunks = (int)((T + CS_ROWS - 1) / CS_ROWS);
  double* wd = (double*)ws;
  hipLaunchKernelGGL(colsum_part_kernel, dim3(chunks, (K + 63) / 64, B), dim3(256), 0, st, y, K, chunks, wd);
  hipLaunchKernelGGL(basis_bias_final_kernel, dim3(1), dim3(256), 0, st, (const double*)wd, B, K, chunks, bsum, out);
}
void launch_colsum(const WgY& y, int B, int N, float alpha, float* ws, float* bc, int ld_bc, float* out, float* out2, hipStream_t st) {
  const int chunks = (int)((y.T + CS_ROWS - 1) / CS_ROWS);
  double* wd = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(colsum_part_kernel, dim3(chunks, (N + 63) / 64, B), dim3(256), 0, st, y, N, chunks, wd);
  hipLaunchKernelGGL(colsum_final_kernel, dim3((N + 255) / 256), dim3(256), 0, st, (const double*)wd, B, N, chunks, alpha, bc, ld_bc, out, out2);
}

long long gn_pgrad_ws_floats(int B, int H, int W, int C) { return ((long long)B * H * W + GN_ROWS - 1) / GN_ROWS * C * 4; }   // doubles
void launch_gn_pgrad(const Src2& x, const float* stats, const float* gamma, const float* beta, int G, int silu, const float* da, int da_mode, int B,
                     int H, int W, int C, float* ws, float* dgamma, float* dbeta, hipStream_t st) {
  const int chunks = (int)(((long long)B * H * W + GN_ROWS - 1) / GN_ROWS);
  double* wd = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(gn_pgrad_part_kernel, dim3(chunks, (C + 63) / 64), dim3(256), 0, st, x, stats, gamma, beta, G, silu, da, da_mode, B, H, W, C, wd);
  hipLaunchKernelGGL(gn_pgrad_final_kernel, dim3((C + 255) / 256), dim3(256), 0, st, (const double*)wd, chunks, C, dgamma, dbeta);
}

void launch_linear_bwd_w(const float* dy, int ld_dy, const float* x, int silu_in, int B, int N, int K, float* gw, float* gb, float* gb2, hipStream_t st) {
  hipLaunchKernelGGL(linear_bwd_w_kernel, dim3(cdiv((long long)N * K, 256)), dim3(256), 0, st, dy, ld_dy, x, silu_in, B, N, K, gw, gb, gb2);
}
void launch_linear_bwd_x(const float* dy, const float* W, const float* x, int silu_in, int B, int N, int K, float* dx, hipStream_t st) {
  hipLaunchKernelGGL(linear_bwd_x_kernel, dim3(cdiv((long long)B * K, 256)), dim3(256), 0, st, dy, W, x, silu_in, B, N, K, dx);
}

}  // namespace buddy
