// Multichannel weighted prediction error (WPE) dereverberation, batch "full statistics" variant, complex128: the front end of the
// real-recordings mode for microphone-array files and the WPE-alone baseline of the reports (oracle/wpe_ref.py:91-120 for any D;
// Nakatani et al. 2010, Drude et al. 2018).  The one-channel warm start keeps its own kernel (wpe.hip).
//
// One workgroup per problem = (utterance, frequency bin): D channels x T frames.  With N = D * taps and the stacked history
//   yt_t[k * D + d] = y_{d, t - delay - k}        (k < taps, d < D; zero before the first frame; the tap order is free: X does not depend on it)
// every iteration computes
//   lambda_t = max(mean_d |x_{d,t}|^2, 1e-10 max_t(.)),   R = sum_t yt_t yt_t^H / lambda_t  (N x N),   P = sum_t yt_t y_t^H / lambda_t  (N x D),
//   G = R^{-1} P  (Cholesky),                             x_t = y_t - G^H yt_t.
//
// Organisation.  Frames go through LDS in tiles of TT = 256 / D frames.  A tile holds the history window with the channel order reversed,
//   H[(f - f0) * D + D - 1 - d] = y_{d, f},  f0 = t0 - delay - taps + 1,    so that    yt_t[n] = H[(t - t0 + taps) * D - 1 - n]:
// the N entries of yt_t are N CONSECUTIVE LDS words (descending), whatever D and taps are, and stepping t steps the address by D.  The tile's
// current frames sit in a second window C in the same order.  R and P are cut into 4 x 4 blocks (lower block triangle of R, all of P), one
// block per thread and round: per frame 4 + 4 LDS reads feed 16 complex multiply-adds kept in registers, and the tile's partial sums are added
// to R (packed lower triangle) and P in LDS once per tile.  The Cholesky factorisation is right-looking on the packed triangle with the diagonal
// of L kept aside; the D right-hand sides are solved side by side, a column of L per step; the filter is applied from the same LDS windows.
// Every sum has a fixed order (frames ascending inside a tile, tiles ascending, columns ascending) and no atomics; a problem reads and writes
// only its own rows, so its bits do not depend on the batch.  A pivot <= 0 (silent channel, silent bin) zeroes its column of L and its row of G.
#include "common.h"

namespace buddy {
namespace {
struct __attribute__((aligned(16))) cd { double x, y; };

constexpr int MC_NT = 256;          // threads per workgroup
constexpr int MC_MAXD = 8;
constexpr int MC_MAXN = 96;         // D * taps; LDS at the limit (D = 8, taps = 12), bytes: R 96*97/2*16 = 74496, P 96*8*16 = 12288,
                                    // H ((32 + 11) * 8 + 4) * 16 = 5568, C (256 + 4) * 16 = 4160, weights 32*8, diagonal 96*8, reduction 256*8
                                    // = 99584 of the 163840 a workgroup may hold
constexpr int MC_PAD = 4;           // words in front of H and C: the ragged last 4 x 4 block reads up to 3 words below its first entry
constexpr int MC_WF = 257;

__host__ __device__ inline int mc_tile(int D) { return MC_NT / D; }
__host__ __device__ inline int mc_hwords(int D, int taps) { return (mc_tile(D) + taps - 1) * D + MC_PAD; }
__host__ __device__ inline int mc_cwords(int D) { return mc_tile(D) * D + MC_PAD; }

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }      // packed lower triangle, j <= i

// Y, X: channel d of problem `row` starts at ((row / Fq) * D * Fq + row % Fq) * T + d * Fq * T   (Fq = 1: (rows, D, T); Fq = 257: the
// (B * D, 257, T) layout the STFT kernel writes, row = b * 257 + f).  pw: T doubles per problem.
__global__ __launch_bounds__(MC_NT) void wpe_mc_kernel(const cd* __restrict__ Yall, cd* __restrict__ Xall, double* __restrict__ pw_all, int Fq, int D,
                                                       int T, int taps, int delay, int iters) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int N = D * taps, ntri = N * (N + 1) / 2, TT = mc_tile(D);
  const int hwords = mc_hwords(D, taps), cwords = mc_cwords(D);
  cd* S = reinterpret_cast<cd*>(smem_raw);
  const int oR = 0, oP = ntri, oH = oP + N * D, oC = oH + hwords;                     // offsets into S, in words of 16 bytes
  double* ws = reinterpret_cast<double*>(S + oC + cwords);                            // TT weights 1 / lambda_t of the tile
  double* Ld = ws + TT;                                                               // N: diagonal of L
  double* red = Ld + N;                                                               // MC_NT
  const int row = blockIdx.x, tid = threadIdx.x;
  const long long base = ((long long)(row / Fq) * D * Fq + row % Fq) * T, cs = (long long)Fq * T;
  const cd* y = Yall + base;
  cd* x = Xall + base;
  double* pw = pw_all + (long long)row * T;
  const int ntiles = (T + TT - 1) / TT;
  const int nb4 = (N + 3) / 4, nrb = nb4 * (nb4 + 1) / 2, nblk = nrb + nb4 * ((D + 3) / 4);

  // stage tile `tile`: history window H, current frames C and (weights != 0) 1 / lambda_t
  auto stage = [&](int tile, double floor_p, bool weights) {
    const int t0 = tile * TT, f0 = t0 - delay - taps + 1, hf = TT + taps - 1;
    for (int e = tid; e < hf * D; e += MC_NT) {
      const int d = e / hf, j = e - d * hf, f = f0 + j;
      S[oH + MC_PAD + j * D + D - 1 - d] = (f >= 0 && f < T) ? y[d * cs + f] : cd{0.0, 0.0};
    }
    for (int e = tid; e < TT * D; e += MC_NT) {
      const int d = e / TT, j = e - d * TT, f = t0 + j;
      S[oC + MC_PAD + j * D + D - 1 - d] = f < T ? y[d * cs + f] : cd{0.0, 0.0};
    }
    if (tid < MC_PAD) { S[oH + tid] = cd{0.0, 0.0}; S[oC + tid] = cd{0.0, 0.0}; }
    if (weights && tid < TT) {
      const int f = t0 + tid;
      double w = 0.0;
      if (f < T) { const double p = pw[f], q = p > floor_p ? p : floor_p; w = q > 0.0 ? 1.0 / q : 0.0; }   // a silent bin: weight 0, not 1 / 0
      ws[tid] = w;
    }
  };

  for (int d = 0; d < D; ++d)
    for (int t = tid; t < T; t += MC_NT) x[d * cs + t] = y[d * cs + t];
  __syncthreads();

  for (int it = 0; it < iters; ++it) {
    // ---- power of the current estimate (mean over channels) and its maximum over frames
    double pm = 0.0;
    for (int t = tid; t < T; t += MC_NT) {
      double p = 0.0;
      for (int d = 0; d < D; ++d) { const cd v = x[d * cs + t]; p += v.x * v.x + v.y * v.y; }
      p /= (double)D;
      pw[t] = p;
      pm = p > pm ? p : pm;
    }
    red[tid] = pm;
    for (int e = tid; e < ntri + N * D; e += MC_NT) S[e] = cd{0.0, 0.0};              // R and P are adjacent
    __syncthreads();
    for (int s = MC_NT / 2; s > 0; s >>= 1) { if (tid < s) red[tid] = red[tid] > red[tid + s] ? red[tid] : red[tid + s]; __syncthreads(); }
    const double floor_p = 1e-10 * red[0];

    // ---- R and P, a tile of frames at a time
    for (int tile = 0; tile < ntiles; ++tile) {
      __syncthreads();                                                                // the previous tile's readers are done
      stage(tile, floor_p, true);
      __syncthreads();
      const int nt = T - tile * TT < TT ? T - tile * TT : TT;
      for (int blk = tid; blk < nblk; blk += MC_NT) {
        int i0, j0, ob;                                                               // block rows i0.., columns j0.., column operand window
        const bool isP = blk >= nrb;
        if (!isP) {
          int bi = 0; while ((bi + 1) * (bi + 2) / 2 <= blk) ++bi;
          i0 = 4 * bi; j0 = 4 * (blk - bi * (bi + 1) / 2);
          ob = oH + MC_PAD + taps * D - 1 - j0;                                       // yt_t[j] = H[(tt + taps) * D - 1 - j]
        } else {
          const int q = blk - nrb;
          i0 = 4 * (q % nb4); j0 = 4 * (q / nb4);
          ob = oC + MC_PAD + D - 1 - j0;                                              // y_t[d] = C[(tt + 1) * D - 1 - d]
        }
        const int oa = oH + MC_PAD + taps * D - 1 - i0;
        cd acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = cd{0.0, 0.0};
        for (int tt = 0; tt < nt; ++tt) {
          const double w = ws[tt];
          cd a[4], b[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) { const cd v = S[oa + tt * D - r]; a[r] = cd{w * v.x, w * v.y}; b[r] = S[ob + tt * D - r]; }
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {                                             // a conj(b)
              acc[r][c].x += a[r].x * b[c].x + a[r].y * b[c].y;
              acc[r][c].y += a[r].y * b[c].x - a[r].x * b[c].y;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int i = i0 + r, j = j0 + c;
            if (i < N && (isP ? j < D : j <= i)) {
              cd* dst = S + (isP ? oP + i * D + j : oR + tri(i, j));
              dst->x += acc[r][c].x; dst->y += acc[r][c].y;
            }
          }
      }
    }
    __syncthreads();

    // ---- Cholesky R = L L^H, right-looking on the packed triangle; Ld holds the diagonal of L
    {
      const int ty = tid >> 4, tx = tid & 15;
      for (int c = 0; c < N; ++c) {
        const double dcc = S[oR + tri(c, c)].x;
        const double l = dcc > 0.0 ? sqrt(dcc) : 0.0;
        const double il = l > 0.0 ? 1.0 / l : 0.0;                                    // a zero pivot: a zero column of L, later a zero row of G
        if (tid == 0) Ld[c] = l;
        for (int i = c + 1 + tid; i < N; i += MC_NT) { cd* v = S + oR + tri(i, c); v->x *= il; v->y *= il; }
        __syncthreads();
        for (int i = c + 1 + ty; i < N; i += 16) {
          const cd lic = S[oR + tri(i, c)];
          for (int j = c + 1 + tx; j <= i; j += 16) {
            const cd ljc = S[oR + tri(j, c)];
            cd* v = S + oR + tri(i, j);
            v->x -= lic.x * ljc.x + lic.y * ljc.y; v->y -= lic.y * ljc.x - lic.x * ljc.y;
          }
        }
        __syncthreads();
      }
    }
    // ---- L Z = P, then L^H G = Z, the D right-hand sides side by side, in place in P
    for (int i = 0; i < N; ++i) {
      const double l = Ld[i];
      if (tid < D) { cd* v = S + oP + i * D + tid; *v = l > 0.0 ? cd{v->x / l, v->y / l} : cd{0.0, 0.0}; }
      __syncthreads();
      for (int e = tid; e < (N - 1 - i) * D; e += MC_NT) {
        const int r = i + 1 + e / D, d = e % D;
        const cd lri = S[oR + tri(r, i)], z = S[oP + i * D + d];
        cd* v = S + oP + r * D + d;
        v->x -= lri.x * z.x - lri.y * z.y; v->y -= lri.x * z.y + lri.y * z.x;
      }
      __syncthreads();
    }
    for (int i = N - 1; i >= 0; --i) {
      const double l = Ld[i];
      if (tid < D) { cd* v = S + oP + i * D + tid; *v = l > 0.0 ? cd{v->x / l, v->y / l} : cd{0.0, 0.0}; }
      __syncthreads();
      for (int e = tid; e < i * D; e += MC_NT) {
        const int r = e / D, d = e % D;
        const cd lir = S[oR + tri(i, r)], g = S[oP + i * D + d];                      // conj(L[i][r]) g
        cd* v = S + oP + r * D + d;
        v->x -= lir.x * g.x + lir.y * g.y; v->y -= lir.x * g.y - lir.y * g.x;
      }
      __syncthreads();
    }

    // ---- x_t = y_t - G^H yt_t from the LDS windows; thread = (frame of the tile, channel)
    for (int tile = 0; tile < ntiles; ++tile) {
      __syncthreads();
      stage(tile, 0.0, false);
      __syncthreads();
      const int nt = T - tile * TT < TT ? T - tile * TT : TT;
      if (tid < nt * D) {
        const int tt = tid / D, d = tid - tt * D;
        cd s = S[oC + MC_PAD + (tt + 1) * D - 1 - d];
        const int oa = oH + MC_PAD + (tt + taps) * D - 1;
        for (int n = 0; n < N; ++n) {
          const cd v = S[oa - n], g = S[oP + n * D + d];                              // yt_t[n] conj(G[n][d])
          s.x -= v.x * g.x + v.y * g.y; s.y -= v.y * g.x - v.x * g.y;
        }
        x[d * cs + tile * TT + tt] = s;
      }
    }
    __syncthreads();
  }
}

size_t mc_lds_bytes(int D, int taps) {
  const size_t N = (size_t)D * taps;
  return (N * (N + 1) / 2 + N * D + mc_hwords(D, taps) + mc_cwords(D)) * sizeof(cd) + (mc_tile(D) + N + MC_NT) * sizeof(double);
}
}  // namespace

bool wpe_mc_supported(int D, int taps) { return D >= 1 && D <= MC_MAXD && taps >= 1 && (long long)D * taps <= MC_MAXN; }

static int launch_mc(const cd* Y, cd* X, double* pw, int rows, int Fq, int D, int T, int taps, int delay, int iters, hipStream_t st) {
  const size_t lds = mc_lds_bytes(D, taps);
  if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)wpe_mc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return 1;
  hipLaunchKernelGGL(wpe_mc_kernel, dim3((unsigned)rows), dim3(MC_NT), lds, st, Y, X, pw, Fq, D, T, taps, delay, iters);
  return 0;
}

int launch_wpe_mc(const double* Y, double* X, double* scratch, int rows, int D, int T, int taps, int delay, int iters, hipStream_t st) {
  return launch_mc(reinterpret_cast<const cd*>(Y), reinterpret_cast<cd*>(X), scratch, rows, 1, D, T, taps, delay, iters, st);
}

int launch_wpe_mc_rows(const double* Y, double* X, double* scratch, int rows, int Fq, int D, int T, int taps, int delay, int iters, hipStream_t st) {
  return launch_mc(reinterpret_cast<const cd*>(Y), reinterpret_cast<cd*>(X), scratch, rows, Fq, D, T, taps, delay, iters, st);
}

size_t wpe_mc_workspace_bytes(int B, int D, int L) {         // Y, X: (B * D, 257, T) complex128; power: (B * 257, T) doubles
  const size_t T = (size_t)wpe_frames(L);
  return (size_t)B * MC_WF * T * (2 * (size_t)D * sizeof(cd) + sizeof(double));
}

int launch_wpe_mc_dereverb(const float* y, float* out, void* work, int B, int D, int L, int taps, int delay, int iters, hipStream_t st) {
  const int T = wpe_frames(L);
  const size_t n = (size_t)B * D * MC_WF * T;
  cd* Y = reinterpret_cast<cd*>(work);
  cd* X = Y + n;
  double* pw = reinterpret_cast<double*>(X + n);
  launch_wpe_stft(y, reinterpret_cast<double*>(Y), B * D, L, T, st);                  // the D channels of an item are D rows of the per-row STFT
  if (launch_mc(Y, X, pw, B * MC_WF, MC_WF, D, T, taps, delay, iters, st)) return 1;
  launch_wpe_istft(reinterpret_cast<const double*>(X), out, B * D, L, T, st);
  return 0;
}

}  // namespace buddy
