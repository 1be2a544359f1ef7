// wMPDR beamformer after multichannel WPE (weighted-power minimisation distortionless response), complex128: the second stage of the array
// front end of the real-recordings mode and of the WPE + beamformer baseline of the reports.  With the WPE weights reused it is the factorised
// form of the convolutional beamformer of Nakatani & Kinoshita (2019/2020).  DESIGN.md section 25 fixes every constant.
//
// One workgroup of 256 threads per problem = (item, frequency bin): D channels x T frames in, one channel out.
//   steering   Phi = sum_t x_t x_t^H;  A <- Phi, ten times { A <- A / max|A_ij|, A <- A A, A <- (A + A^H) / 2 };  v = A[:, r] / A[r][r]
//   iteration  lambda_t = max(p_t, 1e-10 max_t p_t),  p_t = mean_d |x_dt|^2 first and |z_t|^2 of the previous iteration afterwards
//              R = sum_t x_t x_t^H / lambda_t + loading tr(R) / D I,   u = R^-1 v (Cholesky),   w = u / (v^H u),   z_t = w^H x_t
// Pass-through z_t = x_{r,t}: Phi all zero, |v_r|^2 < 1e-12 |v|^2 or v_r = 0, a pivot <= 0 (or not a number), v^H u zero or not finite.
// max_t p_t = 0: z = 0.  D = 1: a copy.
//
// Organisation.  The kernel is a template on D: a thread walks the frames t = tid, tid + 256, ... (16-byte loads, coalesced along T) with the
// packed lower triangle of Phi or R in its registers, D (D + 1) / 2 complex doubles.  The partial sums of the 256 threads are added in one fixed
// tree (a butterfly inside a wave, the four wave totals in wave order) whose result lands in EVERY thread, so every thread then holds the same R
// and runs the same D x D Cholesky solve in its own registers: no broadcast and no divergence.  The squarings work on the full matrix in LDS,
// one lane per entry.  Frames are streamed from global memory in every pass (one pass for Phi, two per iteration); a problem's rows stay in
// the L2 between passes at the lengths of an item and any T >= 1 takes the same path.  p_t and z_t of frame t are written and read back by the
// same thread.  No atomics; a problem reads and writes only its own rows, so its bits do not depend on the batch.
#include "common.h"

namespace buddy {
namespace {
struct __attribute__((aligned(16))) cd { double x, y; };

constexpr int BF_NT = 256;          // threads per workgroup
constexpr int BF_NW = BF_NT / 64;   // waves
constexpr int BF_MAXD = 8;
constexpr int BF_SQUARINGS = 10;    // fixed: not a convergence test
constexpr int BF_WF = 257;

__host__ __device__ constexpr int bf_tri(int i, int j) { return i * (i + 1) / 2 + j; }      // packed lower triangle, j <= i

// K sums over the workgroup, the result in every thread; lds may be reused by the next call (the leading barrier covers it)
template <int K>
__device__ __forceinline__ void bf_block_sum(double (&v)[K], double (&lds)[BF_NW][K], int tid) {
#pragma unroll
  for (int q = 0; q < K; ++q)
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off);
  __syncthreads();
  if ((tid & 63) == 0)
#pragma unroll
    for (int q = 0; q < K; ++q) lds[tid >> 6][q] = v[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < K; ++q) {
    double s = lds[0][q];
    for (int w = 1; w < BF_NW; ++w) s += lds[w][q];
    v[q] = s;
  }
}

__device__ __forceinline__ double bf_block_max(double v, double (&lds)[BF_NW], int tid) {
  for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(v, off); v = o > v ? o : v; }
  __syncthreads();
  if ((tid & 63) == 0) lds[tid >> 6] = v;
  __syncthreads();
  double m = lds[0];
  for (int w = 1; w < BF_NW; ++w) m = lds[w] > m ? lds[w] : m;
  return m;
}

// X: channel d of problem `row` starts at ((row / Fq) * D * Fq + row % Fq) * T + d * Fq * T, as in wpe_mc_kernel (Fq = 1: (rows, D, T); Fq = 257:
// the (B * D, 257, T) layout of the STFT kernel, row = b * 257 + f).  Z: (rows, T).  pw: T doubles per problem.
template <int D>
__global__ __launch_bounds__(BF_NT) void mpdr_kernel(const cd* __restrict__ Xall, cd* __restrict__ Zall, double* __restrict__ pw_all, int Fq, int T,
                                                     int ref, int iters, double loading) {
  constexpr int NTRI = D * (D + 1) / 2;
  __shared__ double part[BF_NW][2 * NTRI];
  __shared__ double pmax[BF_NW];
  __shared__ cd A[D * D], A2[D * D];
  const int row = blockIdx.x, tid = threadIdx.x;
  const long long base = ((long long)(row / Fq) * D * Fq + row % Fq) * T, cs = (long long)Fq * T;
  const cd* x = Xall + base;
  cd* z = Zall + (long long)row * T;
  double* pw = pw_all + (long long)row * T;

  auto pass_through = [&]() { for (int t = tid; t < T; t += BF_NT) z[t] = x[ref * cs + t]; };
  if (D == 1) { pass_through(); return; }

  // ---- Phi (unweighted), p_t = mean_d |x_dt|^2 and its maximum
  double acc[2 * NTRI];
#pragma unroll
  for (int e = 0; e < 2 * NTRI; ++e) acc[e] = 0.0;
  double pm = 0.0;
  for (int t = tid; t < T; t += BF_NT) {
    cd xv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) xv[d] = x[d * cs + t];
    double p = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) p += xv[d].x * xv[d].x + xv[d].y * xv[d].y;
    p /= (double)D;
    pw[t] = p;
    pm = p > pm ? p : pm;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {                                                  // x_i conj(x_j)
        acc[2 * bf_tri(i, j)] += xv[i].x * xv[j].x + xv[i].y * xv[j].y;
        acc[2 * bf_tri(i, j) + 1] += xv[i].y * xv[j].x - xv[i].x * xv[j].y;
      }
  }
  bf_block_sum<2 * NTRI>(acc, part, tid);
  pm = bf_block_max(pm, pmax, tid);

  // ---- steering vector: ten normalised squarings of Phi in LDS, one lane per entry
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        A[i * D + j] = cd{acc[2 * bf_tri(i, j)], acc[2 * bf_tri(i, j) + 1]};
        A[j * D + i] = cd{acc[2 * bf_tri(i, j)], -acc[2 * bf_tri(i, j) + 1]};
      }
  }
  const int ei = tid / D, ej = tid - ei * D;                                           // entry of lane tid < D * D
  for (int s = 0; s < BF_SQUARINGS; ++s) {
    __syncthreads();
    double m = 0.0;
    for (int e = 0; e < D * D; ++e) { const cd a = A[e]; const double v = sqrt(a.x * a.x + a.y * a.y); m = v > m ? v : m; }
    if (m == 0.0) { pass_through(); return; }                                         // the same m in every thread
    __syncthreads();
    if (tid < D * D) { A[tid].x /= m; A[tid].y /= m; }
    __syncthreads();
    if (tid < D * D) {
      cd sum{0.0, 0.0};
      for (int k = 0; k < D; ++k) {
        const cd a = A[ei * D + k], b = A[k * D + ej];
        sum.x += a.x * b.x - a.y * b.y; sum.y += a.x * b.y + a.y * b.x;
      }
      A2[tid] = sum;
    }
    __syncthreads();
    if (tid < D * D) { const cd a = A2[ei * D + ej], b = A2[ej * D + ei]; A[tid] = cd{0.5 * (a.x + b.x), 0.5 * (a.y - b.y)}; }
  }
  __syncthreads();
  double nv = 0.0;
  for (int d = 0; d < D; ++d) { const cd a = A[d * D + ref]; nv += a.x * a.x + a.y * a.y; }
  const double vr = A[ref * D + ref].x;                                               // the diagonal of (A + A^H) / 2 is real
  if (vr * vr < 1e-12 * nv || vr == 0.0) { pass_through(); return; }
  cd* v = A2;                                                                         // the steering vector stays in LDS: every thread reads the same words
  if (tid < D) { const cd a = A[tid * D + ref]; v[tid] = cd{a.x / vr, a.y / vr}; }
  __syncthreads();

  for (int it = 0; it < iters; ++it) {
    if (pm == 0.0) { for (int t = tid; t < T; t += BF_NT) z[t] = cd{0.0, 0.0}; return; }
    const double floor_p = 1e-10 * pm;
    // ---- R = sum_t x_t x_t^H / lambda_t
#pragma unroll
    for (int e = 0; e < 2 * NTRI; ++e) acc[e] = 0.0;
    for (int t = tid; t < T; t += BF_NT) {
      const double p = pw[t], w = 1.0 / (p > floor_p ? p : floor_p);
      cd xv[D];
#pragma unroll
      for (int d = 0; d < D; ++d) xv[d] = x[d * cs + t];
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const cd a{w * xv[i].x, w * xv[i].y};
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          acc[2 * bf_tri(i, j)] += a.x * xv[j].x + a.y * xv[j].y;
          acc[2 * bf_tri(i, j) + 1] += a.y * xv[j].x - a.x * xv[j].y;
        }
      }
    }
    bf_block_sum<2 * NTRI>(acc, part, tid);
    // ---- loading, Cholesky R = L L^H (left-looking, in place on the packed triangle), L y = v, L^H u = y: the same arithmetic in every thread
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) tr += acc[2 * bf_tri(i, i)];
    const double load = loading * tr / (double)D;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double dcc = acc[2 * bf_tri(c, c)] + load;
#pragma unroll
      for (int k = 0; k < c; ++k) dcc -= acc[2 * bf_tri(c, k)] * acc[2 * bf_tri(c, k)] + acc[2 * bf_tri(c, k) + 1] * acc[2 * bf_tri(c, k) + 1];
      if (!(dcc > 0.0)) ok = false;
      const double l = sqrt(dcc);
      acc[2 * bf_tri(c, c)] = l;
#pragma unroll
      for (int i = c + 1; i < D; ++i) {
        double sx = acc[2 * bf_tri(i, c)], sy = acc[2 * bf_tri(i, c) + 1];
#pragma unroll
        for (int k = 0; k < c; ++k) {                                                 // L[i][k] conj(L[c][k])
          const double ax = acc[2 * bf_tri(i, k)], ay = acc[2 * bf_tri(i, k) + 1], bx = acc[2 * bf_tri(c, k)], by = acc[2 * bf_tri(c, k) + 1];
          sx -= ax * bx + ay * by; sy -= ay * bx - ax * by;
        }
        acc[2 * bf_tri(i, c)] = sx / l; acc[2 * bf_tri(i, c) + 1] = sy / l;
      }
    }
    if (!ok) { pass_through(); return; }
    cd u[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double sx = v[i].x, sy = v[i].y;
#pragma unroll
      for (int k = 0; k < i; ++k) {                                                   // L[i][k] y_k
        const double ax = acc[2 * bf_tri(i, k)], ay = acc[2 * bf_tri(i, k) + 1];
        sx -= ax * u[k].x - ay * u[k].y; sy -= ax * u[k].y + ay * u[k].x;
      }
      u[i] = cd{sx / acc[2 * bf_tri(i, i)], sy / acc[2 * bf_tri(i, i)]};
    }
#pragma unroll
    for (int i = D - 1; i >= 0; --i) {
      double sx = u[i].x, sy = u[i].y;
#pragma unroll
      for (int k = i + 1; k < D; ++k) {                                               // conj(L[k][i]) u_k
        const double ax = acc[2 * bf_tri(k, i)], ay = acc[2 * bf_tri(k, i) + 1];
        sx -= ax * u[k].x + ay * u[k].y; sy -= ax * u[k].y - ay * u[k].x;
      }
      u[i] = cd{sx / acc[2 * bf_tri(i, i)], sy / acc[2 * bf_tri(i, i)]};
    }
    double qx = 0.0, qy = 0.0;                                                        // v^H u
#pragma unroll
    for (int d = 0; d < D; ++d) { qx += v[d].x * u[d].x + v[d].y * u[d].y; qy += v[d].x * u[d].y - v[d].y * u[d].x; }
    const double q2 = qx * qx + qy * qy;
    if (!(q2 > 0.0) || !isfinite(q2)) { pass_through(); return; }
    cd w[D];                                                                          // conj(w_d), w = u / (v^H u)
#pragma unroll
    for (int d = 0; d < D; ++d) w[d] = cd{(u[d].x * qx + u[d].y * qy) / q2, -(u[d].y * qx - u[d].x * qy) / q2};
    // ---- z_t = w^H x_t, p_t = |z_t|^2 and its maximum
    pm = 0.0;
    for (int t = tid; t < T; t += BF_NT) {
      double zx = 0.0, zy = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) { const cd xv = x[d * cs + t]; zx += w[d].x * xv.x - w[d].y * xv.y; zy += w[d].x * xv.y + w[d].y * xv.x; }
      z[t] = cd{zx, zy};
      const double p = zx * zx + zy * zy;
      pw[t] = p;
      pm = p > pm ? p : pm;
    }
    if (it + 1 < iters) pm = bf_block_max(pm, pmax, tid);
  }
}

template <int D>
void launch_d(const cd* X, cd* Z, double* pw, int rows, int Fq, int T, int ref, int iters, double loading, hipStream_t st) {
  hipLaunchKernelGGL(mpdr_kernel<D>, dim3((unsigned)rows), dim3(BF_NT), 0, st, X, Z, pw, Fq, T, ref, iters, loading);
}

void launch_rows(const cd* X, cd* Z, double* pw, int rows, int Fq, int D, int T, int ref, int iters, double loading, hipStream_t st) {
  switch (D) {
    case 1: launch_d<1>(X, Z, pw, rows, Fq, T, ref, iters, loading, st); break;
    case 2: launch_d<2>(X, Z, pw, rows, Fq, T, ref, iters, loading, st); break;
    case 3: launch_d<3>(X, Z, pw, rows, Fq, T, ref, iters, loading, st); break;
    case 4: launch_d<4>(X, Z, pw, rows, Fq, T, ref, iters, loading, st); break;
    case 5: launch_d<5>(X, Z, pw, rows, Fq, T, ref, iters, loading, st); break;
    case 6: launch_d<6>(X, Z, pw, rows, Fq, T, ref, iters, loading, st); break;
    case 7: launch_d<7>(X, Z, pw, rows, Fq, T, ref, iters, loading, st); break;
    default: launch_d<8>(X, Z, pw, rows, Fq, T, ref, iters, loading, st); break;
  }
}
}  // namespace

bool mpdr_supported(int D) { return D >= 1 && D <= BF_MAXD; }

void launch_mpdr(const double* X, double* Z, double* scratch, int rows, int D, int T, int reference, int iters, double loading, hipStream_t st) {
  launch_rows(reinterpret_cast<const cd*>(X), reinterpret_cast<cd*>(Z), scratch, rows, 1, D, T, reference, iters, loading, st);
}

// STFT -> wpe_mc_kernel -> beamformer -> iSTFT of B rows in the workspace of launch_wpe_mc_dereverb: Y | X | power.  The beamformer reads X and writes
// its (B, 257, T) output over the start of Y, which nothing reads after the WPE kernel.
int launch_wpe_mc_mpdr_dereverb(const float* y, float* out, void* work, int B, int D, int L, int taps, int delay, int wpe_iters, int reference,
                                int bf_iters, double loading, hipStream_t st) {
  const int T = wpe_frames(L);
  const size_t n = (size_t)B * D * BF_WF * T;
  cd* Y = reinterpret_cast<cd*>(work);
  cd* X = Y + n;
  double* pw = reinterpret_cast<double*>(X + n);
  launch_wpe_stft(y, reinterpret_cast<double*>(Y), B * D, L, T, st);
  if (launch_wpe_mc_rows(reinterpret_cast<const double*>(Y), reinterpret_cast<double*>(X), pw, B * BF_WF, BF_WF, D, T, taps, delay, wpe_iters, st)) return 1;
  launch_rows(X, Y, pw, B * BF_WF, BF_WF, D, T, reference, bf_iters, loading, st);
  launch_wpe_istft(reinterpret_cast<const double*>(Y), out, B, L, T, st);
  return 0;
}

}  // namespace buddy
