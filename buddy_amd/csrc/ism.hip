// Room impulse responses of shoebox rooms by the image-source method (buddy_amd/utils/rooms.py; Allen & Berkley 1979; no reference counterpart).
// Definitions in DESIGN.md section 20: per axis an image (m, q) at offset 2 m L + (1 - 2 q) s - r with gain b0^|m - q| b1^|m|; an image triple has the
// distance d, the amplitude A = g / (4 pi d) and the delay tau = d fs / c; h[n] = sum A sinc(x) (1 + cos(pi x / Hw)) / 2, x = n - Hw - tau, |x| < Hw.
//
//   shoebox_rir      one workgroup per (row, tile of ISM_T output samples); the late tiles, whose shells hold the most images, come first in the grid
//
// A tile n0 .. n0 + ISM_T - 1 can only hear the images of the shell d_lo <= d <= d_hi, c (n0 - 2 Hw - 1) / fs and c (n0 + ISM_T) / fs widened by 1e-12.  The
// workgroup walks the (x image, y image, qz) triples inside the outer radius in index order, 256 at a time, one per thread: with rho^2 = X^2 + Y^2 a
// thread solves for the z images whose |Z| lies in [sqrt(d_lo^2 - rho^2), sqrt(d_hi^2 - rho^2)] -- one run of m, or two on either side of a hole -- so
// the work follows the images of the shell and not the lattice.  The runs are supersets (their ends are moved outwards by 1e-9 (1 + |m|)): whether an
// image counts for a sample is decided by |x| < Hw on its delay alone.  A block prefix sum of the run lengths gives every image its place in the
// list; the list goes through LDS ISM_CAP entries at a time (delay, amplitude and the three per-image trigonometric values), and every thread, owner
// of one output sample, walks each chunk in order.  So the terms of a sample are added in the order of (mx, qx, my, qy, qz, mz) ascending, whatever
// the tile's bounds, the batch or the grid: no atomics, and a row's response does not depend on its batch.
//
// Per image: one pow pair for the z gain, one sqrt, sin(pi f) with f = tau - rint(tau) (exact), and cos / sin of pi (tau mod 2 Hw) / Hw.  Per tap:
// sin(pi x) = -(-1)^(k - rint(tau)) sin(pi f) with k = n - Hw, and cos(pi x / Hw) from the angle-sum with the thread's own cos / sin of pi (k mod 2 Hw) / Hw;
// one division.  Everything is double; the sum is rounded once to fp32.
#include "common.h"

namespace buddy {
namespace {
constexpr int ISM_NT = 256;                   // threads per workgroup = output samples per tile (buddy_ism_tile)
constexpr int ISM_T = ISM_NT;
constexpr int ISM_HW = 40;                    // half-width of the fractional-delay kernel (buddy_ism_half_width)
constexpr int ISM_CAP = 1024;                 // images per LDS chunk (buddy_ism_list)
constexpr double ISM_PI = 3.14159265358979323846;

__device__ __forceinline__ long long to_ll(double v) { return (long long)fmin(fmax(v, -1.0e15), 1.0e15); }
__device__ __forceinline__ long long lmin(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long lmax(long long a, long long b) { return a > b ? a : b; }
__device__ __forceinline__ long long labs64(long long a) { return a < 0 ? -a : a; }

// b0^|m - q| b1^|m| with 0^0 = 1 (pow's own convention) and the reflection order |m - q| + |m|
__device__ __forceinline__ double axis_gain(double b0, double b1, long long m, int q, long long* order) {
  const long long e0 = labs64(m - q), e1 = labs64(m);
  *order = e0 + e1;
  return pow(b0, (double)e0) * pow(b1, (double)e1);
}

__device__ bool row_valid(const double* p) {
  bool ok = true;
  for (int i = 0; i < 16; ++i) ok = ok && isfinite(p[i]);
  double d2 = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double L = p[a], s = p[3 + a], r = p[6 + a];
    ok = ok && L > 0.0 && s > 0.0 && s < L && r > 0.0 && r < L;
    d2 += (s - r) * (s - r);
  }
  for (int i = 9; i < 15; ++i) ok = ok && fabs(p[i]) <= 1.0;
  return ok && p[15] > 0.0 && sqrt(d2) >= 0.01;
}

__global__ __launch_bounds__(ISM_NT) void shoebox_rir_kernel(const double* __restrict__ rooms, int fs, int N, int max_order, float* __restrict__ h, long long ldh,
                                                             int* __restrict__ flags) {
  __shared__ double s_tau[ISM_CAP], s_amp[ISM_CAP], s_p[ISM_CAP], s_cb[ISM_CAP], s_sb[ISM_CAP];
  __shared__ long long s_scan[2][ISM_NT];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int tile = (int)gridDim.x - 1 - (int)blockIdx.x;                // late tiles first
  const int n0 = tile * ISM_T, n = n0 + tid;
  double p[16];
  for (int i = 0; i < 16; ++i) p[i] = rooms[(long long)b * 16 + i];
  const bool valid = row_valid(p);                                      // uniform over the workgroup
  if (tile == 0 && tid == 0) flags[b] = valid ? 1 : 0;
  if (!valid) {
    if (n < N) h[(long long)b * ldh + n] = 0.f;
    return;
  }
  const double Lx = p[0], Ly = p[1], Lz = p[2], c = p[15], dfs = (double)fs;
  const double d_hi = c * (double)(n0 + ISM_T) / dfs * (1.0 + 1e-12);
  const double lo_s = (double)(n0 - 2 * ISM_HW - 1);
  const double d_lo = lo_s > 0.0 ? c * lo_s / dfs * (1.0 - 1e-12) : 0.0;
  const double d_hi2 = d_hi * d_hi, d_lo2 = d_lo * d_lo;
  long long Mx = to_ll(floor(d_hi / (2.0 * Lx))) + 1, My = to_ll(floor(d_hi / (2.0 * Ly))) + 1;
  if (max_order >= 0) { Mx = lmin(Mx, (max_order + 1) / 2); My = lmin(My, (max_order + 1) / 2); }
  const long long CX = 2 * (2 * Mx + 1), CY = 2 * (2 * My + 1), P = CX * CY * 2;

  // the thread's own sample: k = n - Hw, its parity, cos / sin of pi (k mod 2 Hw) / Hw
  const int k = n - ISM_HW;
  const int km = ((k % (2 * ISM_HW)) + 2 * ISM_HW) % (2 * ISM_HW);
  const double kd = (double)k, ca = cospi((double)km / (double)ISM_HW), sa = sinpi((double)km / (double)ISM_HW);
  const double sgn_k = (k & 1) ? -1.0 : 1.0;
  double acc = 0.0;

  for (long long p0 = 0; p0 < P; p0 += ISM_NT) {
    // ---- this thread's triple (mx, qx, my, qy, qz) and its runs of mz ----
    const long long pi = p0 + tid;
    long long a_lo = 0, a_n = 0, b_lo = 0, b_n = 0;                     // run A: a_n images from m = a_lo; run B behind it
    double rho2 = 0.0, gxy = 0.0, oz = 0.0;
    long long oxy = 0;
    int qz = 0;
    if (pi < P) {
      qz = (int)(pi & 1);
      const long long iy = (pi >> 1) % CY, ix = (pi >> 1) / CY;
      const long long mx = (ix >> 1) - Mx, my = (iy >> 1) - My;
      const int qx = (int)(ix & 1), qy = (int)(iy & 1);
      const double X = 2.0 * (double)mx * Lx + (double)(1 - 2 * qx) * p[3] - p[6];
      const double Y = 2.0 * (double)my * Ly + (double)(1 - 2 * qy) * p[4] - p[7];
      rho2 = X * X + Y * Y;
      long long ox, oy;
      const double gx = axis_gain(p[9], p[10], mx, qx, &ox);
      const double gy = axis_gain(p[11], p[12], my, qy, &oy);
      gxy = gx * gy;
      oxy = ox + oy;
      oz = (double)(1 - 2 * qz) * p[5] - p[8];
      const long long R = (long long)max_order - oxy;                   // reflections left for z under a cap
      if (rho2 <= d_hi2 && (max_order < 0 || R >= qz)) {
        const double zhi = sqrt(d_hi2 - rho2), zl2 = d_lo2 - rho2, w2 = 2.0 * Lz;
        const double v0 = (-zhi - oz) / w2, v1 = (zhi - oz) / w2;
        long long olo = to_ll(ceil(v0 - 1e-9 * (1.0 + fabs(v0)))), ohi = to_ll(floor(v1 + 1e-9 * (1.0 + fabs(v1))));
        if (max_order >= 0) {                                           // |m - q| + |m| <= R
          const long long qlo = qz ? -((R - 1) / 2) : -(R / 2), qhi = qz ? (R + 1) / 2 : R / 2;
          olo = lmax(olo, qlo); ohi = lmin(ohi, qhi);
        }
        long long hlo = 1, hhi = 0;                                     // the hole: images certainly nearer than d_lo
        if (zl2 > 0.0) {
          const double zlo = sqrt(zl2), u0 = (-zlo - oz) / w2, u1 = (zlo - oz) / w2;
          hlo = to_ll(ceil(u0 + 1e-9 * (1.0 + fabs(u0))));
          hhi = to_ll(floor(u1 - 1e-9 * (1.0 + fabs(u1))));
        }
        if (hlo <= hhi) {
          a_lo = olo; a_n = lmax(lmin(ohi, hlo - 1) - olo + 1, 0);
          b_lo = lmax(olo, hhi + 1); b_n = lmax(ohi - b_lo + 1, 0);
        } else {
          a_lo = olo; a_n = lmax(ohi - olo + 1, 0);
        }
      }
    }
    const long long cnt = a_n + b_n;
    // ---- exclusive prefix sum of the counts over the workgroup ----
    int cur = 0;
    s_scan[0][tid] = cnt;
    __syncthreads();
    for (int off = 1; off < ISM_NT; off <<= 1) {
      s_scan[cur ^ 1][tid] = s_scan[cur][tid] + (tid >= off ? s_scan[cur][tid - off] : 0);
      cur ^= 1;
      __syncthreads();
    }
    const long long total = s_scan[cur][ISM_NT - 1], mine = s_scan[cur][tid] - cnt;
    __syncthreads();                          // the sums have been read before the next batch overwrites them
    // ---- the list, ISM_CAP images at a time ----
    for (long long base = 0; base < total; base += ISM_CAP) {
      const long long j0 = lmax(mine, base), j1 = lmin(mine + cnt, base + ISM_CAP);
      for (long long j = j0; j < j1; ++j) {
        const long long e = j - mine;
        const long long mz = e < a_n ? a_lo + e : b_lo + (e - a_n);
        long long ozr;
        const double gz = axis_gain(p[13], p[14], mz, qz, &ozr);
        const double Z = 2.0 * (double)mz * Lz + oz;
        const double d = sqrt(rho2 + Z * Z);
        const double A = gxy * gz / (4.0 * ISM_PI * d);
        const double tau = d * dfs / c;
        const double rt = rint(tau), f = tau - rt;                      // exact
        const double par = (to_ll(rt) & 1) ? -1.0 : 1.0;
        const double tm = fmod(tau, (double)(2 * ISM_HW)) / (double)ISM_HW;
        const int slot = (int)(j - base);
        s_tau[slot] = tau;
        s_amp[slot] = A;
        s_p[slot] = -A * par * sinpi(f) / ISM_PI;                       // A sin(pi (k - tau)) / pi = (-1)^k s_p
        s_cb[slot] = cospi(tm);
        s_sb[slot] = sinpi(tm);
      }
      __syncthreads();
      const int ne = (int)lmin(total - base, ISM_CAP);
      if (n < N)
        for (int i = 0; i < ne; ++i) {
          const double x = kd - s_tau[i];
          if (fabs(x) < (double)ISM_HW) {
            const double w = 0.5 * (1.0 + (ca * s_cb[i] + sa * s_sb[i]));
            const double t = x == 0.0 ? s_amp[i] : sgn_k * s_p[i] / x;
            acc += t * w;
          }
        }
      __syncthreads();
    }
  }
  if (n < N) h[(long long)b * ldh + n] = (float)acc;
}

// ---- banded rooms: nb sets of wall coefficients and air attenuations over one geometry -------------------------------------
//
//   shoebox_bands    the tiling, the shell enumeration and the prefix-sum list of shoebox_rir; a list entry carries the band-free kernel factors
//                    1 / (4 pi d) and sin(pi f) / (4 pi^2 d) once and the image's NB band gains g_x,k g_y,k g_z,k exp(-air_k d); a tap's value
//                    sinc w / (4 pi d) is computed once and multiplied into NB double accumulators.  ISM_BCAP images per chunk: 5 x 4 KB + 8 x 4 KB
//                    + the 4 KB scan + the coefficients = 56.4 KB of static LDS.
//   band_combine     h[n] = sum_k sum_j bank[k][j] u_k[n - j] in double, k then j ascending, one rounding to fp32; a workgroup owns CMB_T outputs of a
//                    row and stages CMB_J taps and the CMB_T + CMB_J - 1 inputs they meet through LDS.
//
// Gains are integer powers by repeated squaring: b^e costs at most e - 1 roundings whatever the order of the multiplications, 0^0 = 1 and the sign of a
// negative coefficient come out of the products themselves, and no pow call is made (NB x 6 of them per image would dominate the list building).
constexpr int ISM_MAXB = 8;                   // bands per call (buddy_ism_max_bands)
constexpr int ISM_BCAP = 512;                 // images per LDS chunk of the banded list (buddy_ism_band_list)
constexpr int CMB_T = 256;                    // outputs per workgroup of band_combine (buddy_band_combine_tile) = its threads
constexpr int CMB_J = 256;                    // taps per LDS stage of band_combine

__device__ __forceinline__ double ipow(double b, long long e) {
  double r = 1.0;
  while (e > 0) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

__device__ __forceinline__ double axis_gain_int(double b0, double b1, long long m, int q) { return ipow(b0, labs64(m - q)) * ipow(b1, labs64(m)); }

// section 20's test on the row without its own coefficients, then the bands' coefficients and attenuations
__device__ bool band_row_valid(const double* p, const double* beta, const double* air, int nb) {
  bool ok = true;
  for (int i = 0; i < 9; ++i) ok = ok && isfinite(p[i]);
  ok = ok && isfinite(p[15]);
  double d2 = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double L = p[a], s = p[3 + a], r = p[6 + a];
    ok = ok && L > 0.0 && s > 0.0 && s < L && r > 0.0 && r < L;
    d2 += (s - r) * (s - r);
  }
  for (int i = 0; i < 6 * nb; ++i) ok = ok && isfinite(beta[i]) && fabs(beta[i]) <= 1.0;
  if (air)
    for (int k = 0; k < nb; ++k) ok = ok && isfinite(air[k]) && air[k] >= 0.0;
  return ok && p[15] > 0.0 && sqrt(d2) >= 0.01;
}

template <int NB>
__global__ __launch_bounds__(ISM_NT) void shoebox_bands_kernel(const double* __restrict__ rooms, const double* __restrict__ beta, const double* __restrict__ air,
                                                               int fs, int N, int max_order, double* __restrict__ u, long long ldu, int* __restrict__ flags) {
  __shared__ double s_tau[ISM_BCAP], s_amp[ISM_BCAP], s_p[ISM_BCAP], s_cb[ISM_BCAP], s_sb[ISM_BCAP];
  __shared__ double s_g[NB][ISM_BCAP];
  __shared__ long long s_scan[2][ISM_NT];
  __shared__ double s_beta[NB][6], s_air[NB];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int tile = (int)gridDim.x - 1 - (int)blockIdx.x;                // late tiles first
  const int n0 = tile * ISM_T, n = n0 + tid;
  double p[16];
  for (int i = 0; i < 16; ++i) p[i] = rooms[(long long)b * 16 + i];
  const double* rb = beta + (long long)b * NB * 6;
  const double* ra = air ? air + (long long)b * NB : nullptr;
  const bool valid = band_row_valid(p, rb, ra, NB);                     // uniform over the workgroup
  if (tile == 0 && tid == 0) flags[b] = valid ? 1 : 0;
  double* urow = u + (long long)b * NB * ldu;
  if (!valid) {
    if (n < N)
      for (int k = 0; k < NB; ++k) urow[(long long)k * ldu + n] = 0.0;
    return;
  }
  if (tid < NB * 6) s_beta[tid / 6][tid % 6] = rb[tid];
  if (tid < NB) s_air[tid] = ra ? ra[tid] : 0.0;
  __syncthreads();
  const double Lx = p[0], Ly = p[1], Lz = p[2], c = p[15], dfs = (double)fs;
  const double d_hi = c * (double)(n0 + ISM_T) / dfs * (1.0 + 1e-12);
  const double lo_s = (double)(n0 - 2 * ISM_HW - 1);
  const double d_lo = lo_s > 0.0 ? c * lo_s / dfs * (1.0 - 1e-12) : 0.0;
  const double d_hi2 = d_hi * d_hi, d_lo2 = d_lo * d_lo;
  long long Mx = to_ll(floor(d_hi / (2.0 * Lx))) + 1, My = to_ll(floor(d_hi / (2.0 * Ly))) + 1;
  if (max_order >= 0) { Mx = lmin(Mx, (max_order + 1) / 2); My = lmin(My, (max_order + 1) / 2); }
  const long long CX = 2 * (2 * Mx + 1), CY = 2 * (2 * My + 1), P = CX * CY * 2;

  // the thread's own sample: k = n - Hw, its parity, cos / sin of pi (k mod 2 Hw) / Hw
  const int k = n - ISM_HW;
  const int km = ((k % (2 * ISM_HW)) + 2 * ISM_HW) % (2 * ISM_HW);
  const double kd = (double)k, ca = cospi((double)km / (double)ISM_HW), sa = sinpi((double)km / (double)ISM_HW);
  const double sgn_k = (k & 1) ? -1.0 : 1.0;
  double acc[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q) acc[q] = 0.0;

  for (long long p0 = 0; p0 < P; p0 += ISM_NT) {
    // ---- this thread's triple (mx, qx, my, qy, qz) and its runs of mz ----
    const long long pi = p0 + tid;
    long long a_lo = 0, a_n = 0, b_lo = 0, b_n = 0;                     // run A: a_n images from m = a_lo; run B behind it
    double rho2 = 0.0, oz = 0.0;
    long long mx = 0, my = 0;
    int qx = 0, qy = 0, qz = 0;
    if (pi < P) {
      qz = (int)(pi & 1);
      const long long iy = (pi >> 1) % CY, ix = (pi >> 1) / CY;
      mx = (ix >> 1) - Mx; my = (iy >> 1) - My;
      qx = (int)(ix & 1); qy = (int)(iy & 1);
      const double X = 2.0 * (double)mx * Lx + (double)(1 - 2 * qx) * p[3] - p[6];
      const double Y = 2.0 * (double)my * Ly + (double)(1 - 2 * qy) * p[4] - p[7];
      rho2 = X * X + Y * Y;
      const long long oxy = labs64(mx - qx) + labs64(mx) + labs64(my - qy) + labs64(my);
      oz = (double)(1 - 2 * qz) * p[5] - p[8];
      const long long R = (long long)max_order - oxy;                   // reflections left for z under a cap
      if (rho2 <= d_hi2 && (max_order < 0 || R >= qz)) {
        const double zhi = sqrt(d_hi2 - rho2), zl2 = d_lo2 - rho2, w2 = 2.0 * Lz;
        const double v0 = (-zhi - oz) / w2, v1 = (zhi - oz) / w2;
        long long olo = to_ll(ceil(v0 - 1e-9 * (1.0 + fabs(v0)))), ohi = to_ll(floor(v1 + 1e-9 * (1.0 + fabs(v1))));
        if (max_order >= 0) {                                           // |m - q| + |m| <= R
          const long long qlo = qz ? -((R - 1) / 2) : -(R / 2), qhi = qz ? (R + 1) / 2 : R / 2;
          olo = lmax(olo, qlo); ohi = lmin(ohi, qhi);
        }
        long long hlo = 1, hhi = 0;                                     // the hole: images certainly nearer than d_lo
        if (zl2 > 0.0) {
          const double zlo = sqrt(zl2), u0 = (-zlo - oz) / w2, u1 = (zlo - oz) / w2;
          hlo = to_ll(ceil(u0 + 1e-9 * (1.0 + fabs(u0))));
          hhi = to_ll(floor(u1 - 1e-9 * (1.0 + fabs(u1))));
        }
        if (hlo <= hhi) {
          a_lo = olo; a_n = lmax(lmin(ohi, hlo - 1) - olo + 1, 0);
          b_lo = lmax(olo, hhi + 1); b_n = lmax(ohi - b_lo + 1, 0);
        } else {
          a_lo = olo; a_n = lmax(ohi - olo + 1, 0);
        }
      }
    }
    const long long cnt = a_n + b_n;
    double gxy[NB];                                                     // the bands' x and y gains of this triple, only where it has images
    if (cnt > 0) {
#pragma unroll
      for (int q = 0; q < NB; ++q) gxy[q] = axis_gain_int(s_beta[q][0], s_beta[q][1], mx, qx) * axis_gain_int(s_beta[q][2], s_beta[q][3], my, qy);
    }
    // ---- exclusive prefix sum of the counts over the workgroup ----
    int cur = 0;
    s_scan[0][tid] = cnt;
    __syncthreads();
    for (int off = 1; off < ISM_NT; off <<= 1) {
      s_scan[cur ^ 1][tid] = s_scan[cur][tid] + (tid >= off ? s_scan[cur][tid - off] : 0);
      cur ^= 1;
      __syncthreads();
    }
    const long long total = s_scan[cur][ISM_NT - 1], mine = s_scan[cur][tid] - cnt;
    __syncthreads();                          // the sums have been read before the next batch overwrites them
    // ---- the list, ISM_BCAP images at a time ----
    for (long long base = 0; base < total; base += ISM_BCAP) {
      const long long j0 = lmax(mine, base), j1 = lmin(mine + cnt, base + ISM_BCAP);
      for (long long j = j0; j < j1; ++j) {
        const long long e = j - mine;
        const long long mz = e < a_n ? a_lo + e : b_lo + (e - a_n);
        const double Z = 2.0 * (double)mz * Lz + oz;
        const double d = sqrt(rho2 + Z * Z);
        const double A = 1.0 / (4.0 * ISM_PI * d);
        const double tau = d * dfs / c;
        const double rt = rint(tau), f = tau - rt;                      // exact
        const double par = (to_ll(rt) & 1) ? -1.0 : 1.0;
        const double tm = fmod(tau, (double)(2 * ISM_HW)) / (double)ISM_HW;
        const int slot = (int)(j - base);
        s_tau[slot] = tau;
        s_amp[slot] = A;
        s_p[slot] = -A * par * sinpi(f) / ISM_PI;                       // sin(pi (k - tau)) / (4 pi^2 d) = (-1)^k s_p
#pragma unroll
        for (int q = 0; q < NB; ++q) {
          const double g = gxy[q] * axis_gain_int(s_beta[q][4], s_beta[q][5], mz, qz);
          const double a = s_air[q];
          s_g[q][slot] = a > 0.0 ? g * exp(-a * d) : g;
        }
        s_cb[slot] = cospi(tm);
        s_sb[slot] = sinpi(tm);
      }
      __syncthreads();
      const int ne = (int)lmin(total - base, ISM_BCAP);
      if (n < N)
        for (int i = 0; i < ne; ++i) {
          const double x = kd - s_tau[i];
          if (fabs(x) < (double)ISM_HW) {
            const double w = 0.5 * (1.0 + (ca * s_cb[i] + sa * s_sb[i]));
            const double t = x == 0.0 ? s_amp[i] : sgn_k * s_p[i] / x;
            const double v = t * w;                                     // sinc(x) w / (4 pi d): once for all bands
#pragma unroll
            for (int q = 0; q < NB; ++q) acc[q] += v * s_g[q][i];
          }
        }
      __syncthreads();
    }
  }
  if (n < N) {
#pragma unroll
    for (int q = 0; q < NB; ++q) urow[(long long)q * ldu + n] = acc[q];
  }
}

__global__ __launch_bounds__(CMB_T) void band_combine_kernel(const double* __restrict__ u, int nb, long long ldu, int N, const double* __restrict__ bank, int Nh,
                                                             float* __restrict__ h, long long ldh) {
  __shared__ double s_bank[CMB_J], s_u[CMB_T + CMB_J];
  const int tid = threadIdx.x, b = blockIdx.y;
  const long long n0 = (long long)blockIdx.x * CMB_T, n = n0 + tid;
  double acc = 0.0;
  for (int k = 0; k < nb; ++k) {
    const double* uk = u + ((long long)b * nb + k) * ldu;
    for (int j0 = 0; j0 < Nh; j0 += CMB_J) {
      if (n0 + CMB_T - 1 - j0 < 0) break;                               // every input of this and the later stages lies below sample 0 (uniform)
      const int nj = min(CMB_J, Nh - j0);
      if (tid < nj) s_bank[tid] = bank[(long long)k * Nh + j0 + tid];
      // s_u[i] = u_k[n0 - j0 - (CMB_J - 1) + i], i = 0 .. CMB_T + CMB_J - 2: zero below sample 0, and at n >= N (never read by a stored output)
      for (int i = tid; i < CMB_T + CMB_J - 1; i += CMB_T) {
        const long long g = n0 - j0 - (CMB_J - 1) + i;
        s_u[i] = (g >= 0 && g < N) ? uk[g] : 0.0;
      }
      __syncthreads();
      for (int jj = 0; jj < nj; ++jj) acc += s_bank[jj] * s_u[tid + (CMB_J - 1) - jj];
      __syncthreads();
    }
  }
  if (n < N) h[(long long)b * ldh + n] = (float)acc;
}
}  // namespace

int ism_half_width() { return ISM_HW; }
int ism_tile() { return ISM_T; }
int ism_list() { return ISM_CAP; }
int ism_max_bands() { return ISM_MAXB; }
int ism_band_list() { return ISM_BCAP; }
int band_combine_tile() { return CMB_T; }

void launch_shoebox_rir(const double* rooms, int B, int fs, int N, int max_order, float* h, long long ldh, int* flags, hipStream_t st) {
  const unsigned tiles = (unsigned)((N + ISM_T - 1) / ISM_T);
  hipLaunchKernelGGL(shoebox_rir_kernel, dim3(tiles, (unsigned)B), dim3(ISM_NT), 0, st, rooms, fs, N, max_order, h, ldh, flags);
}

namespace {
template <int NB>
void launch_bands_nb(const double* rooms, const double* beta, const double* air, int B, int fs, int N, int max_order, double* u, long long ldu, int* flags,
                     hipStream_t st) {
  const unsigned tiles = (unsigned)((N + ISM_T - 1) / ISM_T);
  hipLaunchKernelGGL(shoebox_bands_kernel<NB>, dim3(tiles, (unsigned)B), dim3(ISM_NT), 0, st, rooms, beta, air, fs, N, max_order, u, ldu, flags);
}
}  // namespace

// nb in 1..ISM_MAXB (checked by the C entry): one instantiation per band count keeps the accumulators in registers
void launch_shoebox_bands(const double* rooms, const double* beta, const double* air, int B, int nb, int fs, int N, int max_order, double* u, long long ldu,
                          int* flags, hipStream_t st) {
  switch (nb) {
    case 1: launch_bands_nb<1>(rooms, beta, air, B, fs, N, max_order, u, ldu, flags, st); break;
    case 2: launch_bands_nb<2>(rooms, beta, air, B, fs, N, max_order, u, ldu, flags, st); break;
    case 3: launch_bands_nb<3>(rooms, beta, air, B, fs, N, max_order, u, ldu, flags, st); break;
    case 4: launch_bands_nb<4>(rooms, beta, air, B, fs, N, max_order, u, ldu, flags, st); break;
    case 5: launch_bands_nb<5>(rooms, beta, air, B, fs, N, max_order, u, ldu, flags, st); break;
    case 6: launch_bands_nb<6>(rooms, beta, air, B, fs, N, max_order, u, ldu, flags, st); break;
    case 7: launch_bands_nb<7>(rooms, beta, air, B, fs, N, max_order, u, ldu, flags, st); break;
    default: launch_bands_nb<8>(rooms, beta, air, B, fs, N, max_order, u, ldu, flags, st); break;
  }
}

void launch_band_combine(const double* u, int B, int nb, long long ldu, int N, const double* bank, int Nh, float* h, long long ldh, hipStream_t st) {
  const unsigned tiles = (unsigned)((N + CMB_T - 1) / CMB_T);
  hipLaunchKernelGGL(band_combine_kernel, dim3(tiles, (unsigned)B), dim3(CMB_T), 0, st, u, nb, ldu, N, bank, Nh, h, ldh);
}

}  // namespace buddy
