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
}  // namespace

int ism_half_width() { return ISM_HW; }
int ism_tile() { return ISM_T; }
int ism_list() { return ISM_CAP; }

void launch_shoebox_rir(const double* rooms, int B, int fs, int N, int max_order, float* h, long long ldh, int* flags, hipStream_t st) {
  const unsigned tiles = (unsigned)((N + ISM_T - 1) / ISM_T);
  hipLaunchKernelGGL(shoebox_rir_kernel, dim3(tiles, (unsigned)B), dim3(ISM_NT), 0, st, rooms, fs, N, max_order, h, ldh, flags);
}

}  // namespace buddy
