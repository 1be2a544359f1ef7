// Diffuse late tail of simulated rooms (buddy_amd/utils/rooms.py; no reference counterpart): the image-source response u up to
// a crossover n_x after the direct sound, cross-faded over R samples into Gaussian noise under the exponential envelope of the room's nominal decay,
// level-matched to the energy of u in the fit window [n_f, n_x).  Rows come in groups of D consecutive rows (the microphones of one room) that share
// window, decay and amplitude.  With t_n = (n - Hw) / fs, Hw = buddy_ism_half_width():
//
//   tail_fit   one workgroup of 256 threads per (group, band): E = sum_rows sum_{n_f <= n < n_x} u^2 and S = D sum exp(-2 delta t_n), each thread
//              adding its elements (stride 256, ascending) in double, then the fixed-order workgroup sum of reduce.h; amp = sqrt(E / S) / nu_row.
//   tail_flags one thread per group: 4 where a band's amplitude is zero (E = 0), else 0 -- after tail_fit on the same stream, so no two workgroups
//              write one flag.
//   tail_mix   one thread per four consecutive output samples = one Philox block (normals4), generated once and used for every band:
//              out = u below n_x (the bits of u), cos(th) u + sin(th) amp exp(-delta t_n) z from there, th = (pi / 2) clip((n - n_x + 1/2) / R, 0, 1),
//              u = 0 from n_x + R.  All in double, rounded once to the output's type.  fp32 rows whose bases and strides allow it move as 16-byte
//              vectors.  No atomics; a thread reads and writes its own four samples of its own row only.
#include "../../include/buddy_hip.h"
#include "common.h"
#include "net.h"
#include "philox.h"
#include "reduce.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace buddy;

namespace {

constexpr int TL_T = 256;                     // threads per workgroup; tail_mix covers 4 TL_T samples per workgroup (buddy_tail_tile)
constexpr int TL_MAXD = 8;                    // microphones per group at most: those of buddy_noise_bank
constexpr int TL_ZERO = 4;                    // flag bit 2: a band's fit window holds no energy

typedef float f32x4t __attribute__((ext_vector_type(4)));

template <typename T>
__global__ __launch_bounds__(TL_T) void tail_fit_kernel(const T* __restrict__ u, long long ldr, long long ldk, const int* __restrict__ win,
                                                        const double* __restrict__ delta, const double* __restrict__ nu, int D, int nb, int fs, int Hw,
                                                        double* __restrict__ amp) {
  __shared__ double lds[TL_T / 64][2];
  const int g = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int nf = win[2 * g], W = win[2 * g + 1] - nf;
  const double dl = delta[(long long)g * nb + k];
  double v[2] = {0.0, 0.0};
  const int total = W * D;                    // W <= 2^20 (the host check), D <= 8
  for (int e = tid; e < total; e += TL_T) {
    const int d = e / W, j = e - d * W;
    const double x = (double)u[((long long)g * D + d) * ldr + (long long)k * ldk + nf + j];
    v[0] += x * x;
  }
  for (int j = tid; j < W; j += TL_T) v[1] += exp(-2.0 * dl * ((double)(nf + j - Hw) / (double)fs));
  block_sum<2>(v, lds, tid);
  if (tid == 0) {
    const double A = v[0] > 0.0 ? sqrt(v[0] / ((double)D * v[1])) : 0.0;
    for (int d = 0; d < D; ++d) {
      const long long row = (long long)g * D + d;
      amp[row * nb + k] = nu ? A / nu[row] : A;
    }
  }
}

__global__ __launch_bounds__(TL_T) void tail_flags_kernel(const double* __restrict__ amp, int G, int D, int nb, int* __restrict__ flags) {
  const int g = blockIdx.x * TL_T + threadIdx.x;
  if (g >= G) return;
  int f = 0;
  for (int k = 0; k < nb; ++k)
    if (amp[(long long)g * D * nb + k] == 0.0) f = TL_ZERO;
  flags[g] = f;
}

// grid (tiles of 4 TL_T samples, rows).  VEC: the fp32 form, whose full blocks may move as 16-byte vectors (vin / vout / vz say which arrays allow it)
template <typename T, bool VEC>
__global__ __launch_bounds__(TL_T) void tail_mix_kernel(const T* __restrict__ u, long long ldr, long long ldk, const int* __restrict__ win, int R,
                                                        const double* __restrict__ delta, const double* __restrict__ amp, const float* __restrict__ z,
                                                        long long ldz, const uint32_t* __restrict__ keys, uint32_t purpose, int D, int nb, int fs, int Hw,
                                                        int n, T* __restrict__ out, long long ldor, long long ldok, int vin, int vout, int vz) {
  const int row = blockIdx.y, g = row / D;
  const long long blk = (long long)blockIdx.x * TL_T + threadIdx.x;
  const long long i0 = blk * 4;
  if (i0 >= n) return;
  const long long nx = win[2 * g + 1], ne = nx + R;
  const bool mixes = i0 + 3 >= nx;            // a sample at or after the crossover: the noise and the angles are needed
  float zz[4] = {0.f, 0.f, 0.f, 0.f};
  double cs[4], sn[4], t[4];
  if (mixes) {
    if (z) {
      const float* zr = z + (long long)row * ldz + i0;
      if (VEC && vz && i0 + 4 <= n) {
        const f32x4t q = *reinterpret_cast<const f32x4t*>(zr);
        zz[0] = q.x; zz[1] = q.y; zz[2] = q.z; zz[3] = q.w;
      } else {
        for (int j = 0; j < 4; ++j)
          if (i0 + j < n) zz[j] = zr[j];
      }
    } else {
      normals4(philox4x32_10((uint32_t)blk, 0u, purpose, 0u, keys[2 * row], keys[2 * row + 1]), zz);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double x = fmin(fmax(((double)(i0 + j - nx) + 0.5) / (double)R, 0.0), 1.0);
      const double th = 1.5707963267948966 * x;
      cs[j] = cos(th); sn[j] = sin(th);
      t[j] = (double)(i0 + j - Hw) / (double)fs;
    }
  }
  for (int k = 0; k < nb; ++k) {
    const T* ur = u + (long long)row * ldr + (long long)k * ldk + i0;
    T* o = out + (long long)row * ldor + (long long)k * ldok + i0;
    T v[4];
    if (VEC && vin && i0 + 4 <= ne) {
      const f32x4t q = *reinterpret_cast<const f32x4t*>(ur);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = i0 + j < ne ? ur[j] : (T)0;
    }
    if (mixes) {
      const double a = amp[(long long)row * nb + k], dl = delta[(long long)g * nb + k];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j >= nx) v[j] = (T)(cs[j] * (double)v[j] + sn[j] * (a * exp(-dl * t[j]) * (double)zz[j]));
    }
    if (VEC && vout && i0 + 4 <= n) {
      *reinterpret_cast<f32x4t*>(o) = f32x4t{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < n) o[j] = v[j];
    }
  }
}

// a small device array copied to the host once (after the work queued on the stream), so that a bad value is refused before anything is launched;
// on a host without a HIP device no device pointer exists and the array is read where it lies
template <typename T>
int fetch(const T* dev, long long count, std::vector<T>& host, void* stream, const char* who) {
  host.resize((size_t)count);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    std::memcpy(host.data(), dev, sizeof(T) * (size_t)count);
    return BUDDY_OK;
  }
  hipError_t e = hipMemcpyAsync(host.data(), dev, sizeof(T) * (size_t)count, hipMemcpyDefault, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) { set_error(std::string(who) + ": reading a device array: " + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

// what both entries check: the shape, the strides of u, the windows against the rows of u (n_x + R <= len) and the decays
int check(const char* who, const void* u, int B, int nb, int D, long long ldr, long long ldk, int len, const int* win, int R, const double* delta,
          const double* nu, int fs, void* stream) {
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (!u || !win || !delta) return bad("null pointer");
  if (B < 1 || B > 65535) return bad("B must be in 1..65535");
  if (nb < 1 || nb > buddy_ism_max_bands()) return bad("nb must be in 1..buddy_ism_max_bands()");
  if (D < 1 || D > TL_MAXD) return bad("D must be in 1..8");
  if (B % D != 0) return bad("B must be a multiple of D");
  if (fs < 1000 || fs > 1000000) return bad("fs must be in 1000..1000000");
  if (len < 1 || len > (1 << 20)) return bad("the rows of u must hold 1..2^20 samples");
  if (ldr < len || (nb > 1 && ldk < len)) return bad("a stride of u is below its row length");
  if (R < 0 || R > (1 << 20)) return bad("R must be in 1..2^20");
  const int G = B / D;
  std::vector<int> w;
  std::vector<double> dl, nv;
  int rc = fetch(win, 2LL * G, w, stream, who);
  if (rc == BUDDY_OK) rc = fetch(delta, (long long)G * nb, dl, stream, who);
  if (rc == BUDDY_OK && nu) rc = fetch(nu, (long long)B, nv, stream, who);
  if (rc != BUDDY_OK) return rc;
  for (int g = 0; g < G; ++g) {
    if (w[2 * g] < 0 || w[2 * g] >= w[2 * g + 1]) return bad("a window needs 0 <= n_f < n_x");
    if ((long long)w[2 * g + 1] + R > len) return bad("a window ends beyond the rows of u (n_x + R above their length)");
  }
  for (double v : dl)
    if (!std::isfinite(v)) return bad("a decay is not finite");
  for (double v : nv)
    if (!(std::isfinite(v) && v > 0.0)) return bad("nu must be positive and finite");
  return BUDDY_OK;
}

int launched(const char* who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string(who) + ": kernel launch: " + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int buddy_tail_tile(void) { return 4 * TL_T; }

int buddy_tail_fit(const void* u, int f64, int B, int nb, int D, long long ldr, long long ldk, int len, const int* win, const double* delta, const double* nu,
                   int fs, double* amp, int* flags, void* stream) {
  const char* who = "buddy_tail_fit";
  if (!amp || !flags) { set_error(std::string(who) + ": null pointer"); return BUDDY_ERR_ARG; }
  const int rc = check(who, u, B, nb, D, ldr, ldk, len, win, 0, delta, nu, fs, stream);
  if (rc != BUDDY_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int G = B / D, Hw = buddy_ism_half_width();
  const dim3 grid((unsigned)G, (unsigned)nb);
  if (f64) hipLaunchKernelGGL(tail_fit_kernel<double>, grid, dim3(TL_T), 0, st, (const double*)u, ldr, ldk, win, delta, nu, D, nb, fs, Hw, amp);
  else hipLaunchKernelGGL(tail_fit_kernel<float>, grid, dim3(TL_T), 0, st, (const float*)u, ldr, ldk, win, delta, nu, D, nb, fs, Hw, amp);
  hipLaunchKernelGGL(tail_flags_kernel, dim3((unsigned)((G + TL_T - 1) / TL_T)), dim3(TL_T), 0, st, amp, G, D, nb, flags);
  return launched(who);
}

int buddy_tail_mix(const void* u, int f64, int B, int nb, int D, long long ldr, long long ldk, int len, const int* win, int R, const double* delta,
                   const double* amp, const float* z, long long ldz, const unsigned* keys, unsigned purpose, int fs, int n, void* out, long long ldor,
                   long long ldok, void* stream) {
  const char* who = "buddy_tail_mix";
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (!amp || !out || (!z && !keys)) return bad("null pointer (keys may be null only where z is given)");
  if (R < 1) return bad("R must be in 1..2^20");
  if (n < 1 || n > (1 << 30)) return bad("n must be in 1..2^30");
  if (z && ldz < n) return bad("ldz is below n");
  if ((nb > 1 && ldok < n) || ldor < (long long)(nb - 1) * ldok + n) return bad("a stride of out is below what its rows hold");
  const int rc = check(who, u, B, nb, D, ldr, ldk, len, win, R, delta, nullptr, fs, stream);
  if (rc != BUDDY_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int Hw = buddy_ism_half_width();
  const dim3 grid((unsigned)(((long long)n + 4 * TL_T - 1) / (4 * TL_T)), (unsigned)B);
  if (f64) {
    hipLaunchKernelGGL((tail_mix_kernel<double, false>), grid, dim3(TL_T), 0, st, (const double*)u, ldr, ldk, win, R, delta, amp, z, ldz, keys, purpose, D, nb,
                       fs, Hw, n, (double*)out, ldor, ldok, 0, 0, 0);
  } else {
    const int vin = aligned16(u) && ldr % 4 == 0 && (nb == 1 || ldk % 4 == 0), vout = aligned16(out) && ldor % 4 == 0 && (nb == 1 || ldok % 4 == 0);
    const int vz = z && aligned16(z) && ldz % 4 == 0;
    hipLaunchKernelGGL((tail_mix_kernel<float, true>), grid, dim3(TL_T), 0, st, (const float*)u, ldr, ldk, win, R, delta, amp, z, ldz, keys, purpose, D, nb, fs,
                       Hw, n, (float*)out, ldor, ldok, vin, vout, vz);
  }
  return launched(who);
}

}  // extern "C"
