// The optimizer step of training on flat fp32 buffers (include/buddy_hip.h, "the optimizer step of training"): the global gradient norm as a
// deterministic two-stage double reduction, and clip + Adam + EMA as one streaming pass.  HBM-bound: 36 bytes per parameter (p, g, m, v, ema read;
// p, m, v, ema written), one 16-byte word per array and thread, 4 KB per array and short-lived workgroup (the form that
// streams fastest on this part), non-temporal loads for g, which is read once and not needed again.
#include "../../include/buddy_hip.h"
#include "common.h"
#include "net.h"

#include <cmath>

using namespace buddy;

namespace {

typedef float f32x4o __attribute__((ext_vector_type(4)));
constexpr int SQ_THREADS = 256, SQ_WORDS = 16;                  // 256 threads x 16 float4 = 16384 floats = 64 KB per workgroup
constexpr long long SQ_CHUNK = (long long)SQ_THREADS * SQ_WORDS * 4;
constexpr int MAX_FROZEN = 8;

// the 256 per-thread doubles of a workgroup in a fixed order: lanes of a wave by shuffle (64 -> 1), then the four waves in wave order
__device__ __forceinline__ double block_sum_256(double s, double* lds) {
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = s;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ __launch_bounds__(SQ_THREADS) void optim_sqnorm_part_kernel(const float* __restrict__ g, long long n, int aligned, double* __restrict__ partials) {
  __shared__ double lds[4];
  const long long base = (long long)blockIdx.x * SQ_CHUNK;
  double s = 0.0;
#pragma unroll 4
  for (int u = 0; u < SQ_WORDS; ++u) {
    const long long i = base + ((long long)u * SQ_THREADS + threadIdx.x) * 4;
    if (aligned && i + 4 <= n) {
      const f32x4o w = __builtin_nontemporal_load(reinterpret_cast<const f32x4o*>(g + i));
      const double a = w.x, b = w.y, c = w.z, d = w.w;
      s += a * a; s += b * b; s += c * c; s += d * d;      // squares of floats are exact in double: only the additions round
    } else {
      for (int k = 0; k < 4; ++k)
        if (i + k < n) { const double a = g[i + k]; s += a * a; }
    }
  }
  s = block_sum_256(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(SQ_THREADS) void optim_sqnorm_final_kernel(const double* __restrict__ partials, long long chunks, double* __restrict__ out) {
  __shared__ double lds[4];
  double s = 0.0;
  for (long long c = threadIdx.x; c < chunks; c += SQ_THREADS) s += partials[c];
  s = block_sum_256(s, lds);
  if (threadIdx.x == 0) out[0] = s;
}

// ---- the replica checksum: sum_i bits(x[i]) * (2 i + 1) mod 2^64, the same streaming form as the squared norm (plain loads: the buffers it
// reads -- p, m, v, ema -- are read again by the next step)
typedef unsigned int u32x4o __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

// the 256 per-thread sums of a workgroup; integer addition mod 2^64 is associative, so the order does not matter
__device__ __forceinline__ u64 block_sum_256_u64(u64 s, u64* lds) {
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = s;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ __launch_bounds__(SQ_THREADS) void optim_checksum_part_kernel(const unsigned int* __restrict__ x, long long n, int aligned, u64* __restrict__ partials) {
  __shared__ u64 lds[4];
  const long long base = (long long)blockIdx.x * SQ_CHUNK;
  u64 s = 0;
#pragma unroll 4
  for (int u = 0; u < SQ_WORDS; ++u) {
    const long long i = base + ((long long)u * SQ_THREADS + threadIdx.x) * 4;
    const u64 k = 2ull * (u64)i + 1ull;
    if (aligned && i + 4 <= n) {
      const u32x4o w = *reinterpret_cast<const u32x4o*>(x + i);
      s += (u64)w.x * k; s += (u64)w.y * (k + 2); s += (u64)w.z * (k + 4); s += (u64)w.w * (k + 6);
    } else {
      for (int j = 0; j < 4; ++j)
        if (i + j < n) s += (u64)x[i + j] * (k + 2ull * j);
    }
  }
  s = block_sum_256_u64(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(SQ_THREADS) void optim_checksum_final_kernel(const u64* __restrict__ partials, long long chunks, u64* __restrict__ out) {
  __shared__ u64 lds[4];
  u64 s = 0;
  for (long long c = threadIdx.x; c < chunks; c += SQ_THREADS) s += partials[c];
  s = block_sum_256_u64(s, lds);
  if (threadIdx.x == 0) out[0] = s;
}

struct Frozen { long long lo[MAX_FROZEN], hi[MAX_FROZEN]; int n; };

struct StepArgs {
  float* p; const float* g; float* m; float* v; float* ema; long long n;
  const double* sqnorm; double max_norm, beta1, beta2, eps, step_size, bias2_sqrt, ema_s, grad_scale;
};

__device__ __forceinline__ bool is_frozen(const Frozen& fz, long long i) {
  bool f = false;
  for (int r = 0; r < fz.n; ++r) f = f || (i >= fz.lo[r] && i < fz.hi[r]);
  return f;
}

// one element: returns through the references; frozen elements keep p, m, v bit for bit and still feed the EMA
__device__ __forceinline__ void step_one(const StepArgs& a, double coef, bool frozen, float& p, float g, float& m, float& v, float& e) {
  if (!frozen) {
    const double gc = coef * (double)g;
    m = (float)(a.beta1 * (double)m + (1.0 - a.beta1) * gc);
    v = (float)(a.beta2 * (double)v + (1.0 - a.beta2) * gc * gc);
    const double denom = sqrt((double)v) / a.bias2_sqrt + a.eps;
    p = (float)((double)p - a.step_size * ((double)m / denom));
  }
  if (a.ema) e = (float)((double)e * a.ema_s + (double)p * (1.0 - a.ema_s));
}

__global__ __launch_bounds__(256) void optim_step_kernel(StepArgs a, Frozen fz) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= a.n) return;
  // grad_scale: g holds a sum over ranks and the step uses its average; the clip acts on the norm of the average.  grad_scale = 1 multiplies
  // by one twice, which is exact: the bits of the unscaled step
  double coef = 1.0;
  if (a.max_norm > 0.0) coef = fmin(1.0, a.max_norm / (a.grad_scale * sqrt(a.sqnorm[0]) + 1e-6));
  coef *= a.grad_scale;
  if (i + 4 <= a.n) {
    const f32x4o pw = *reinterpret_cast<const f32x4o*>(a.p + i);
    const f32x4o gw = __builtin_nontemporal_load(reinterpret_cast<const f32x4o*>(a.g + i));
    const f32x4o mw = *reinterpret_cast<const f32x4o*>(a.m + i);
    const f32x4o vw = *reinterpret_cast<const f32x4o*>(a.v + i);
    f32x4o ew = {0.f, 0.f, 0.f, 0.f};
    if (a.ema) ew = *reinterpret_cast<const f32x4o*>(a.ema + i);
    float p[4] = {pw.x, pw.y, pw.z, pw.w}, m[4] = {mw.x, mw.y, mw.z, mw.w}, v[4] = {vw.x, vw.y, vw.z, vw.w}, e[4] = {ew.x, ew.y, ew.z, ew.w};
    const float g[4] = {gw.x, gw.y, gw.z, gw.w};
    bool all = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool fr = is_frozen(fz, i + k);
      all = all && fr;
      step_one(a, coef, fr, p[k], g[k], m[k], v[k], e[k]);
    }
    if (!all) {            // a word that lies wholly inside a frozen range is not written at all
      *reinterpret_cast<f32x4o*>(a.p + i) = f32x4o{p[0], p[1], p[2], p[3]};
      *reinterpret_cast<f32x4o*>(a.m + i) = f32x4o{m[0], m[1], m[2], m[3]};
      *reinterpret_cast<f32x4o*>(a.v + i) = f32x4o{v[0], v[1], v[2], v[3]};
    }
    if (a.ema) *reinterpret_cast<f32x4o*>(a.ema + i) = f32x4o{e[0], e[1], e[2], e[3]};
  } else {                 // the last, partial word of an n that is no multiple of 4
    for (long long j = i; j < a.n; ++j) {
      float p = a.p[j], m = a.m[j], v = a.v[j], e = a.ema ? a.ema[j] : 0.f;
      const bool fr = is_frozen(fz, j);
      step_one(a, coef, fr, p, a.g[j], m, v, e);
      if (!fr) { a.p[j] = p; a.m[j] = m; a.v[j] = v; }
      if (a.ema) a.ema[j] = e;
    }
  }
}

__global__ __launch_bounds__(256) void optim_ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long long n, double s) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 4 <= n) {
    f32x4o e = *reinterpret_cast<const f32x4o*>(ema + i);
    const f32x4o w = *reinterpret_cast<const f32x4o*>(p + i);
    e.x = (float)((double)e.x * s + (double)w.x * (1.0 - s));
    e.y = (float)((double)e.y * s + (double)w.y * (1.0 - s));
    e.z = (float)((double)e.z * s + (double)w.z * (1.0 - s));
    e.w = (float)((double)e.w * s + (double)w.w * (1.0 - s));
    *reinterpret_cast<f32x4o*>(ema + i) = e;
  } else {
    for (long long j = i; j < n; ++j) ema[j] = (float)((double)ema[j] * s + (double)p[j] * (1.0 - s));
  }
}

int launched() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string("kernel launch: ") + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

bool misaligned(const void* q) { return ((uintptr_t)q & 15) != 0; }

}  // namespace

extern "C" {

long long buddy_optim_sqnorm_chunk(void) { return SQ_CHUNK; }

int buddy_optim_sqnorm(const float* g, long long n, double* partials, double* out, void* stream) {
  if (!g || !partials || !out || n < 1) { set_error("optim_sqnorm: null argument or n < 1"); return BUDDY_ERR_ARG; }
  if (((uintptr_t)g & 3) || ((uintptr_t)partials & 7) || ((uintptr_t)out & 7)) { set_error("optim_sqnorm: misaligned buffer"); return BUDDY_ERR_ARG; }
  const long long chunks = (n + SQ_CHUNK - 1) / SQ_CHUNK;
  if (chunks > 0x7fffffffLL) { set_error("optim_sqnorm: n too large"); return BUDDY_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  optim_sqnorm_part_kernel<<<dim3((unsigned)chunks), dim3(SQ_THREADS), 0, st>>>(g, n, misaligned(g) ? 0 : 1, partials);
  optim_sqnorm_final_kernel<<<dim3(1), dim3(SQ_THREADS), 0, st>>>(partials, chunks, out);
  return launched();
}

int buddy_optim_checksum(const float* x, long long n, unsigned long long* partials, unsigned long long* out, void* stream) {
  if (!x || !partials || !out || n < 1) { set_error("optim_checksum: null argument or n < 1"); return BUDDY_ERR_ARG; }
  if (((uintptr_t)x & 3) || ((uintptr_t)partials & 7) || ((uintptr_t)out & 7)) { set_error("optim_checksum: misaligned buffer"); return BUDDY_ERR_ARG; }
  const long long chunks = (n + SQ_CHUNK - 1) / SQ_CHUNK;
  if (chunks > 0x7fffffffLL) { set_error("optim_checksum: n too large"); return BUDDY_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  optim_checksum_part_kernel<<<dim3((unsigned)chunks), dim3(SQ_THREADS), 0, st>>>(reinterpret_cast<const unsigned int*>(x), n, misaligned(x) ? 0 : 1, partials);
  optim_checksum_final_kernel<<<dim3(1), dim3(SQ_THREADS), 0, st>>>(partials, chunks, out);
  return launched();
}

int buddy_optim_step(float* p, const float* g, float* m, float* v, float* ema, long long n, const double* sqnorm, double max_norm, double beta1,
                     double beta2, double eps, double step_size, double bias2_sqrt, double ema_s, const long long* frozen, int n_frozen,
                     void* stream) {
  return buddy_optim_step_scaled(p, g, m, v, ema, n, sqnorm, max_norm, beta1, beta2, eps, step_size, bias2_sqrt, ema_s, 1.0, frozen, n_frozen, stream);
}

int buddy_optim_step_scaled(float* p, const float* g, float* m, float* v, float* ema, long long n, const double* sqnorm, double max_norm,
                            double beta1, double beta2, double eps, double step_size, double bias2_sqrt, double ema_s, double grad_scale,
                            const long long* frozen, int n_frozen, void* stream) {
  if (!(std::isfinite(grad_scale) && grad_scale > 0.0)) { set_error("optim_step: grad_scale must be finite and > 0"); return BUDDY_ERR_ARG; }
  if (!p || !g || !m || !v || n < 1) { set_error("optim_step: null argument or n < 1"); return BUDDY_ERR_ARG; }
  if (misaligned(p) || misaligned(g) || misaligned(m) || misaligned(v) || misaligned(ema)) { set_error("optim_step: buffers must be 16-byte aligned"); return BUDDY_ERR_ARG; }
  if (max_norm > 0.0 && (!sqnorm || ((uintptr_t)sqnorm & 7))) { set_error("optim_step: max_norm > 0 needs the device double of buddy_optim_sqnorm"); return BUDDY_ERR_ARG; }
  if (n_frozen < 0 || n_frozen > MAX_FROZEN || (n_frozen > 0 && !frozen)) { set_error("optim_step: at most 8 frozen ranges"); return BUDDY_ERR_ARG; }
  if (!(bias2_sqrt > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !std::isfinite(step_size) ||
      !(ema_s >= 0.0 && ema_s <= 1.0)) { set_error("optim_step: bad hyper-parameter"); return BUDDY_ERR_ARG; }
  Frozen fz; fz.n = n_frozen;
  for (int r = 0; r < MAX_FROZEN; ++r) { fz.lo[r] = 0; fz.hi[r] = 0; }
  for (int r = 0; r < n_frozen; ++r) {
    fz.lo[r] = frozen[2 * r]; fz.hi[r] = frozen[2 * r + 1];
    if (fz.lo[r] < 0 || fz.hi[r] > n || fz.lo[r] > fz.hi[r]) { set_error("optim_step: frozen range outside [0, n)"); return BUDDY_ERR_ARG; }
  }
  const long long words = (n + 3) / 4, blocks = (words + 255) / 256;
  if (blocks > 0x7fffffffLL) { set_error("optim_step: n too large"); return BUDDY_ERR_ARG; }
  StepArgs a{p, g, m, v, ema, n, max_norm > 0.0 ? sqnorm : nullptr, max_norm, beta1, beta2, eps, step_size, bias2_sqrt, ema_s, grad_scale};
  optim_step_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(a, fz);
  return launched();
}

int buddy_optim_ema(float* ema, const float* p, long long n, double ema_s, void* stream) {
  if (!ema || !p || n < 1 || misaligned(ema) || misaligned(p) || !(ema_s >= 0.0 && ema_s <= 1.0)) { set_error("optim_ema: bad arguments"); return BUDDY_ERR_ARG; }
  const long long words = (n + 3) / 4, blocks = (words + 255) / 256;
  if (blocks > 0x7fffffffLL) { set_error("optim_ema: n too large"); return BUDDY_ERR_ARG; }
  optim_ema_kernel<<<dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream>>>(ema, p, n, ema_s);
  return launched();
}

}  // extern "C"
