// Counter-based noise for seeded sampling (include/buddy_hip.h, "per-utterance Philox noise streams"): Philox4x32-10 (Salmon et al., SC'11), one
// block of four 32-bit words per thread.  Sample i of draw d of a stream with key (k0, k1) and purpose p is word i & 3 of the block with counter
// (i >> 2, d, p, 0): a pure function of (key, p, d, i) -- nothing here reads B, n or the row's position in the batch except to find its address.
// HBM-bound on the write side: one 16-byte store per thread, 4 KB per short-lived workgroup (the one-shot form that streams
// fastest for writes); rows whose base is not 16-byte aligned (n % 4 != 0) and the last partial block fall back to per-element stores.
#include "../../include/buddy_hip.h"
#include "common.h"
#include "net.h"
#include "philox.h"

using namespace buddy;

namespace {

typedef float f32x4r __attribute__((ext_vector_type(4)));

// out (R, B, n): row (r, b) = draw draw0 + r of stream b.  grid (blocks of 256 four-sample blocks, R * B rows)
template <int KIND>
__global__ __launch_bounds__(256) void philox_fill_kernel(float* __restrict__ out, int B, int n, const uint32_t* __restrict__ keys, uint32_t purpose,
                                                          uint32_t draw0, int vec) {
  const int row = blockIdx.y, b = row % B;
  const long long blk = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long i0 = blk * 4;
  if (i0 >= n) return;
  const Words q = philox4x32_10((uint32_t)blk, draw0 + (uint32_t)(row / B), purpose, 0u, keys[2 * b], keys[2 * b + 1]);
  float v[4];
  if (KIND == 0) normals4(q, v);
  else if (KIND == 1) { for (int j = 0; j < 4; ++j) v[j] = (float)(q.w[j] >> 8) * 0x1p-24f; }
  else { for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(q.w[j]); }
  float* o = out + (long long)row * n + i0;
  if (vec && i0 + 4 <= n) {
    *reinterpret_cast<f32x4r*>(o) = f32x4r{v[0], v[1], v[2], v[3]};
  } else {
    for (int j = 0; j < 4; ++j)
      if (i0 + j < n) o[j] = v[j];
  }
}

// out[b][i] = x[b][i] + scale * eps[b][i], eps = the normals of purpose 0, draw `draw` of stream b, never stored.  The update is written as
// perturb_kernel (sampler.hip) writes it, on a value that is complete before it is used, so both contract to the same fused multiply-add.
__global__ __launch_bounds__(256) void perturb_philox_kernel(const float* __restrict__ x, const uint32_t* __restrict__ keys, uint32_t draw, float scale,
                                                             float* __restrict__ out, int L, int vec) {
  const int b = blockIdx.y;
  const long long blk = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long i0 = blk * 4;
  if (i0 >= L) return;
  const Words q = philox4x32_10((uint32_t)blk, draw, 0u, 0u, keys[2 * b], keys[2 * b + 1]);
  float eps[4];
  normals4(q, eps);
  const float* xr = x + (long long)b * L + i0;
  float* o = out + (long long)b * L + i0;
  if (vec && i0 + 4 <= L) {
    const f32x4r xv = *reinterpret_cast<const f32x4r*>(xr);
    f32x4r r;
    r.x = xv.x + scale * eps[0]; r.y = xv.y + scale * eps[1]; r.z = xv.z + scale * eps[2]; r.w = xv.w + scale * eps[3];
    *reinterpret_cast<f32x4r*>(o) = r;
  } else {
    for (int j = 0; j < 4; ++j)
      if (i0 + j < L) o[j] = xr[j] + scale * eps[j];
  }
}

int launched() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string("kernel launch: ") + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int buddy_philox_fill(float* out, int R, int B, int n, const unsigned* keys, unsigned purpose, unsigned draw0, int kind, void* stream) {
  if (!out || !keys || R < 1 || B < 1 || n < 1 || kind < 0 || kind > 2) { set_error("philox_fill: bad arguments (kind 0 normal, 1 uniform, 2 raw words)"); return BUDDY_ERR_ARG; }
  if ((long long)R * B > 65535) { set_error("philox_fill: more than 65535 rows"); return BUDDY_ERR_ARG; }
  const int vec = (n % 4 == 0) && aligned16(out);
  const dim3 grid((unsigned)(((long long)n + 1023) / 1024), (unsigned)(R * B));
  hipStream_t st = (hipStream_t)stream;
  if (kind == 0) philox_fill_kernel<0><<<grid, dim3(256), 0, st>>>(out, B, n, keys, purpose, draw0, vec);
  else if (kind == 1) philox_fill_kernel<1><<<grid, dim3(256), 0, st>>>(out, B, n, keys, purpose, draw0, vec);
  else philox_fill_kernel<2><<<grid, dim3(256), 0, st>>>(out, B, n, keys, purpose, draw0, vec);
  return launched();
}

int buddy_perturb_philox(const float* x, const unsigned* keys, unsigned draw, float scale, float* out, int B, int L, void* stream) {
  if (!x || !keys || !out || B < 1 || L < 1) { set_error("perturb_philox: bad arguments"); return BUDDY_ERR_ARG; }
  if (B > 65535) { set_error("perturb_philox: more than 65535 rows"); return BUDDY_ERR_ARG; }
  const int vec = (L % 4 == 0) && aligned16(x) && aligned16(out);
  const dim3 grid((unsigned)(((long long)L + 1023) / 1024), (unsigned)B);
  perturb_philox_kernel<<<grid, dim3(256), 0, (hipStream_t)stream>>>(x, keys, draw, scale, out, L, vec);
  return launched();
}

}  // extern "C"
