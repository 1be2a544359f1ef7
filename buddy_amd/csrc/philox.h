// Philox4x32-10 (Salmon et al., SC'11) and the Box-Muller map of the per-utterance noise streams (include/buddy_hip.h, "per-utterance Philox noise
// streams"), shared by every kernel that draws them (rng.hip, noise.hip): sample i of draw d of purpose p of the stream with
// key (k0, k1) is word i & 3 of the block with counter (i >> 2, d, p, 0).  One definition, so that a kernel that generates its normals where it
// consumes them gets the bits buddy_philox_fill stores.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace buddy {

struct Words { uint32_t w[4]; };

__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  return Words{{c0, c1, c2, c3}};
}

// Box-Muller of one word pair.  u1 = (k + 0.5) 2^-24 with k = w_even >> 8 needs 25 bits once k >= 2^23, so -log(u1) is taken from whichever of
// u1 and 1 - u1 = (2^24 - 1 - k + 0.5) 2^-24 is exact in fp32 (logf below one half, log1pf above): the logarithm's argument is never rounded.
// The angle 2 u2 (u2 = (w_odd >> 8) 2^-24) is exact too, and sincospif takes it in half-turns.  Largest radius sqrt(50 ln 2) = 5.887, no NaN / inf.
__device__ __forceinline__ void box_muller(uint32_t we, uint32_t wo, float& ze, float& zo) {
  const uint32_t k = we >> 8;
  float nl;
  if (k < (1u << 23)) nl = -logf(((float)k + 0.5f) * 0x1p-24f);
  else nl = -log1pf(-(((float)(0xFFFFFFu - k) + 0.5f) * 0x1p-24f));
  const float r = sqrtf(2.0f * nl);
  float s, c;
  sincospif((float)(wo >> 8) * 0x1p-23f, &s, &c);
  ze = r * c; zo = r * s;
}

__device__ __forceinline__ void normals4(const Words& q, float z[4]) {
  box_muller(q.w[0], q.w[1], z[0], z[1]);
  box_muller(q.w[2], q.w[3], z[2], z[3]);
}

}  // namespace buddy
