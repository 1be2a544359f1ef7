// Winograd-domain batched GEMM in plain f16 (network option gemm = "f16", mode 3: the opt-in fast mode, not the default)
//   M[p][tile][n] = 2^-e[tile] . u_inv[p] . sum_c V16[p][tile][c] . U1[p][n][c]
// V16 = f16_rn(V . 2^e[tile]): ONE f16 term per element of the transformed input, with one power of two per TILE (row of every position's GEMM),
// chosen by the F(6x6,3x3) input transform over that tile's values at all 64 positions and all channels (w6_input_f16_kernel, wino6.hip);
// U1 = f16_rn(U . 2^eu[p]): the hi term of the f16x2 image, one power of two per position.  One v_mfma_f32_32x32x16_f16 per 16 k (a third of f16x2's
// matrix work) with fp32 accumulation; V is read at 2 bytes per element instead of 4 (and written so by the input transform).  Operand format:
// include/buddy_hip.h (buddy_gemm_winograd_domain_f16).
//
// Structure = wgemm_f16x2_rt2_kernel (wgemm.hip): workgroup = 4 waves x 64 rows (two 32-row tiles per wave) x all 128 columns of one column block,
// two workgroups per CU, XCD x owns positions x mod 8, the weights' stage image goes global -> LDS by LDS-DMA (double-buffered, one barrier per
// K-stage), the accumulator tile leaves through a wave-private LDS slab in 256-byte row pieces (those pieces: wgemm_tile.h).  Differences: a K-stage (32 k) of V is 32 bytes per lane
// and row (2 x 16 B of f16 instead of 4 x 16 B of fp32), the weight stage 8 KB; the A operand needs no split: a stage's rows are copied aside and the
// registers reloaded in place for stage s + 1 while stage s multiplies.  A 64-k stage (one barrier
// per 32 instead of 16 MFMAs per wave) needs 64 more VGPRs than two workgroups per CU leave: it spilled.
#include "wgemm_tile.h"
#include <cstdint>
#include <type_traits>

namespace buddy {
namespace {
constexpr int BM = 128, BN = 128, KS = 32, NT = 256;
constexpr int STAGE_BYTES = BN * KS * 2;                      // 8 KB: 2 k-chunks x 4 column blocks x 1 KB

// U fp32 [P][Cout][Cin] -> stage images [P][Cout/128][Cin/32][2 k chunks][4 column blocks][64 lanes] x 16 B (lane: column n = nb * 128 + cb * 32 + lane % 32,
// k = s * 32 + 16 * (lane / 32) + 8 * kc + 0..7), then P inverse scales (floats); one thread per 16-byte element.  The power of two takes the position's
// abs-max into [2^14, 2^15) (pow2_scale, wgemm_tile.h: as the f16x2 image)
__global__ __launch_bounds__(256) void wgemm16_pack_kernel(const float* __restrict__ U, u32x4* __restrict__ out, const unsigned* __restrict__ umax, int P, int Cout,
                                                           int Cin) {
  const long long n16 = (long long)P * Cout * Cin * 2 / 16;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < P) { float s, inv; pow2_scale(umax[i], s, inv); reinterpret_cast<float*>(out + n16)[i] = inv; }
  if (i >= n16) return;
  const int lane = (int)(i & 63);
  long long r = i >> 6;
  const int cb = (int)(r & 3); r >>= 2;
  const int kc = (int)(r & 1); r >>= 1;
  const int S = Cin / KS, NB = Cout / BN;
  const int s = (int)(r % S); r /= S;
  const int nb = (int)(r % NB); r /= NB;
  const int p = (int)r;
  const int n = nb * BN + cb * 32 + (lane & 31), k = s * KS + 16 * (lane >> 5) + 8 * kc;
  const float* src = U + ((long long)p * Cout + n) * Cin + k;
  float sc, inv; pow2_scale(umax[p], sc, inv);
  f16x8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (_Float16)(src[j] * sc);
  out[i] = (u32x4)h;
}

struct Args {
  const _Float16* V; const signed char* vexp; const unsigned char* U1; const float* uinv; float* M;
  int Mt, Cin, Cout, S, NB;                                    // rows per position, K, N, K-stages, column blocks
  int pz, gx;                                                  // pz > 0: positions folded into a 1-D grid (pz positions x gx workgroups), XCD x owns positions x mod 8
  long long sV, sM;                                            // strides between positions (elements)
};

__global__ __launch_bounds__(NT, 2) void wgemm_f16_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[(2 * STAGE_BYTES > 4 * SLAB_BYTES) ? 2 * STAGE_BYTES : 4 * SLAB_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int lid, p;
  xcd_tile_position(a.pz, a.gx, lid, p);
  const int nb = lid % a.NB, m0 = (lid / a.NB) * (2 * BM);
  const char* Vb = reinterpret_cast<const char*>(a.V + (long long)p * a.sV);
  const char* Ub = reinterpret_cast<const char*>(a.U1 + ((long long)p * a.NB + nb) * a.S * STAGE_BYTES);
  const int S = a.S;

  float inv[2];
  unsigned aoff[2];
  {
    const float ui = a.uinv[p];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int row = min(m0 + wid * 64 + t * 32 + (lane & 31), a.Mt - 1);
      inv[t] = __uint_as_float((unsigned)(127 - (int)a.vexp[row]) << 23) * ui;    // 2^-e: e in [-112, 126]
      aoff[t] = (unsigned)(((long long)row * a.Cin + 16 * (lane >> 5)) * 2);
    }
  }
  const unsigned boff = (unsigned)tid * 16u;

  f32x16 acc[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][c][r] = 0.f;

  f16x8 ra[2][2];                                              // [row tile][k chunk]
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)(__attribute__((address_space(3))) char*)smem + wid * 1024);
  auto loadA = [&](int s) {
    const char* base = Vb + (long long)s * (KS * 2);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 2; ++j) ra[t][j] = *reinterpret_cast<const f16x8*>(base + aoff[t] + 16 * j);
  };
  auto dmaB = [&](int s) {
    const void* base = uniform_ptr(Ub + (long long)s * STAGE_BYTES);
    const unsigned l = lds0 + (s & 1) * STAGE_BYTES;
#pragma unroll
    for (int j = 0; j < 2; ++j) glds16(base, boff + j * (NT * 16), l + j * (NT * 16));
  };
  auto stage = [&](int s, auto nx_) {
    constexpr bool NX = decltype(nx_)::value;                  // stage s + 1 exists: request its weights and A rows
    f16x8 av[2][2];                                            // this stage's rows; ra is reloaded in place for stage s + 1
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) av[t][kc] = ra[t][kc];
    if (NX) { dmaB(s + 1); loadA(s + 1); }
    __builtin_amdgcn_sched_barrier(0);
    const unsigned char* Bcur = smem + (s & 1) * STAGE_BYTES + lane * 16;
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      f16x8 b[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) b[cb] = *reinterpret_cast<const f16x8*>(Bcur + (kc * 4 + cb) * FRAG);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[t][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b[cb], av[t][kc], acc[t][cb], 0, 0, 0);
    }
    if (NX) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");    // the two weight DMAs have landed, the four A loads stay in flight
    __syncthreads();
  };
  dmaB(0);
  loadA(0);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  __syncthreads();
  int s = 0;
  for (; s + 1 < S; ++s) stage(s, std::true_type{});
  stage(s, std::false_type{});

  float* St = reinterpret_cast<float*>(smem) + wid * (SLAB_BYTES / 4);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int rb = m0 + wid * 64 + t * 32;
    slab_store<true>(acc[t], inv[t], St, a.M + (long long)p * a.sM + (long long)rb * a.Cout + nb * BN, a.Cout, a.Mt - rb, lane);
  }
}
}  // namespace

bool wgemm_f16_supported(int Cout, int Cin) { return Cout % BN == 0 && Cin % KS == 0 && Cin > 0 && Cout > 0; }    // Cout % 128, Cin % 32
// image = P * Cout * Cin * 2 bytes of stage images + 256 bytes (the positions' inverse scales, floats) + 256 bytes (their abs-max bit patterns); P <= 64
size_t wgemm_f16_packed_bytes(int P, int Cout, int Cin) { return (size_t)P * Cout * Cin * 2 + 512; }
void wgemm_f16_pack_weights(const float* U_dev, void* U1_dev, int P, int Cout, int Cin, hipStream_t st) {
  unsigned* umax_scratch = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(U1_dev) + (size_t)P * Cout * Cin * 2 + 256);
  launch_wgemm_umax(U_dev, umax_scratch, P, (long long)Cout * Cin, st);
  const long long n16 = (long long)P * Cout * Cin * 2 / 16;
  hipLaunchKernelGGL(wgemm16_pack_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, U_dev, reinterpret_cast<u32x4*>(U1_dev), umax_scratch, P, Cout, Cin);
}
void launch_wgemm_f16(const void* V16, const signed char* vexp, const void* U1, float* M, long long Mt, int Cout, int Cin, int P, hipStream_t st) {
  Args a{};
  a.V = reinterpret_cast<const _Float16*>(V16); a.vexp = vexp; a.U1 = reinterpret_cast<const unsigned char*>(U1); a.M = M;
  a.uinv = reinterpret_cast<const float*>(a.U1 + (size_t)P * Cout * Cin * 2);
  a.Mt = (int)Mt; a.Cin = Cin; a.Cout = Cout; a.S = Cin / KS; a.NB = Cout / BN;
  a.sV = Mt * Cin; a.sM = Mt * Cout;
  const dim3 grid = xcd_batched_grid(a, cdiv(Mt, 2 * BM) * a.NB, P);
  hipLaunchKernelGGL(wgemm_f16_kernel, grid, dim3(NT), 0, st, a);
}

}  // namespace buddy
