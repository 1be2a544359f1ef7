// What the matrix-pipe GEMM kernels of wgemm.hip and wgemm16.hip share (private to those two files): the vector types, the LDS-DMA instruction, the
// power-of-two scale of an abs-max, the XCD-aware workgroup order with its launch geometry, and how an accumulator tile leaves a wave.
#pragma once
#include "common.h"

namespace buddy {
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int FRAG = 1024;                                    // bytes of one MFMA operand fragment block in a stage image: 64 lanes x 16 B

// LDS-DMA of 16 bytes per lane as inline asm: source = uniform 64-bit base (SGPR pair) + a 32-bit per-lane byte offset, LDS destination = M0 + 16 * lane
__device__ __forceinline__ void glds16(const void* sbase, unsigned voff, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_addr) : "memory");
}
__device__ __forceinline__ const void* uniform_ptr(const void* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (const void*)(((unsigned long long)hi << 32) | lo);
}

// the power of two that takes an abs-max (float bits) into [2^14, 2^15), and its inverse; exponent fields outside [15, 253] are clamped (zero / tiny / huge
// tensors: the scale stays a finite normal number)
__device__ __forceinline__ void pow2_scale(unsigned bits, float& s, float& inv) {
  int e = (int)((bits >> 23) & 0xFF);
  e = e < 15 ? 15 : (e > 253 ? 253 : e);
  s = __uint_as_float((unsigned)(268 - e) << 23);
  inv = __uint_as_float((unsigned)(e - 14) << 23);
}
// abs-max of every one of P weight matrices of `per` floats (a multiple of 4) -> umax[p] (float bits), zeroed here first (wgemm.hip)
void launch_wgemm_umax(const float* U_dev, unsigned* umax, int P, long long per, hipStream_t st);

// ---- XCD-aware workgroup order
// The hardware places workgroup b of the flattened grid on XCD b % 8, each XCD with its own L2.
// 1-D form: the logical tile of workgroup `orig` of `nwg`, such that each XCD gets a contiguous range of logical tiles.
__device__ __forceinline__ int xcd_tile(int orig, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7, k = orig >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}
// Batched form: logical tile `lid` and position `p` of this workgroup.  Positions a multiple of 8 are folded into a 1-D grid of pz positions x gx
// workgroups each (pz > 0): XCD x takes the positions x, x + 8, ... and walks all their tiles, so a position's weight panel is fetched into ONE L2
// instead of all eight.  Otherwise blockIdx.z is the position and the tiles go by the 1-D form.
__device__ __forceinline__ void xcd_tile_position(int pz, int gx, int& lid, int& p) {
  if (pz > 0) {
    const int orig = blockIdx.x, xcd = orig & 7, k = orig >> 3;     // k-th workgroup of this XCD: gx * pz / 8 of them
    lid = k % gx; p = xcd + 8 * (k / gx);
  } else {
    lid = xcd_tile(blockIdx.x, gridDim.x);
    p = blockIdx.z;
  }
}
// its host side: the grid of a batched launch of P positions x gx workgroups, and the kernel arguments pz / gx that xcd_tile_position reads
template <class A>
inline dim3 xcd_batched_grid(A& a, int gx, int P) {
  const bool fold = P % 8 == 0 && (long long)gx * P < (1LL << 31);
  a.pz = fold ? P : 0; a.gx = gx;
  return dim3(fold ? (unsigned)(gx * P) : (unsigned)gx, 1, fold ? 1u : (unsigned)P);
}

// ---- the slab-transpose store
// The accumulator is C^T (weights as the MFMA's first operand): lane (row = lane & 31, h = lane >> 5) holds channels 8 g + 4 h + 0..3 of each 32-channel
// block of ONE row.  A 32-row x 128-column tile leaves in two halves of 64 columns through a wave-private LDS slab (the weight buffers are free after the
// last stage) so that a lane owns 16-byte pieces of 256-byte ROW pieces (16 lanes per row: whole cache lines per instruction; in MFMA order a lane pair
// covers 32 bytes of 32 rows, +0.3 ... 1.9 % slower).
constexpr int SLAB_SP = 68;                                   // floats per staged row (64 columns + 4: conflict-free 16-byte writes down a column)
constexpr int SLAB_BYTES = 32 * SLAB_SP * 4;                  // one wave's slab
// half hb of the tile, (SCALE) times the row's scale, into the slab St; afterwards lane (rr = lane >> 4, c4 = 4 * (lane & 15)) reads row 4 it + rr at St +
// (4 it + rr) * SLAB_SP + c4, and ends with slab_done before the next half is written
template <bool SCALE>
__device__ __forceinline__ void slab_write(const f32x16 (&acc)[4], const float inv, const int hb, float* St, const int lane) {
#pragma unroll
  for (int cl = 0; cl < 2; ++cl)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x16& c = acc[2 * hb + cl];
      *reinterpret_cast<float4*>(St + (lane & 31) * SLAB_SP + cl * 32 + 8 * g + 4 * (lane >> 5)) =
          SCALE ? make_float4(c[4 * g] * inv, c[4 * g + 1] * inv, c[4 * g + 2] * inv, c[4 * g + 3] * inv) : make_float4(c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]);
    }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void slab_done() {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// the whole tile to Mrow (the tile's first row and column; row stride ld floats), rows < nrows only
template <bool SCALE>
__device__ __forceinline__ void slab_store(const f32x16 (&acc)[4], const float inv, float* St, float* Mrow, const long long ld, const int nrows, const int lane) {
  const int rr = lane >> 4, c4 = (lane & 15) * 4;
#pragma unroll
  for (int hb = 0; hb < 2; ++hb) {
    slab_write<SCALE>(acc, inv, hb, St, lane);
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int r = 4 * it + rr;
      const float4 v = *reinterpret_cast<const float4*>(St + r * SLAB_SP + c4);
      if (r < nrows) *reinterpret_cast<float4*>(Mrow + (long long)r * ld + hb * 64 + c4) = v;
    }
    slab_done();
  }
}

}  // namespace buddy
