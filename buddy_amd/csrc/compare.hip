// Paired comparison of two runs (buddy_amd/utils/compare.py; no reference counterpart): the resampling behind the bootstrap
// intervals and the sign-flip randomisation test of a column of paired differences.  A call holds C ragged columns (C, ld) with lens (C,); column c
// draws from the Philox stream keys[c] only, so its bits depend on its own data, length, key and draw0 and on nothing else in the call.
//
//   boot      one workgroup of 256 threads per (resample, column).  A thread takes Philox blocks (stride 256): word q of block i is sample j = 4 i + q
//             of draw draw0 + r of purpose 11, and rank (w n) >> 32 of the SORTED column gets one more count -- integer LDS atomics, whose result
//             has no order.  Mean: thread t adds cnt[k] s[k] over k = t, t + 256, ... ascending in double, then the fixed-order workgroup sum of
//             reduce.h, / n.  Median: each thread owns CH consecutive counters (CH odd: conflict-free LDS strides), a workgroup scan of the CH-sums
//             gives every thread the count before its chunk, and the thread whose chunk holds sorted position (n - 1) / 2 (and n / 2) walks to it.
//   select    one workgroup per (rank, row): the 8-bit radix select of select.h on the order-preserving 64-bit key of a double.  After eight
//             passes the key is the element: exact for any R, no copy of the row.
//   signflip  one thread per pattern: T = sum_j (+-) d[j], j ascending, one accumulator in double (the signs are applied by negation: no product,
//             nothing to contract).  Random columns take bit j & 31 of sample j >> 5 of draw draw0 + r of purpose 12 (one Philox block per 128
//             elements), exhaustive columns bit j of r.  Pattern 0 of the first workgroup also runs the same loop with all signs + into tobs.
//   count     one workgroup per column: #{r < m : |T[r]| >= thr} in 64-bit integers.
#include "../../include/buddy_hip.h"
#include "common.h"
#include "net.h"
#include "philox.h"
#include "reduce.h"
#include "select.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace buddy;

namespace {

constexpr int CP_T = 256;                     // threads per workgroup
constexpr int CP_MAXN = 8192;                 // pairs per column at most: 32 KiB of LDS counters
constexpr unsigned CP_BOOT = 11, CP_SIGN = 12;   // purposes of the two draws (utils/compare.py COMPARE_BOOT, COMPARE_SIGN)

static_assert(CP_T == SEL_T, "the scan and the select of select.h run on workgroups of 256 threads");

__global__ __launch_bounds__(CP_T) void boot_kernel(const double* __restrict__ s, long long ld, const int* __restrict__ lens,
                                                    const uint32_t* __restrict__ keys, int R, uint32_t draw0, double* __restrict__ out) {
  __shared__ unsigned cnt[CP_MAXN];
  __shared__ double lds[CP_T / 64][1];
  __shared__ unsigned ws[CP_T / 64];
  __shared__ int found[2];
  const int r = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int n = lens[c];
  const double* sc = s + (long long)c * ld;
  for (int k = tid; k < n; k += CP_T) cnt[k] = 0u;
  __syncthreads();
  const uint32_t k0 = keys[2 * c], k1 = keys[2 * c + 1];
  const int blocks = (n + 3) >> 2;
  for (int i = tid; i < blocks; i += CP_T) {
    const Words q = philox4x32_10((uint32_t)i, draw0 + (uint32_t)r, CP_BOOT, 0u, k0, k1);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * i + e < n) atomicAdd(&cnt[(unsigned)(((unsigned long long)q.w[e] * (unsigned long long)n) >> 32)], 1u);
  }
  __syncthreads();
  // the mean
  double v[1] = {0.0};
  for (int k = tid; k < n; k += CP_T) v[0] += (double)cnt[k] * sc[k];
  block_sum<1>(v, lds, tid);
  // the median: sorted positions pa <= pb of the drawn ranks
  const int CH = ((n + CP_T - 1) / CP_T) | 1;
  const int lo = tid * CH, hi = min(lo + CH, n);
  unsigned mine = 0;
  for (int k = lo; k < hi; ++k) mine += cnt[k];
  const unsigned before = block_excl_scan(mine, ws, tid, nullptr);
  const unsigned pa = (unsigned)(n - 1) >> 1, pb = (unsigned)n >> 1;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const unsigned p = e ? pb : pa;
    if (p >= before && p < before + mine) {   // exactly one thread: the chunks partition the n drawn positions
      unsigned run = before;
      int k = lo;
      for (; k < hi; ++k) {
        run += cnt[k];
        if (run > p) break;
      }
      found[e] = k;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const long long o = ((long long)c * 2) * R + r;
    out[o] = v[0] / (double)n;
    out[o + R] = found[0] == found[1] ? sc[found[0]] : (sc[found[0]] + sc[found[1]]) * 0.5;
  }
}

__global__ __launch_bounds__(CP_T) void select_kernel(const double* __restrict__ x, long long ldx, int R, const int* __restrict__ ranks, int K,
                                                      double* __restrict__ out) {
  __shared__ unsigned hist[256];
  __shared__ unsigned ws[CP_T / 64];
  __shared__ unsigned pick[2];
  const int q = blockIdx.x, m = blockIdx.y, tid = threadIdx.x;
  const double v = radix_select<false>(x + (long long)m * ldx, R, (unsigned)ranks[q], hist, ws, pick, tid);
  if (tid == 0) out[(long long)m * K + q] = v;
}

// MODE 0: the signs of a random pattern, 1: of an exhaustive one, 2: all +
template <int MODE>
__device__ __forceinline__ double flip_sum(const double* __restrict__ d, int n, uint32_t k0, uint32_t k1, uint32_t draw, uint32_t r) {
  double T = 0.0;
  for (int j0 = 0; j0 < n; j0 += 128) {
    Words q = {{0u, 0u, 0u, 0u}};
    if (MODE == 0) q = philox4x32_10((uint32_t)(j0 >> 7), draw, CP_SIGN, 0u, k0, k1);
    if (MODE == 1) q.w[0] = r;                // n <= 30: the first word of the first block only
#pragma unroll
    for (int w = 0; w < 4; ++w) {             // j ascending: word after word, bit after bit
      const uint32_t bits = q.w[w];
      const int base = j0 + 32 * w, end = min(n - base, 32);
      for (int b = 0; b < end; ++b) {
        const double x = d[base + b];
        T += ((bits >> b) & 1u) ? -x : x;
      }
    }
  }
  return T;
}

__global__ __launch_bounds__(CP_T) void signflip_kernel(const double* __restrict__ d, long long ld, const int* __restrict__ lens,
                                                        const int* __restrict__ modes, const uint32_t* __restrict__ keys, int P, uint32_t draw0,
                                                        double* __restrict__ T, double* __restrict__ tobs) {
  const int c = blockIdx.y;
  const long long r = (long long)blockIdx.x * CP_T + threadIdx.x;
  const int n = lens[c], exhaustive = modes[c];
  const long long m = exhaustive ? (1ll << n) : (long long)P;      // an exhaustive column has 2^n <= P (the host check)
  if (r >= m) return;
  const double* dc = d + (long long)c * ld;
  const uint32_t k0 = keys[2 * c], k1 = keys[2 * c + 1];
  T[(long long)c * P + r] = exhaustive ? flip_sum<1>(dc, n, k0, k1, 0u, (uint32_t)r) : flip_sum<0>(dc, n, k0, k1, draw0 + (uint32_t)r, 0u);
  if (r == 0) tobs[c] = flip_sum<2>(dc, n, k0, k1, 0u, 0u);
}

__global__ __launch_bounds__(CP_T) void count_kernel(const double* __restrict__ T, long long ldt, const int* __restrict__ counts,
                                                     const double* __restrict__ thr, long long* __restrict__ out) {
  __shared__ unsigned long long ws[CP_T / 64];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int m = counts[c];
  const double t = thr[c];
  const double* row = T + (long long)c * ldt;
  unsigned long long v = 0;
  for (int r = tid; r < m; r += CP_T) v += fabs(row[r]) >= t ? 1ull : 0ull;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((tid & 63) == 0) ws[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    unsigned long long all = 0;
    for (int w = 0; w < CP_T / 64; ++w) all += ws[w];
    out[c] = (long long)all;
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

int launched(const char* who) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string(who) + ": kernel launch: " + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

// what the two resampling entries share: the columns, their lengths (returned in ``n``) and the draws
int check_columns(const char* who, const void* d, const int* lens, const unsigned* keys, int C, long long ld, long long draws, unsigned draw0,
                  std::vector<int>& n, void* stream) {
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (!d || !lens || !keys) return bad("null pointer");
  if (C < 1 || C > 65535) return bad("C must be in 1..65535");
  if ((long long)draw0 + draws > (1ll << 32)) return bad("draw0 plus the draws passes 2^32 (draw indices are 32-bit)");
  const int rc = fetch(lens, C, n, stream, who);
  if (rc != BUDDY_OK) return rc;
  for (int v : n) {
    if (v < 1 || v > CP_MAXN) return bad("a length is outside 1..buddy_compare_max_pairs()");
    if (ld < v) return bad("ld is below a length");
  }
  return BUDDY_OK;
}

}  // namespace

extern "C" {

int buddy_compare_max_pairs(void) { return CP_MAXN; }

int buddy_compare_bootstrap(const double* s, const int* lens, const unsigned* keys, int C, long long ld, int R, unsigned draw0, double* out, void* stream) {
  const char* who = "buddy_compare_bootstrap";
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (!out) return bad("null pointer");
  if (R < 1 || R > (1 << 24)) return bad("R must be in 1..2^24");
  std::vector<int> n;
  const int rc = check_columns(who, s, lens, keys, C, ld, R, draw0, n, stream);
  if (rc != BUDDY_OK) return rc;
  hipLaunchKernelGGL(boot_kernel, dim3((unsigned)R, (unsigned)C), dim3(CP_T), 0, (hipStream_t)stream, s, ld, lens, keys, R, draw0, out);
  return launched(who);
}

int buddy_compare_select(const double* x, int M, int R, long long ldx, const int* ranks, int K, double* out, void* stream) {
  const char* who = "buddy_compare_select";
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (!x || !ranks || !out) return bad("null pointer");
  if (M < 1 || M > 65535) return bad("M must be in 1..65535");
  if (R < 1) return bad("R must be at least 1");
  if (ldx < R) return bad("ldx is below R");
  if (K < 1 || K > 65535) return bad("K must be in 1..65535");
  std::vector<int> rk;
  const int rc = fetch(ranks, K, rk, stream, who);
  if (rc != BUDDY_OK) return rc;
  for (int v : rk)
    if (v < 0 || v >= R) return bad("a rank is outside 0..R-1");
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)K, (unsigned)M), dim3(CP_T), 0, (hipStream_t)stream, x, ldx, R, ranks, K, out);
  return launched(who);
}

int buddy_compare_signflip(const double* d, const int* lens, const int* modes, const unsigned* keys, int C, long long ld, int P, unsigned draw0, double* T,
                           double* tobs, void* stream) {
  const char* who = "buddy_compare_signflip";
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (!modes || !T || !tobs) return bad("null pointer");
  if (P < 1 || P > (1 << 30)) return bad("P must be in 1..2^30");
  std::vector<int> n, md;
  int rc = check_columns(who, d, lens, keys, C, ld, P, draw0, n, stream);
  if (rc == BUDDY_OK) rc = fetch(modes, C, md, stream, who);
  if (rc != BUDDY_OK) return rc;
  for (int c = 0; c < C; ++c) {
    if (md[c] != 0 && md[c] != 1) return bad("a mode is neither 0 (random) nor 1 (exhaustive)");
    if (md[c] == 1 && (n[c] > 30 || (1ll << n[c]) > (long long)P)) return bad("an exhaustive column has 2^n above P");
  }
  hipLaunchKernelGGL(signflip_kernel, dim3((unsigned)((P + CP_T - 1) / CP_T), (unsigned)C), dim3(CP_T), 0, (hipStream_t)stream, d, ld, lens, modes, keys, P,
                     draw0, T, tobs);
  return launched(who);
}

int buddy_compare_count_ge(const double* T, const int* counts, const double* thr, int C, long long ldt, long long* out, void* stream) {
  const char* who = "buddy_compare_count_ge";
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (!T || !counts || !thr || !out) return bad("null pointer");
  if (C < 1 || C > 65535) return bad("C must be in 1..65535");
  std::vector<int> m;
  const int rc = fetch(counts, C, m, stream, who);
  if (rc != BUDDY_OK) return rc;
  for (int v : m)
    if (v < 1 || v > ldt) return bad("a count is outside 1..ldt");
  hipLaunchKernelGGL(count_kernel, dim3((unsigned)C), dim3(CP_T), 0, (hipStream_t)stream, T, ldt, counts, thr, out);
  return launched(who);
}

}  // extern "C"
