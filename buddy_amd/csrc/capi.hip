// extern "C" boundary (include/buddy_hip.h) over the C++ graph and kernels.
#include "../../include/buddy_hip.h"
#include "common.h"
#include "net.h"
#include "reduce.h"                           // frames_of

#include <cmath>
#include <cstring>
#include <vector>

using namespace buddy;

static int finish() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string("kernel launch: ") + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

static NetCfg mk_cfg(int nf, const int* ch_mult, int nlev, int nrb, int n_fft, int hop, int attn_mask = 0) {
  NetCfg c; std::memset(&c, 0, sizeof(c));
  c.nf = nf; c.nlev = nlev; c.nrb = nrb; c.n_fft = n_fft; c.hop = hop; c.attn_mask = attn_mask;
  for (int i = 0; i < nlev && i < 8; ++i) c.ch_mult[i] = ch_mult[i];
  return c;
}

extern "C" {

const char* buddy_last_error(void) { return last_error(); }
int buddy_version(void) { return 1; }

int buddy_ncsnpp_param_count(int nf, const int* ch_mult, int n_levels, int num_res_blocks, long long* count) {
  if (!ch_mult || !count || n_levels < 1 || n_levels > 8) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  *count = param_count(mk_cfg(nf, ch_mult, n_levels, num_res_blocks, 510, 128));
  return BUDDY_OK;
}

int buddy_ncsnpp_param_count_attn(int nf, const int* ch_mult, int n_levels, int num_res_blocks, int attn_mask, long long* count) {
  if (!ch_mult || !count || n_levels < 1 || n_levels > 8 || attn_mask < 0 || (attn_mask >> n_levels) != 0) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  *count = param_count(mk_cfg(nf, ch_mult, n_levels, num_res_blocks, 510, 128, attn_mask));
  return BUDDY_OK;
}

int buddy_ncsnpp_create_attn(const float* host_params, long long n_params, int nf, const int* ch_mult, int n_levels, int num_res_blocks,
                             int n_fft, int hop, int attn_mask, void** handle) {
  if (!host_params || !ch_mult || !handle || n_levels < 1 || n_levels > 8 || nf % 32 != 0) { set_error("bad arguments (nf must be a multiple of 32)"); return BUDDY_ERR_ARG; }
  if (attn_mask < 0 || (attn_mask >> n_levels) != 0) { set_error("attention mask selects a level the network does not have"); return BUDDY_ERR_ARG; }
  Net* N = nullptr;
  int rc = net_create(host_params, n_params, mk_cfg(nf, ch_mult, n_levels, num_res_blocks, n_fft, hop, attn_mask), &N);
  if (rc) return rc;
  *handle = N;
  return BUDDY_OK;
}

int buddy_ncsnpp_create(const float* host_params, long long n_params, int nf, const int* ch_mult, int n_levels, int num_res_blocks,
                        int n_fft, int hop, void** handle) {
  return buddy_ncsnpp_create_attn(host_params, n_params, nf, ch_mult, n_levels, num_res_blocks, n_fft, hop, 0, handle);
}

int buddy_ncsnpp_destroy(void* handle) { net_destroy((Net*)handle); return BUDDY_OK; }

int buddy_ncsnpp_replica(void* handle, void** replica) {
  if (!handle || !replica) { set_error("null argument"); return BUDDY_ERR_ARG; }
  Net* N = nullptr;
  int rc = net_replica((Net*)handle, &N);
  if (rc) return rc;
  *replica = N;
  return BUDDY_OK;
}

int buddy_ncsnpp_weight_bytes(void* handle, long long* params, long long* packed, long long* lazy, int* lazy_forms) {
  if (!handle) { set_error("null handle"); return BUDDY_ERR_ARG; }
  return net_weight_bytes((Net*)handle, params, packed, lazy, lazy_forms);
}

int buddy_conv3_weight_prep(const float* w_oihw, int O, int I, int dgrad, int kind, float* out, void* stream) {
  if (!w_oihw || !out || O < 1 || I < 1 || conv3_weight_floats(O, I, kind) == 0) { set_error("bad arguments (kind must be 0, 2, 4, 6 or 61)"); return BUDDY_ERR_ARG; }
  if (launch_conv3_weight_prep(w_oihw, O, I, dgrad != 0, kind, out, (hipStream_t)stream)) { set_error("F(2x2,3x3) form needs an input-channel count that is a multiple of 8"); return BUDDY_ERR_ARG; }
  return finish();
}

int buddy_ncsnpp_reserve(void* handle, int B, int L, int with_vjp, long long* bytes) {
  if (!handle) { set_error("null handle"); return BUDDY_ERR_ARG; }
  return net_reserve((Net*)handle, B, L, with_vjp, bytes);
}

int buddy_ncsnpp_forward(void* handle, const float* x, const float* cnoise, const float* cin, const float* cskip, const float* cout, float* y,
                         int B, int L, int save_for_vjp, void* stream) {
  if (!handle || !x || !cnoise || !y) { set_error("null argument"); return BUDDY_ERR_ARG; }
  if ((cin == nullptr) != (cskip == nullptr) || (cin == nullptr) != (cout == nullptr)) { set_error("cin/cskip/cout must be given together"); return BUDDY_ERR_ARG; }
  return net_forward((Net*)handle, x, cnoise, cin, cskip, cout, y, B, L, save_for_vjp, (hipStream_t)stream);
}

int buddy_ncsnpp_vjp(void* handle, const float* cot, float* grad_x, void* stream) {
  if (!handle || !cot || !grad_x) { set_error("null argument"); return BUDDY_ERR_ARG; }
  return net_vjp((Net*)handle, cot, grad_x, (hipStream_t)stream);
}

int buddy_ncsnpp_vjp_params(void* handle, const float* cot, float* grad_x, float* grad_params, int accumulate, void* stream) {
  if (!handle || !cot || !grad_params) { set_error("null argument"); return BUDDY_ERR_ARG; }
  return net_vjp_params((Net*)handle, cot, grad_x, grad_params, accumulate, (hipStream_t)stream);
}

int buddy_ncsnpp_update_params(void* handle, const float* dev_params, void* stream) {
  if (!handle || !dev_params) { set_error("null argument"); return BUDDY_ERR_ARG; }
  return net_update_params((Net*)handle, dev_params, (hipStream_t)stream);
}

int buddy_ncsnpp_tap(void* handle, int module_idx, const float** ptr, int dims[4]) {
  if (!handle || !ptr || !dims) { set_error("null argument"); return BUDDY_ERR_ARG; }
  return net_get_tap((Net*)handle, module_idx, ptr, dims);
}

int buddy_copy_d2d(void* dst, const void* src, long long bytes, void* stream) {
  if (!dst || !src || bytes < 0) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  hipError_t e = hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e != hipSuccess) { set_error(std::string("hipMemcpyAsync: ") + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

int buddy_hbm_ubench(const void* src, void* dst, long long bytes, int mode, int nt, int blocks, void* stream) {
  if ((mode == 3 || mode == 4) && (!src || !dst)) { set_error("hbm_ubench: null buffer"); return BUDDY_ERR_ARG; }
  if ((mode != 2 && !src) || !dst || bytes < 16 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) { set_error("hbm_ubench: 16-byte aligned device buffers of >= 16 bytes"); return BUDDY_ERR_ARG; }
  if (launch_hbm_ubench(src, dst, bytes, mode, nt, blocks, (hipStream_t)stream)) { set_error("hbm_ubench: mode 0 copy | 1 read | 2 write; blocks >= 1 (grid-stride) or -1 | -2 | -4 | -8 (one chunk of that many 16-byte words per thread and workgroup)"); return BUDDY_ERR_ARG; }
  return BUDDY_OK;
}
int buddy_mfma_ubench(const float* seed, float* out, int blocks, int iters, unsigned long long* clk, void* stream) {
  if (!seed || !out || !clk) { set_error("null argument"); return BUDDY_ERR_ARG; }
  launch_mfma_ubench(seed, out, blocks, iters, clk, (hipStream_t)stream);
  return finish();
}

int buddy_mfma_ubench_bf16(const float* seed, float* out, int blocks, int iters, unsigned long long* clk, void* stream) {
  if (!seed || !out || !clk) { set_error("null argument"); return BUDDY_ERR_ARG; }
  launch_mfma_ubench_bf16(seed, out, blocks, iters, clk, (hipStream_t)stream);
  return finish();
}

int buddy_prof_enable(int on) { igemm_prof_enable(on); return BUDDY_OK; }
int buddy_prof_collect(double* ms, double* flops, long long* launches, double* bytes, double* exec_flops) {
  if (!ms || !flops || !launches || !bytes || !exec_flops) { set_error("null argument"); return BUDDY_ERR_ARG; }
  if (igemm_prof_collect(ms, flops, launches, bytes, exec_flops)) { set_error("event timing failed"); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

int buddy_prof_collect_hbm(double* ms, double* bytes, long long* launches) {
  if (!ms || !bytes || !launches) { set_error("null argument"); return BUDDY_ERR_ARG; }
  if (prof_hbm_collect(ms, bytes, launches)) { set_error("event timing failed"); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

int buddy_prof_collect_wino4(double* ms, double* gemm_flops, double* bytes_in, double* bytes_out, double* bytes_gemm, long long* launches) {
  if (!ms || !gemm_flops || !bytes_in || !bytes_out || !bytes_gemm || !launches) { set_error("null argument"); return BUDDY_ERR_ARG; }
  if (prof_w4_collect(ms, gemm_flops, bytes_in, bytes_out, bytes_gemm, launches)) { set_error("event timing failed"); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

static int gemm_impl(const float* A, int ldA, int transA, const float* Bt, int ldB, int transB, float* C, int ldC, int M, int N, int K, float alpha,
                     const float* bias_n, int accumulate, int batch, long long strideA, long long strideB, long long strideC, int tag, void* stream) {
  if (!A || !Bt || !C || K % 4 || (transA && M % 4) || (transB && N % 4)) { set_error("bad gemm arguments (K, and M/N of k-major operands, must be multiples of 4)"); return BUDDY_ERR_ARG; }
  IgemmParams p; std::memset(&p, 0, sizeof(p));
  p.A0 = A; p.ldA0 = ldA; p.Cin = K; p.M = M; p.N = N; p.Bt = Bt; p.ldB = ldB; p.C = C; p.ldC = ldC; p.sA = strideA; p.sB = strideB; p.sC = strideC;
  p.alpha = alpha; p.out_scale = 1.f; p.bias_n = bias_n; p.accumulate = accumulate; p.H = 1; p.W = 1; p.rows_per_batch = 1;
  p.tag = tag;
  launch_igemm(p, 1, transA != 0, transB != 0, batch, (hipStream_t)stream);
  return finish();
}

int buddy_gemm(const float* A, int ldA, int transA, const float* Bt, int ldB, int transB, float* C, int ldC, int M, int N, int K, float alpha,
               const float* bias_n, int accumulate, int batch, long long strideA, long long strideB, long long strideC, void* stream) {
  return gemm_impl(A, ldA, transA, Bt, ldB, transB, C, ldC, M, N, K, alpha, bias_n, accumulate, batch, strideA, strideB, strideC, 0, stream);
}

int buddy_gemm_winograd_domain(const float* V, const float* U, float* Mo, int tiles, int Cout, int Cin, int positions, void* stream) {
  if (positions < 1) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  return gemm_impl(V, Cin, 0, U, Cin, 0, Mo, Cout, tiles, Cout, Cin, 1.f, nullptr, 0, positions, (long long)tiles * Cin, (long long)Cout * Cin,
                   (long long)tiles * Cout, 36, stream);
}

long long buddy_wgemm_packed_bytes(int positions, int Cout, int Cin) {
  return (positions < 1 || !wgemm_supported(Cout, Cin)) ? 0 : (long long)wgemm_packed_bytes(positions, Cout, Cin);
}

int buddy_wgemm_pack_weights(const float* U, void* U3, int positions, int Cout, int Cin, void* stream) {
  if (!U || !U3 || positions < 1 || !wgemm_supported(Cout, Cin)) { set_error("bad arguments (Cout % 128, Cin % 32)"); return BUDDY_ERR_ARG; }
  wgemm_pack_weights(U, U3, positions, Cout, Cin, (hipStream_t)stream);
  return finish();
}

int buddy_gemm_winograd_domain_bf16x3(const float* V, const void* U3, float* Mo, int tiles, int Cout, int Cin, int positions, void* stream) {
  if (!V || !U3 || !Mo || tiles < 1 || positions < 1 || !wgemm_supported(Cout, Cin)) { set_error("bad arguments (Cout % 128, Cin % 32)"); return BUDDY_ERR_ARG; }
  launch_wgemm_bf16x3(V, U3, Mo, tiles, Cout, Cin, positions, (hipStream_t)stream);
  return finish();
}

long long buddy_wgemm_f16x2_packed_bytes(int positions, int Cout, int Cin) {
  return (positions < 1 || positions > 64 || !wgemm_f16x2_supported(Cout, Cin)) ? 0 : (long long)wgemm_f16x2_packed_bytes(positions, Cout, Cin);
}
int buddy_wgemm_f16x2_pack_weights(const float* U, void* U2, int positions, int Cout, int Cin, void* stream) {
  if (!U || !U2 || positions < 1 || positions > 64 || !wgemm_f16x2_supported(Cout, Cin)) { set_error("bad arguments (positions <= 64, Cout % 128, Cin % 64)"); return BUDDY_ERR_ARG; }
  wgemm_f16x2_pack_weights(U, U2, positions, Cout, Cin, (hipStream_t)stream);
  return finish();
}
int buddy_gemm_winograd_domain_f16x2(const float* V, const void* U2, float* Mo, int tiles, int Cout, int Cin, int positions, const unsigned* vmax,
                                     int tiles_per_utt, void* stream) {
  if (!V || !U2 || !Mo || !vmax || tiles < 1 || tiles_per_utt < 32 || tiles % tiles_per_utt || positions < 1 || positions > 64 || !wgemm_f16x2_supported(Cout, Cin)) {
    set_error("bad arguments (positions <= 64, Cout % 128, Cin % 64, tiles a multiple of tiles_per_utt >= 32)"); return BUDDY_ERR_ARG;
  }
  launch_wgemm_f16x2(V, U2, Mo, tiles, Cout, Cin, positions, vmax, tiles_per_utt, (hipStream_t)stream);
  return finish();
}
long long buddy_wgemm_f16_packed_bytes(int positions, int Cout, int Cin) {
  return (positions < 1 || positions > 64 || !wgemm_f16_supported(Cout, Cin)) ? 0 : (long long)wgemm_f16_packed_bytes(positions, Cout, Cin);
}
int buddy_wgemm_f16_pack_weights(const float* U, void* U1, int positions, int Cout, int Cin, void* stream) {
  if (!U || !U1 || positions < 1 || positions > 64 || !wgemm_f16_supported(Cout, Cin)) { set_error("bad arguments (positions <= 64, Cout % 128, Cin % 32)"); return BUDDY_ERR_ARG; }
  wgemm_f16_pack_weights(U, U1, positions, Cout, Cin, (hipStream_t)stream);
  return finish();
}
int buddy_gemm_winograd_domain_f16(const void* V16, const signed char* vexp, const void* U1, float* Mo, int tiles, int Cout, int Cin, int positions, void* stream) {
  if (!V16 || !vexp || !U1 || !Mo || tiles < 1 || positions < 1 || positions > 64 || !wgemm_f16_supported(Cout, Cin)) {
    set_error("bad arguments (positions <= 64, Cout % 128, Cin % 32)"); return BUDDY_ERR_ARG;
  }
  launch_wgemm_f16(V16, vexp, U1, Mo, tiles, Cout, Cin, positions, (hipStream_t)stream);
  return finish();
}
int buddy_abs_max_bits(const float* x, int groups, int segments, long long seg_len, unsigned* out, void* stream) {
  if (!x || !out || groups < 1 || segments < 1 || seg_len < 1) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  launch_abs_max_bits(x, groups, segments, seg_len, out, (hipStream_t)stream);
  return finish();
}

int buddy_gemm_bf16x3(const float* A0, int ldA0, const float* A1, int ldA1, int C0, const void* W3, float* Cm, int ldC, long long M, int N, int K,
                      const float* bias_n, float alpha, int accumulate, void* stream) {
  if (!A0 || !W3 || !Cm || M < 1 || !wgemm_general_supported(N, K, A1 ? C0 : 0, ldA0, A1 ? ldA1 : 0, ldC, A0, A1, Cm, bias_n)) {
    set_error("bad arguments (N % 128, K % 32, C0 % 32, 16-byte aligned rows)"); return BUDDY_ERR_ARG;
  }
  launch_wgemm_bf16x3_general(A0, ldA0, A1, ldA1, C0, W3, Cm, ldC, M, N, K, bias_n, alpha, accumulate, (hipStream_t)stream);
  return finish();
}

// the same general form in f16x2 arithmetic (W2 = buddy_wgemm_f16x2_pack_weights(W, ., 1, N, K)); gn_bwd != 0 arguments as buddy_gemm_bf16x3_gn_bwd
int buddy_gemm_f16x2(const float* A0, int ldA0, const float* A1, int ldA1, int C0, const void* W2, float* Cm, int ldC, long long M, int N, int K,
                     const float* bias_n, float alpha, int accumulate, void* stream) {
  if (!A0 || !W2 || !Cm || M < 1 || !wgemm_f16x2_general_supported(N, K, A1 ? C0 : 0, ldA0, A1 ? ldA1 : 0, ldC, A0, A1, Cm, bias_n)) {
    set_error("bad arguments (N % 128, K % 64, C0 % 32, 16-byte aligned rows)"); return BUDDY_ERR_ARG;
  }
  launch_wgemm_f16x2_general(A0, ldA0, A1, ldA1, C0, W2, Cm, ldC, M, N, K, bias_n, alpha, accumulate, (hipStream_t)stream);
  return finish();
}
// the two *_gn_bwd entries: argument check, views, the GroupNorm backward's sums, then the arithmetic's launcher (arith_ok: its own shape condition)
static int gemm_gn_bwd(decltype(&launch_wgemm_bf16x3_gnbwd) launch, bool arith_ok, const char* shape_msg, const float* A, int ldA, const void* Wp, const float* x0,
                       const float* x1, int C0, const float* da, const float* stats, const float* gamma, const float* beta, int G, int silu, float alpha, float* dx0,
                       float* dx1, int acc0, int acc1, double* stat_scratch, float* red, int B, int HW, int N, int K, void* stream) {
  if (!A || !Wp || !x0 || !da || !stats || !gamma || !beta || !dx0 || !stat_scratch || !red || B < 1 || HW < 1 || G < 1 || N % 4 || (N / G) % 4 || N > 1024 ||
      (x1 && (C0 % 4 || C0 < 4 || C0 >= N)) || (x1 != nullptr) != (dx1 != nullptr)) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  Src2 x; x.p0 = x0; x.p1 = x1; x.C0 = x1 ? C0 : N; x.ld0 = x1 ? C0 : N; x.ld1 = x1 ? N - C0 : 0;
  Dst2 d; d.p0 = dx0; d.p1 = dx1; d.C0 = x.C0; d.ld0 = x.ld0; d.ld1 = x.ld1; d.acc0 = acc0; d.acc1 = acc1;
  if (!wgemm_gnbwd_supported(N, K, ldA, x, d, A, da) || !arith_ok) { set_error(shape_msg); return BUDDY_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  launch_gn_bwd_sums(x, stats, gamma, beta, da, B, 1, HW, N, G, 0, silu, stat_scratch, red, st);
  launch(A, ldA, Wp, (long long)B * HW, N, K, alpha, x, da, stats, red, gamma, beta, G, silu, HW, d, st);
  return finish();
}
int buddy_gemm_f16x2_gn_bwd(const float* A, int ldA, const void* W2, const float* x0, const float* x1, int C0, const float* da, const float* stats,
                            const float* gamma, const float* beta, int G, int silu, float alpha, float* dx0, float* dx1, int acc0, int acc1,
                            double* stat_scratch, float* red, int B, int HW, int N, int K, void* stream) {
  return gemm_gn_bwd(launch_wgemm_f16x2_gnbwd, wgemm_f16x2_supported(N, K), "bad arguments (N % 128, K % 64, C0 % 128, 16-byte aligned rows)", A, ldA, W2, x0, x1, C0, da,
                     stats, gamma, beta, G, silu, alpha, dx0, dx1, acc0, acc1, stat_scratch, red, B, HW, N, K, stream);
}
int buddy_gemm_bf16x3_gn_bwd(const float* A, int ldA, const void* W3, const float* x0, const float* x1, int C0, const float* da, const float* stats,
                             const float* gamma, const float* beta, int G, int silu, float alpha, float* dx0, float* dx1, int acc0, int acc1,
                             double* stat_scratch, float* red, int B, int HW, int N, int K, void* stream) {
  return gemm_gn_bwd(launch_wgemm_bf16x3_gnbwd, true, "bad arguments (N % 128, K % 32, C0 % 128, 16-byte aligned rows)", A, ldA, W3, x0, x1, C0, da,
                     stats, gamma, beta, G, silu, alpha, dx0, dx1, acc0, acc1, stat_scratch, red, B, HW, N, K, stream);
}

int buddy_conv3x3(const float* x, const float* wt, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, void* stream) {
  if (!x || !wt || !y || Cin % 4) { set_error("bad conv arguments"); return BUDDY_ERR_ARG; }
  IgemmParams p; std::memset(&p, 0, sizeof(p));
  p.A0 = x; p.ldA0 = Cin; p.Cin = Cin; p.H = H; p.W = W; p.M = B * H * W; p.N = Cout; p.Bt = wt; p.ldB = 9 * Cin; p.C = y; p.ldC = Cout;
  p.bias_n = bias; p.alpha = 1.f; p.out_scale = 1.f; p.rows_per_batch = H * W;
  launch_igemm(p, 9, false, false, 1, (hipStream_t)stream);
  return finish();
}

int buddy_winograd_transform_weights(const float* wt_host, int Cout, int Cin, float* U_host) {
  if (!wt_host || !U_host || Cin % 16) { set_error("bad arguments (Cin must be a multiple of 16)"); return BUDDY_ERR_ARG; }
  wino_transform_weights(wt_host, Cout, Cin, U_host);
  return BUDDY_OK;
}

int buddy_conv3x3_winograd(const float* x, const float* U, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, void* stream) {
  if (!x || !U || !y) { set_error("null argument"); return BUDDY_ERR_ARG; }
  IgemmParams p; std::memset(&p, 0, sizeof(p));
  p.A0 = x; p.ldA0 = Cin; p.Cin = Cin; p.H = H; p.W = W; p.M = B * H * W; p.N = Cout; p.C = y; p.ldC = Cout;
  p.bias_n = bias; p.alpha = 1.f; p.out_scale = 1.f; p.rows_per_batch = H * W;
  if (!wino_supported(p)) { set_error("shape not supported by the Winograd kernel (H, W even; Cin % 16; Cout % 32)"); return BUDDY_ERR_ARG; }
  igemm_prof_record(p, 9, 1, (hipStream_t)stream, true);
  launch_wino(p, U, (hipStream_t)stream);
  igemm_prof_record(p, 9, 1, (hipStream_t)stream, false);
  return finish();
}

int buddy_winograd4_transform_weights(const float* wt_host, int Cout, int Cin, float* U4_host) {
  if (!wt_host || !U4_host || Cout < 1 || Cin < 1) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  wino4_transform_weights(wt_host, Cout, Cin, U4_host);
  return BUDDY_OK;
}
int buddy_conv3x3_winograd4(const float* x, const float* U4, const float* bias, float* y, float* scratch, int B, int H, int W, int Cin, int Cout,
                            void* stream) {
  if (!x || !U4 || !y || !scratch) { set_error("null argument"); return BUDDY_ERR_ARG; }
  IgemmParams p; std::memset(&p, 0, sizeof(p));
  p.A0 = x; p.ldA0 = Cin; p.Cin = Cin; p.H = H; p.W = W; p.M = B * H * W; p.N = Cout; p.C = y; p.ldC = Cout;
  p.bias_n = bias; p.alpha = 1.f; p.out_scale = 1.f; p.rows_per_batch = H * W;
  if (!wino4_supported(p)) { set_error("shape not supported by the F(4x4,3x3) path (H, W, Cin, Cout multiples of 4)"); return BUDDY_ERR_ARG; }
  long long vf = 0, mf = 0; wino4_scratch(p, &vf, &mf);
  igemm_prof_record(p, 9, 1, (hipStream_t)stream, true, 0.25);
  launch_wino4(p, U4, scratch, scratch + vf, (hipStream_t)stream);
  igemm_prof_record(p, 9, 1, (hipStream_t)stream, false, 0.25);
  return finish();
}

int buddy_winograd6_transform_weights(const float* wt_host, int Cout, int Cin, float* U6_host) {
  if (!wt_host || !U6_host || Cout < 1 || Cin < 1) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  wino6_transform_weights(wt_host, Cout, Cin, U6_host);
  return BUDDY_OK;
}
int buddy_conv3x3_winograd6(const float* x, const float* U6, const float* bias, float* y, float* scratch, int B, int H, int W, int Cin, int Cout,
                            void* stream) {
  if (!x || !U6 || !y || !scratch) { set_error("null argument"); return BUDDY_ERR_ARG; }
  IgemmParams p; std::memset(&p, 0, sizeof(p));
  p.A0 = x; p.ldA0 = Cin; p.Cin = Cin; p.H = H; p.W = W; p.M = B * H * W; p.N = Cout; p.C = y; p.ldC = Cout;
  p.bias_n = bias; p.alpha = 1.f; p.out_scale = 1.f; p.rows_per_batch = H * W;
  if (!wino6_supported(p)) { set_error("shape not supported by the F(6x6,3x3) path (H, W >= 6; Cin, Cout multiples of 4)"); return BUDDY_ERR_ARG; }
  long long vf = 0, mf = 0; wino6_scratch(p, &vf, &mf);
  const double xr = wino6_exec_ratio(p);
  igemm_prof_record(p, 9, 1, (hipStream_t)stream, true, xr);
  launch_wino6(p, U6, scratch, scratch + vf, (hipStream_t)stream);
  igemm_prof_record(p, 9, 1, (hipStream_t)stream, false, xr);
  return finish();
}

int buddy_conv3x3_winograd6_f16(const float* x, const void* U1, const float* bias, float* y, float* scratch, int B, int H, int W, int Cin, int Cout,
                                void* stream) {
  if (!x || !U1 || !y || !scratch) { set_error("null argument"); return BUDDY_ERR_ARG; }
  IgemmParams p; std::memset(&p, 0, sizeof(p));
  p.A0 = x; p.ldA0 = Cin; p.Cin = Cin; p.H = H; p.W = W; p.M = B * H * W; p.N = Cout; p.C = y; p.ldC = Cout;
  p.bias_n = bias; p.alpha = 1.f; p.out_scale = 1.f; p.rows_per_batch = H * W;
  if (!wino6_supported(p) || !wgemm_f16_supported(Cout, Cin)) { set_error("shape not supported by the f16 F(6x6,3x3) path (H, W >= 6; Cout % 128, Cin % 32)"); return BUDDY_ERR_ARG; }
  long long vf = 0, mf = 0; wino6_scratch(p, &vf, &mf);
  launch_wino6(p, nullptr, scratch, scratch + vf, (hipStream_t)stream, nullptr, nullptr, nullptr, U1, 0, 3);
  return finish();
}

// U1 != nullptr (F(6x6,3x3) only): the GEMM pass in f16 on that image (gemm = "f16"), U4 unused
static int gn_conv3x3_winograd(bool f6, const float* x0, const float* x1, int C0, const float* gamma, const float* beta, int G, int silu, const float* U4,
                               const float* bias, float* y, float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W,
                               int Cin, int Cout, void* stream, const void* U1 = nullptr) {
  if (!x0 || !gamma || !beta || !(U4 || U1) || !y || !scratch || !stats || !stat_scratch || G < 1 || Cin % 4 || (Cin / G) % 4 || Cin > 1024 ||
      (x1 && (C0 % 4 || C0 < 4 || C0 >= Cin)) || (U1 && !wgemm_f16_supported(Cout, Cin))) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  IgemmParams p; std::memset(&p, 0, sizeof(p));
  p.ldA0 = Cin; p.Cin = Cin; p.H = H; p.W = W; p.M = B * H * W; p.N = Cout; p.C = y; p.ldC = Cout;
  p.bias_n = bias; p.alpha = 1.f; p.out_scale = 1.f; p.rows_per_batch = H * W;
  if (!(f6 ? wino6_supported(p) : wino4_supported(p))) { set_error("shape not supported by this Winograd path"); return BUDDY_ERR_ARG; }
  const int sc = csum ? (f6 ? wino6_stat_chunks(p) : wino4_stat_chunks(p)) : 0;
  if (csum && (sc == 0 || (long long)sc * Cout > 256LL * 1024)) { set_error("shape not supported by the statistics epilogue"); return BUDDY_ERR_ARG; }
  W4Gn gn;
  gn.x.p0 = x0; gn.x.p1 = x1; gn.x.C0 = x1 ? C0 : Cin; gn.x.ld0 = x1 ? C0 : Cin; gn.x.ld1 = x1 ? Cin - C0 : 0;
  gn.stats = stats; gn.gamma = gamma; gn.beta = beta; gn.G = G; gn.silu = silu;
  launch_gn_stats(gn.x, B, H * W, Cin, G, 1e-6f, stat_scratch, stats, st);
  long long vf = 0, mf = 0;
  if (f6) { wino6_scratch(p, &vf, &mf); launch_wino6(p, U4, scratch, scratch + vf, st, &gn, csum ? stat_scratch : nullptr, nullptr, U1, 0, U1 ? 3 : 1); }
  else { wino4_scratch(p, &vf, &mf); launch_wino4(p, U4, scratch, scratch + vf, st, &gn, csum ? stat_scratch : nullptr); }
  if (csum) launch_csum_collapse(stat_scratch, sc, B, Cout, csum, st);
  return finish();
}
int buddy_gn_conv3x3_winograd4(const float* x0, const float* x1, int C0, const float* gamma, const float* beta, int G, int silu, const float* U4,
                               const float* bias, float* y, float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W,
                               int Cin, int Cout, void* stream) {
  return gn_conv3x3_winograd(false, x0, x1, C0, gamma, beta, G, silu, U4, bias, y, scratch, stats, stat_scratch, csum, B, H, W, Cin, Cout, stream);
}
int buddy_gn_conv3x3_winograd6(const float* x0, const float* x1, int C0, const float* gamma, const float* beta, int G, int silu, const float* U6,
                               const float* bias, float* y, float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W,
                               int Cin, int Cout, void* stream) {
  return gn_conv3x3_winograd(true, x0, x1, C0, gamma, beta, G, silu, U6, bias, y, scratch, stats, stat_scratch, csum, B, H, W, Cin, Cout, stream);
}

int buddy_gn_conv3x3_winograd6_f16(const float* x0, const float* x1, int C0, const float* gamma, const float* beta, int G, int silu, const void* U1,
                                   const float* bias, float* y, float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W,
                                   int Cin, int Cout, void* stream) {
  if (!U1) { set_error("null argument"); return BUDDY_ERR_ARG; }
  return gn_conv3x3_winograd(true, x0, x1, C0, gamma, beta, G, silu, nullptr, bias, y, scratch, stats, stat_scratch, csum, B, H, W, Cin, Cout, stream, U1);
}

int buddy_conv3x3_winograd6_gn_bwd_sums(const float* g, const float* U6, float* da, float* scratch, const float* x0, const float* x1, int C0,
                                        const float* stats, const float* gamma, const float* beta, int G, int silu, double* stat_scratch,
                                        double* chsum, int B, int H, int W, int Cin, int Cout, void* stream) {
  if (!g || !U6 || !da || !scratch || !x0 || !stats || !gamma || !beta || !stat_scratch || !chsum || G < 1 || Cout % 4 || (Cout / G) % 4 ||
      Cout > 1024 || (x1 && (C0 % 4 || C0 < 4 || C0 >= Cout))) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  IgemmParams p; std::memset(&p, 0, sizeof(p));
  p.A0 = g; p.ldA0 = Cin; p.Cin = Cin; p.H = H; p.W = W; p.M = B * H * W; p.N = Cout; p.C = da; p.ldC = Cout;
  p.alpha = 1.f; p.out_scale = 1.f; p.rows_per_batch = H * W;
  if (!wino6_supported(p)) { set_error("shape not supported by the F(6x6,3x3) path (H, W >= 6; Cin, Cout multiples of 4)"); return BUDDY_ERR_ARG; }
  const int sc = wino6_stat_chunks(p);
  if (sc == 0 || (long long)sc * Cout > 256LL * 1024) { set_error("shape not supported by the statistics epilogue"); return BUDDY_ERR_ARG; }
  W4Gn bg;
  bg.x.p0 = x0; bg.x.p1 = x1; bg.x.C0 = x1 ? C0 : Cout; bg.x.ld0 = x1 ? C0 : Cout; bg.x.ld1 = x1 ? Cout - C0 : 0;
  bg.stats = stats; bg.gamma = gamma; bg.beta = beta; bg.G = G; bg.silu = silu;
  long long vf = 0, mf = 0; wino6_scratch(p, &vf, &mf);
  launch_wino6(p, U6, scratch, scratch + vf, st, nullptr, stat_scratch, &bg);
  launch_csum_collapse(stat_scratch, sc, B, Cout, chsum, st);
  return finish();
}

// up = 0 / 2: conv3x3 / the sub-pixel up data-gradient of the GroupNorm backward of da; U1 != nullptr: the GEMM pass in f16 on that image (U6 unused)
static int gnbwd_conv3x3_winograd6(int up, const float* x, const float* gamma, const float* beta, const float* stats, const float* da, int G, int silu,
                                   const float* U6, const void* U1, float* y, float* scratch, double* stat_scratch, float* red, int B, int H, int W, int C,
                                   int Cout, void* stream) {
  if (!x || !gamma || !beta || !stats || !da || !(U6 || U1) || !y || !scratch || !stat_scratch || !red || G < 1 || C % 4 || (C / G) % 4 || C > 1024 ||
      (up && Cout % 4) || (U1 && !wgemm_f16_supported(Cout, up ? 4 * C : C))) {
    set_error("bad arguments"); return BUDDY_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  IgemmParams p; std::memset(&p, 0, sizeof(p));
  p.ldA0 = C; p.Cin = C; p.H = H; p.W = W; p.M = B * H * W; p.N = Cout; p.C = y; p.ldC = Cout;
  p.alpha = 1.f; p.out_scale = 1.f; p.rows_per_batch = H * W;
  if (!wino6_supported(p)) { set_error("shape not supported by the F(6x6,3x3) path (H, W >= 6; channels multiples of 4)"); return BUDDY_ERR_ARG; }
  W4Gn gn;
  gn.x.p0 = x; gn.x.p1 = nullptr; gn.x.C0 = C; gn.x.ld0 = C; gn.x.ld1 = 0;
  gn.stats = stats; gn.gamma = gamma; gn.beta = beta; gn.G = G; gn.silu = silu; gn.da = da; gn.ldda = C; gn.red = red;
  launch_gn_bwd_sums(gn.x, stats, gamma, beta, da, B, up ? 2 * H : H, up ? 2 * W : W, C, G, 0, silu, stat_scratch, red, st);
  long long vf = 0, mf = 0; wino6_scratch(p, &vf, &mf, up);
  launch_wino6(p, U6, scratch, scratch + vf, st, &gn, nullptr, nullptr, U1, up, U1 ? 3 : 1);
  return finish();
}
int buddy_gnbwd_conv3x3_winograd6(const float* x, const float* gamma, const float* beta, const float* stats, const float* da, int G, int silu,
                                  const float* U6, float* y, float* scratch, double* stat_scratch, float* red, int B, int H, int W, int C, int Cout,
                                  void* stream) {
  return gnbwd_conv3x3_winograd6(0, x, gamma, beta, stats, da, G, silu, U6, nullptr, y, scratch, stat_scratch, red, B, H, W, C, Cout, stream);
}
int buddy_gnbwd_conv3x3_winograd6_f16(const float* x, const float* gamma, const float* beta, const float* stats, const float* da, int G, int silu,
                                      const void* U1, float* y, float* scratch, double* stat_scratch, float* red, int B, int H, int W, int C, int Cout,
                                      void* stream) {
  if (!U1) { set_error("null argument"); return BUDDY_ERR_ARG; }
  return gnbwd_conv3x3_winograd6(0, x, gamma, beta, stats, da, G, silu, nullptr, U1, y, scratch, stat_scratch, red, B, H, W, C, Cout, stream);
}

// U1 != nullptr: the GEMM pass in f16 on that image (U6up unused)
static int gn_upconv3x3_winograd6(const float* x, const float* gamma, const float* beta, int G, int silu, const float* U6up, const void* U1, const float* bias,
                                  float* y, float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W, int Cin, int Cout, void* stream) {
  if (!x || !gamma || !beta || !(U6up || U1) || !y || !scratch || !stats || !stat_scratch || G < 1 || Cin % 4 || (Cin / G) % 4 || Cin > 1024 || Cout % 4 ||
      (U1 && !wgemm_f16_supported(4 * Cout, Cin))) {
    set_error("bad arguments"); return BUDDY_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  IgemmParams p; std::memset(&p, 0, sizeof(p));
  p.ldA0 = Cin; p.Cin = Cin; p.H = H; p.W = W; p.M = B * H * W; p.N = Cout; p.C = y; p.ldC = Cout;
  p.bias_n = bias; p.alpha = 1.f; p.out_scale = 1.f; p.rows_per_batch = H * W;
  if (!wino6_supported(p)) { set_error("shape not supported by the F(6x6,3x3) path (H, W >= 6; Cin, Cout multiples of 4)"); return BUDDY_ERR_ARG; }
  const int sc = csum ? wino6_stat_chunks(p, 1) : 0;
  if (csum && (sc == 0 || (long long)sc * Cout > 256LL * 1024)) { set_error("shape not supported by the statistics epilogue"); return BUDDY_ERR_ARG; }
  W4Gn gn;
  gn.x.p0 = x; gn.x.p1 = nullptr; gn.x.C0 = Cin; gn.x.ld0 = Cin; gn.x.ld1 = 0;
  gn.stats = stats; gn.gamma = gamma; gn.beta = beta; gn.G = G; gn.silu = silu;
  launch_gn_stats(gn.x, B, H * W, Cin, G, 1e-6f, stat_scratch, stats, st);
  long long vf = 0, mf = 0; wino6_scratch(p, &vf, &mf, 1);
  launch_wino6(p, U6up, scratch, scratch + vf, st, &gn, csum ? stat_scratch : nullptr, nullptr, U1, 1, U1 ? 3 : 1);
  if (csum) launch_csum_collapse(stat_scratch, sc, B, Cout, csum, st);
  return finish();
}

int buddy_gn_upconv3x3_winograd6(const float* x, const float* gamma, const float* beta, int G, int silu, const float* U6up, const float* bias, float* y,
                                 float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W, int Cin, int Cout, void* stream) {
  return gn_upconv3x3_winograd6(x, gamma, beta, G, silu, U6up, nullptr, bias, y, scratch, stats, stat_scratch, csum, B, H, W, Cin, Cout, stream);
}
int buddy_gn_upconv3x3_winograd6_f16(const float* x, const float* gamma, const float* beta, int G, int silu, const void* U1up, const float* bias, float* y,
                                     float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W, int Cin, int Cout, void* stream) {
  if (!U1up) { set_error("null argument"); return BUDDY_ERR_ARG; }
  return gn_upconv3x3_winograd6(x, gamma, beta, G, silu, nullptr, U1up, bias, y, scratch, stats, stat_scratch, csum, B, H, W, Cin, Cout, stream);
}

int buddy_gnbwd_upconv3x3_winograd6(const float* h, const float* gamma, const float* beta, const float* stats, const float* da, int G, int silu,
                                    const float* U6upT, float* y, float* scratch, double* stat_scratch, float* red, int B, int H, int W, int C,
                                    int Cout, void* stream) {
  return gnbwd_conv3x3_winograd6(2, h, gamma, beta, stats, da, G, silu, U6upT, nullptr, y, scratch, stat_scratch, red, B, H, W, C, Cout, stream);
}
int buddy_gnbwd_upconv3x3_winograd6_f16(const float* h, const float* gamma, const float* beta, const float* stats, const float* da, int G, int silu,
                                        const void* U1upT, float* y, float* scratch, double* stat_scratch, float* red, int B, int H, int W, int C,
                                        int Cout, void* stream) {
  if (!U1upT) { set_error("null argument"); return BUDDY_ERR_ARG; }
  return gnbwd_conv3x3_winograd6(2, h, gamma, beta, stats, da, G, silu, nullptr, U1upT, y, scratch, stat_scratch, red, B, H, W, C, Cout, stream);
}

// What the stand-alone GroupNorm kernels (ops.hip) cannot compute, for all four entries below; nullptr = fine.  G is checked before it divides;
// C <= 1024: a reduction block holds C / 4 <= 256 channel quads; mode 1 / extra_mode 2 read a tensor of H/2 x W/2 pixels at (h >> 1, w >> 1).
static const char* gn_refusal(int B, int H, int W, int C, int G, int mode, int extra_mode) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || G < 1) return "groupnorm: B, H, W, C and G must be at least 1";
  if (C % G != 0) return "groupnorm: C must be a multiple of G";
  if ((C / G) % 4 != 0) return "groupnorm: the channels of a group must be a multiple of 4 (a thread holds one channel quad of one group)";
  if (C > 1024) return "groupnorm: C must be at most 1024";
  if (mode < 0 || mode > 2) return "groupnorm: mode must be 0 (same), 1 (2x down) or 2 (2x up)";
  if (extra_mode < 0 || extra_mode > 2) return "groupnorm: extra_mode must be 0 (none), 1 (same resolution) or 2 (H/2 x W/2)";
  if ((mode == 1 || extra_mode == 2) && ((H | W) & 1)) return "groupnorm: mode 1 and extra_mode 2 (tensors at H/2 x W/2) need even H and W";
  return nullptr;
}
// a two-pointer channel view: the first part's width w0 (w1 = C - w0 for the second, where there is one) and the row strides
static const char* gn_view_refusal(const void* p1, int w0, int w1, int ld0, int ld1, int C) {
  if (p1 == nullptr && w0 != C) return "groupnorm: a single-pointer view has all C channels in its first part";
  if (p1 != nullptr && (w0 < 4 || w1 < 4 || w0 + w1 != C)) return "groupnorm: both parts of a two-pointer view hold at least 4 channels, C in all";
  if (w0 % 4 != 0) return "groupnorm: the first part of a view must be a multiple of 4 channels wide (a thread's channel quad lies in one part)";
  if (ld0 < w0 || ld0 % 4 != 0) return "groupnorm: a row stride must be a multiple of 4 floats, at least the part's width";
  if (p1 != nullptr && (ld1 < w1 || ld1 % 4 != 0)) return "groupnorm: a row stride must be a multiple of 4 floats, at least the part's width";
  return nullptr;
}
#define GN_REFUSE(expr) do { const char* gn_msg_ = (expr); if (gn_msg_) { set_error(gn_msg_); return BUDDY_ERR_ARG; } } while (0)

int buddy_groupnorm_act(const float* x, const float* gamma, const float* beta, float* y, float* stats, void* scratch, int B, int H, int W, int C,
                        int G, int mode, int silu, void* stream) {
  GN_REFUSE((!x || !gamma || !beta || !y || !stats || !scratch) ? "groupnorm: null pointer" : nullptr);
  GN_REFUSE(gn_refusal(B, H, W, C, G, mode, 0));
  Src2 s; s.p0 = x; s.p1 = nullptr; s.C0 = C; s.ld0 = C; s.ld1 = 0;
  launch_gn_stats(s, B, H * W, C, G, 1e-6f, (double*)scratch, stats, (hipStream_t)stream);
  launch_gn_apply(s, stats, gamma, beta, B, H, W, C, G, mode, silu, y, nullptr, (hipStream_t)stream);
  return finish();
}

int buddy_groupnorm_act_bwd(const float* x, const float* gamma, const float* beta, const float* stats, const float* dy, float* dx, void* scratch,
                            float* red, int B, int H, int W, int C, int G, int mode, int silu, void* stream) {
  GN_REFUSE((!x || !gamma || !beta || !dy || !dx || !stats || !scratch || !red) ? "groupnorm: null pointer" : nullptr);
  GN_REFUSE(gn_refusal(B, H, W, C, G, mode, 0));
  Src2 s; s.p0 = x; s.p1 = nullptr; s.C0 = C; s.ld0 = C; s.ld1 = 0;
  Dst2 d; d.p0 = dx; d.p1 = nullptr; d.C0 = C; d.ld0 = C; d.ld1 = 0; d.acc0 = 0; d.acc1 = 0;
  launch_gn_bwd(s, stats, gamma, beta, dy, B, H, W, C, G, mode, silu, nullptr, 0, 0.f, (double*)scratch, red, d, (hipStream_t)stream);
  return finish();
}

// The stand-alone GroupNorm launchers with everything they take: a (concatenated, strided) source view, both statistics routes, pooled_raw; and
// in the backward the extra gradient and a two-destination gradient view (tests/test_hip_groupnorm.py).
int buddy_groupnorm_view_fwd(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, const float* gamma, const float* beta, int G, int mode,
                             int silu, float* y, float* pooled_raw, float* stats, int route, double* csum0, double* csum1, double* scratch, int B,
                             int H, int W, void* stream) {
  GN_REFUSE((!x0 || !gamma || !beta || !y || !stats || !scratch) ? "groupnorm: null pointer" : nullptr);
  const int C = x1 ? C0 + C1 : C0;
  GN_REFUSE((C0 < 1 || (x1 && C1 < 1)) ? "groupnorm: B, H, W, C and G must be at least 1" : nullptr);
  GN_REFUSE(gn_refusal(B, H, W, C, G, mode, 0));
  GN_REFUSE(gn_view_refusal(x1, C0, C1, ld0, ld1, C));
  GN_REFUSE((route < 0 || route > 1) ? "groupnorm: route must be 0 (one reduction over the view) or 1 (per-source channel sums)" : nullptr);
  GN_REFUSE((route == 1 && (!csum0 || (x1 && !csum1))) ? "groupnorm: route 1 needs a csum buffer per source" : nullptr);
  GN_REFUSE((pooled_raw && mode != 1) ? "groupnorm: pooled_raw exists in mode 1 only" : nullptr);
  hipStream_t st = (hipStream_t)stream;
  Src2 s; s.p0 = x0; s.p1 = x1; s.C0 = C0; s.ld0 = ld0; s.ld1 = x1 ? ld1 : 0;
  if (route == 0) {
    launch_gn_stats(s, B, H * W, C, G, 1e-6f, scratch, stats, st);
  } else {
    launch_chan_sums(x0, B, H * W, C0, scratch, csum0, st, ld0);
    if (x1) launch_chan_sums(x1, B, H * W, C1, scratch, csum1, st, ld1);
    launch_gn_stats_csum(csum0, x1 ? csum1 : nullptr, C0, B, H * W, C, G, 1e-6f, stats, st);
  }
  launch_gn_apply(s, stats, gamma, beta, B, H, W, C, G, mode, silu, y, pooled_raw, st);
  return finish();
}

int buddy_groupnorm_view_bwd(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, const float* gamma, const float* beta,
                             const float* stats, const float* dy, int G, int mode, int silu, const float* extra, int extra_mode, float extra_scale,
                             float* dx0, int ldd0, int acc0, float* dx1, int ldd1, int acc1, int Cd0, double* scratch, float* red, int B, int H,
                             int W, void* stream) {
  GN_REFUSE((!x0 || !gamma || !beta || !stats || !dy || !dx0 || !scratch || !red) ? "groupnorm: null pointer" : nullptr);
  const int C = x1 ? C0 + C1 : C0;
  GN_REFUSE((C0 < 1 || (x1 && C1 < 1)) ? "groupnorm: B, H, W, C and G must be at least 1" : nullptr);
  GN_REFUSE(gn_refusal(B, H, W, C, G, mode, extra_mode));
  GN_REFUSE(gn_view_refusal(x1, C0, C1, ld0, ld1, C));
  GN_REFUSE(gn_view_refusal(dx1, Cd0, C - Cd0, ldd0, ldd1, C));
  GN_REFUSE(((extra_mode != 0) != (extra != nullptr)) ? "groupnorm: extra and extra_mode go together" : nullptr);
  Src2 s; s.p0 = x0; s.p1 = x1; s.C0 = C0; s.ld0 = ld0; s.ld1 = x1 ? ld1 : 0;
  Dst2 d; d.p0 = dx0; d.p1 = dx1; d.C0 = Cd0; d.ld0 = ldd0; d.ld1 = dx1 ? ldd1 : 0; d.acc0 = acc0 ? 1 : 0; d.acc1 = (dx1 && acc1) ? 1 : 0;
  launch_gn_bwd(s, stats, gamma, beta, dy, B, H, W, C, G, mode, silu, extra, extra_mode, extra_scale, scratch, red, d, (hipStream_t)stream, 0);
  return finish();
}

int buddy_options_check(void) { return options_check(); }
int buddy_option_validate(const char* key, int value) { Options o = default_options(); return option_set(o, key, value); }
int buddy_ncsnpp_set_option(void* h, const char* key, int value) { if (!h) { set_error("null handle"); return BUDDY_ERR_ARG; } return net_set_option((Net*)h, key, value); }
int buddy_ncsnpp_get_option(void* h, const char* key, int* value) { if (!h) { set_error("null handle"); return BUDDY_ERR_ARG; } return net_get_option((Net*)h, key, value); }
int buddy_ncsnpp_set_gemm(void* h, int mode) { if (!h) { set_error("null handle"); return BUDDY_ERR_ARG; } return net_set_gemm((Net*)h, mode); }
int buddy_ncsnpp_set_attention(void* h, int mode) { if (!h) { set_error("null handle"); return BUDDY_ERR_ARG; } return net_set_attention((Net*)h, mode); }
int buddy_ncsnpp_set_fir(void* h, int fir) { if (!h) { set_error("null handle"); return BUDDY_ERR_ARG; } return net_set_fir((Net*)h, fir); }
int buddy_fir_resample2(const float* x, float* y, int B, int H, int W, int C, int up, float scale, int accumulate, void* stream) {
  if (!x || !y || B < 1 || H < 1 || W < 1 || C < 1 || (!up && ((H | W) & 1))) { set_error("bad resample arguments"); return BUDDY_ERR_ARG; }
  if (up) launch_fir_up2(x, y, B, H, W, C, scale, accumulate, (hipStream_t)stream);
  else launch_fir_down2(x, y, B, H, W, C, scale, accumulate, (hipStream_t)stream);
  return finish();
}

int buddy_flash_attention_fwd(const float* q, const float* k, const float* v, float* O, float* lse, int B, int T, int C, float scale, int prec,
                              void* stream) {
  if (!q || !k || !v || !O || !lse || B < 1 || T < 1 || !flash_attn_supported(C) || prec != 0) {
    set_error("bad attention arguments (C in {32, 64, 128, 256}; prec 0 -- the 16-bit-operand kernels are buddy_flash_attention16_*)"); return BUDDY_ERR_ARG;
  }
  launch_flash_attn_fwd(q, k, v, O, lse, B, T, C, scale, nullptr, 1, (hipStream_t)stream);
  return finish();
}
long long buddy_flash_attention16_workspace(int B, int T, int C) { return (B < 1 || T < 1 || !flash_attn16_supported(C)) ? 0 : flash_attn16_ws_floats(B, T, C); }
int buddy_flash_attention16_fwd(const float* q, const float* k, const float* v, float* O, float* lse, int B, int T, int C, float scale, int prec, float* ws,
                                void* stream) {
  if (!q || !k || !v || !O || !lse || !ws || B < 1 || T < 1 || !flash_attn16_supported(C) || prec < 1 || prec > 2) {
    set_error("bad attention arguments (C in {64, 128, 256}; prec 1 = bf16, 2 = f16; ws = buddy_flash_attention16_workspace floats)"); return BUDDY_ERR_ARG;
  }
  launch_flash_attn16_fwd(q, k, v, O, lse, B, T, C, scale, prec, ws, (hipStream_t)stream);
  return finish();
}
int buddy_flash_attention16_bwd(const float* q, const float* k, const float* v, const float* O, const float* dO, const float* lse, float* delta, float* dq,
                                float* dk, float* dv, int B, int T, int C, float scale, int prec, float* ws, void* stream) {
  if (!q || !k || !v || !O || !dO || !lse || !delta || !dq || !dk || !dv || !ws || B < 1 || T < 1 || !flash_attn16_supported(C) || prec < 1 || prec > 2) {
    set_error("bad attention arguments (C in {64, 128, 256}; prec 1 = bf16, 2 = f16; ws = buddy_flash_attention16_workspace floats)"); return BUDDY_ERR_ARG;
  }
  launch_flash_attn16_bwd(q, k, v, O, dO, lse, delta, dq, dk, dv, B, T, C, scale, prec, ws, (hipStream_t)stream);
  return finish();
}
long long buddy_flash_attention_workspace(int B, int T, int C, int splits) {
  if (B < 1 || T < 1 || !flash_attn_supported(C)) return 0;
  return flash_attn_ws_floats(B, T, C, splits > 0 ? splits : flash_attn_splits(B, T));
}
int buddy_flash_attention_splits(int B, int T) { return (B < 1 || T < 1) ? 1 : flash_attn_splits(B, T); }
static bool split_args_ok(int T, int splits, const float* ws) {
  const int nb = (T + 31) / 32;
  if (splits < 1 || splits > nb || (splits > 1 && !ws)) return false;
  return splits == 1 || (long long)((nb + splits - 1) / splits) * (splits - 1) < nb;     // every split non-empty
}
int buddy_flash_attention_fwd_split(const float* q, const float* k, const float* v, float* O, float* lse, int B, int T, int C, float scale, int splits,
                                    float* ws, void* stream) {
  if (!q || !k || !v || !O || !lse || B < 1 || T < 1 || !flash_attn_supported(C) || !split_args_ok(T, splits, ws)) {
    set_error("bad split-attention arguments (C in {32, 64, 128, 256}; every split needs at least one 32-row block)"); return BUDDY_ERR_ARG;
  }
  launch_flash_attn_fwd(q, k, v, O, lse, B, T, C, scale, ws, splits, (hipStream_t)stream);
  return finish();
}
int buddy_flash_attention_bwd_split(const float* q, const float* k, const float* v, const float* O, const float* dO, const float* lse, float* delta,
                                    float* dq, float* dk, float* dv, int B, int T, int C, float scale, int splits, float* ws, void* stream) {
  if (!q || !k || !v || !O || !dO || !lse || !delta || !dq || !dk || !dv || B < 1 || T < 1 || !flash_attn_supported(C) || !split_args_ok(T, splits, ws)) {
    set_error("bad split-attention arguments (C in {32, 64, 128, 256}; every split needs at least one 32-row block)"); return BUDDY_ERR_ARG;
  }
  launch_flash_attn_bwd(q, k, v, O, dO, lse, delta, dq, dk, dv, B, T, C, scale, ws, splits, (hipStream_t)stream);
  return finish();
}
int buddy_flash_attention_bwd(const float* q, const float* k, const float* v, const float* O, const float* dO, const float* lse, float* delta, float* dq,
                              float* dk, float* dv, int B, int T, int C, float scale, int prec, void* stream) {
  if (prec != 0 || !q || !k || !v || !O || !dO || !lse || !delta || !dq || !dk || !dv || B < 1 || T < 1 || !flash_attn_supported(C)) {
    set_error("bad attention arguments (C in {32, 64, 128, 256}; prec 0 -- the 16-bit-operand kernels are buddy_flash_attention16_*)"); return BUDDY_ERR_ARG;
  }
  launch_flash_attn_bwd(q, k, v, O, dO, lse, delta, dq, dk, dv, B, T, C, scale, nullptr, 1, (hipStream_t)stream);
  return finish();
}

int buddy_axpby_rows(const float* x, const float* y, const float* a, const float* c, float* out, int B, int L, void* stream) {
  if (!x || !a || !out || (y && !c)) { set_error("null argument"); return BUDDY_ERR_ARG; }
  if (B < 1 || L < 1) { set_error("axpby_rows: B and L must be >= 1"); return BUDDY_ERR_ARG; }
  launch_axpby_rows(x, y, a, c, out, B, L, (hipStream_t)stream);
  return finish();
}

int buddy_perturb(const float* x, const float* eps, float scale, float* out, long long n, void* stream) {
  if (!x || !eps || !out) { set_error("null argument"); return BUDDY_ERR_ARG; }
  if (n < 1) { set_error("perturb: n must be >= 1"); return BUDDY_ERR_ARG; }
  launch_perturb(x, eps, scale, out, n, (hipStream_t)stream);
  return finish();
}

int buddy_dps_update(const float* x_hat, const float* x_den, const float* lh, const float* lh_scale, const float* den_scale, const float* base,
                     const float* d_prev, float t, float dt, float w_prev, float w_cur, float* out, float* d_out, float* x_den_out, int B, int L, void* stream) {
  if (!x_hat || !x_den || !base || !out || !(t > 0.f) || B < 1 || L < 1) {       // !(t > 0): a NaN sigma is refused too
    set_error("dps_update: null argument, t not > 0, or B / L < 1"); return BUDDY_ERR_ARG;
  }
  launch_dps_update(x_hat, x_den, lh, lh_scale, den_scale, base, d_prev, t, dt, w_prev, w_cur, out, d_out, x_den_out, B, L, (hipStream_t)stream);
  return finish();
}
int buddy_row_scale(const float* x, float* out, int B, int L, int mode, float p0, float p1, void* stream) {
  if (!x || !out || B < 1 || L < 2 || (mode != 0 && mode != 1) || (mode == 1 && !(p1 > 0.f))) { set_error("row_scale: mode 0 (p0 / std) or 1 (p0 / (norm / p1 + 1e-8)), L >= 2"); return BUDDY_ERR_ARG; }
  launch_row_scale(x, out, B, L, mode, p0, p1, (hipStream_t)stream);
  return finish();
}
int buddy_fill_rows4(float* out, int B, float v0, float v1, float v2, float v3, void* stream) {
  if (!out || B < 1) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  launch_fill_rows4(out, B, v0, v1, v2, v3, (hipStream_t)stream);
  return finish();
}

int buddy_row_moments(const float* x, double* out, int B, int L, void* stream) {
  if (!x || !out) { set_error("null argument"); return BUDDY_ERR_ARG; }
  if (B < 1 || L < 1) { set_error("row_moments: B and L must be >= 1"); return BUDDY_ERR_ARG; }
  launch_row_moments(x, out, B, L, (hipStream_t)stream);
  return finish();
}

int buddy_fir(const float* x, const float* h, long long h_stride, float* y, int B, int L, int M, int adjoint, void* stream) {
  if (!x || !h || !y || M < 1 || B < 1 || L < 1 || B > 65535) {      // the batch is gridDim.y
    set_error("bad fir arguments (M, L >= 1, 1 <= B <= 65535)"); return BUDDY_ERR_ARG;
  }
  launch_fir(x, h, h_stride, y, B, L, M, adjoint, (hipStream_t)stream);
  return finish();
}


// ---- rational polyphase resampler (resample.hip) ----
int buddy_resample(const float* x, int B, long long Lin, const float* h, int Nh, int up, int down, float* y, long long Lout, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_resample: ") + why); return BUDDY_ERR_ARG; };
  if (!x || !h || !y) return bad("null pointer");
  if (B < 1 || Lin < 1) return bad("B and Lin must be >= 1");
  if (Lin > (1LL << 40)) return bad("Lin above 2^40");
  if (up < 1 || down < 1 || up > 1024 || down > 1024) return bad("up and down must be in 1..1024");
  int a = up, b = down;
  while (b) { const int t = a % b; a = b; b = t; }
  if (a != 1) return bad("up / down is not in lowest terms");
  if (Nh < 1 || Nh % 2 == 0 || Nh > 65537) return bad("Nh must be odd and <= 65537");
  if (Lout != (Lin * up + down - 1) / down) return bad("Lout is not ceil(Lin * up / down)");
  if (resample_tiles(Lout) * B > 0x7fffffffLL) return bad("more output tiles than one grid holds");
  launch_resample(x, B, Lin, h, Nh, up, down, y, Lout, (hipStream_t)stream);
  return finish();
}

// ---- room-acoustic analysis of RIR rows (acoustics.hip) ----
// The row lengths are a device array: one small copy to the host (after the work queued on `stream`) so that a bad length or a stride below the
// longest row is refused before anything is launched.  On a host without a HIP device no device pointer exists and the array is read where it lies.
static int fetch_lengths(const int* lens, int B, std::vector<int>& host, void* stream, const char* who) {
  host.resize(B);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    (void)hipGetLastError();
    std::memcpy(host.data(), lens, sizeof(int) * (size_t)B);
    return BUDDY_OK;
  }
  hipError_t e = hipMemcpyAsync(host.data(), lens, sizeof(int) * (size_t)B, hipMemcpyDefault, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) { set_error(std::string(who) + ": reading the row lengths: " + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  return BUDDY_OK;
}

int buddy_decay_tile(void) { return decay_tile(); }

int buddy_row_argmax_abs(const float* h, const int* lens, int B, long long ldh, int* n0, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_row_argmax_abs: ") + why); return BUDDY_ERR_ARG; };
  if (!h || !lens || !n0) return bad("null pointer");
  if (B < 1 || B > 65535) return bad("B must be in 1..65535");
  if (ldh < 1) return bad("ldh must be >= 1");
  std::vector<int> len;
  if (int rc = fetch_lengths(lens, B, len, stream, "buddy_row_argmax_abs")) return rc;
  for (int b = 0; b < B; ++b) {
    if (len[b] < 1 || len[b] > (1 << 30)) return bad("every lens[b] must be in 1..2^30");
    if (len[b] > ldh) return bad("ldh is smaller than the longest row");
  }
  launch_row_argmax_abs(h, lens, B, ldh, n0, (hipStream_t)stream);
  return finish();
}

int buddy_fir_bank(const float* h, const int* lens, int B, long long ldh, const float* bank, int nb, int Nh, float* g, long long ldg, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_fir_bank: ") + why); return BUDDY_ERR_ARG; };
  if (!h || !lens || !bank || !g) return bad("null pointer");
  if (B < 1 || B > 65535 || nb < 1 || nb > 65535) return bad("B and nb must be in 1..65535");
  if (Nh < 1 || Nh % 2 == 0 || Nh > 65537) return bad("Nh must be odd and <= 65537");
  if (ldh < 1 || ldg < 1) return bad("ldh and ldg must be >= 1");
  std::vector<int> len;
  if (int rc = fetch_lengths(lens, B, len, stream, "buddy_fir_bank")) return rc;
  const int P = (Nh - 1) / 2;
  int longest = 0;
  for (int b = 0; b < B; ++b) {
    if (len[b] < 1 || len[b] > (1 << 30)) return bad("every lens[b] must be in 1..2^30");
    if (len[b] > ldh) return bad("ldh is smaller than the longest row");
    if ((long long)len[b] + P > ldg) return bad("ldg is smaller than the longest row plus (Nh - 1) / 2");
    longest = len[b] > longest ? len[b] : longest;
  }
  launch_fir_bank(h, lens, B, ldh, longest, bank, nb, Nh, g, ldg, (hipStream_t)stream);
  return finish();
}

int buddy_decay_metrics(const float* g, const int* lens_g, const int* n0, int B, int nb, long long ldg, int fs, double* out, int* flags, float* edc_db,
                        void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_decay_metrics: ") + why); return BUDDY_ERR_ARG; };
  if (!g || !lens_g || !n0 || !out || !flags) return bad("null pointer");
  if (B < 1 || B > 65535 || nb < 1 || nb > 65535 || (long long)B * nb > 0x7fffffffLL) return bad("B and nb must be in 1..65535");
  if (fs < 1) return bad("fs must be >= 1");
  if (ldg < 1) return bad("ldg must be >= 1");
  std::vector<int> len;
  if (int rc = fetch_lengths(lens_g, B, len, stream, "buddy_decay_metrics")) return rc;
  for (int b = 0; b < B; ++b) {
    if (len[b] < 1 || len[b] > (1 << 30) + 32768) return bad("every lens_g[b] must be in 1..2^30 + 2^15");
    if (len[b] > ldg) return bad("ldg is smaller than the longest row");
  }
  launch_decay_metrics(g, lens_g, n0, B, nb, ldg, fs, out, flags, edc_db, (hipStream_t)stream);
  return finish();
}

// ---- objective evaluation of (estimate, clean) pairs (metrics.hip) ----
// the lengths of ragged rows, fetched once: each in lo..2^30 and within the stride; *longest receives the largest
static int check_rows(const int* lens, int B, long long ld, int lo, void* stream, const char* who, int* longest) {
  auto bad = [who](const char* why) { set_error(std::string(who) + ": " + why); return BUDDY_ERR_ARG; };
  if (B < 1 || B > 65535) return bad("B must be in 1..65535");
  if (ld < 1) return bad("the row stride must be >= 1");
  std::vector<int> len;
  if (int rc = fetch_lengths(lens, B, len, stream, who)) return rc;
  *longest = 0;
  for (int b = 0; b < B; ++b) {
    if (len[b] < lo || len[b] > (1 << 30)) return bad(lo ? "every length must be in 1..2^30" : "every length must be in 0..2^30");
    if (len[b] > ld) return bad("the row stride is smaller than the longest row");
    *longest = len[b] > *longest ? len[b] : *longest;
  }
  return BUDDY_OK;
}
static long long at_least_one(long long v) { return v > 1 ? v : 1; }

int buddy_metrics_tile(void) { return metrics_tile(); }

int buddy_pair_moments(const float* e, const float* x, const int* lens, int B, long long ld, double* out, int* flags, void* stream) {
  if (!e || !x || !lens || !out || !flags) { set_error("buddy_pair_moments: null pointer"); return BUDDY_ERR_ARG; }
  int longest;
  if (int rc = check_rows(lens, B, ld, 1, stream, "buddy_pair_moments", &longest)) return rc;
  launch_pair_moments(e, x, lens, B, ld, out, flags, (hipStream_t)stream);
  return finish();
}

long long buddy_stoi_select_workspace(int B, long long max_len) {
  if (B < 1 || max_len < 1 || max_len > (1LL << 30)) return -1;
  return 8LL * B * at_least_one(metrics_frames(max_len));
}

int buddy_stoi_select(const float* x, const float* e, const int* lens, int B, long long ld, float* xo, float* eo, long long ldo, int* lens_out, int* K, int* F,
                      int* src, long long ldf, void* ws, long long ws_bytes, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_stoi_select: ") + why); return BUDDY_ERR_ARG; };
  if (!x || !e || !lens || !xo || !eo || !lens_out || !K || !F || !src || !ws) return bad("null pointer");
  int longest;
  if (int rc = check_rows(lens, B, ld, 1, stream, "buddy_stoi_select", &longest)) return rc;
  const long long maxF = metrics_frames(longest);
  if (ldf < at_least_one(maxF)) return bad("ldf is smaller than the frames of the longest row");
  if (ldo < 1 || (maxF > 0 && ldo < (maxF - 1) * 128 + 256)) return bad("ldo is smaller than the full frames of the longest row");
  if (ws_bytes < 8LL * B * ldf) return bad("the workspace is smaller than 8 B ldf bytes");
  launch_stoi_select(x, e, lens, B, ld, longest, xo, eo, ldo, lens_out, K, F, src, ldf, (double*)ws, (hipStream_t)stream);
  return finish();
}

int buddy_band_spectra(const float* x, const int* lens, int B, long long ld, const int* lo, const int* hi, int J, float* out, long long ldm, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_band_spectra: ") + why); return BUDDY_ERR_ARG; };
  if (!x || !lens || !lo || !hi || !out) return bad("null pointer");
  if (J < 1 || J > 32) return bad("J must be in 1..32");
  for (int j = 0; j < J; ++j)
    if (lo[j] < 0 || hi[j] < lo[j] || hi[j] > 257) return bad("every band must be bins [lo, hi) with 0 <= lo <= hi <= 257");
  int longest;
  if (int rc = check_rows(lens, B, ld, 0, stream, "buddy_band_spectra", &longest)) return rc;      // a row without a kept frame has length 0
  if (ldm < at_least_one(metrics_frames(longest))) return bad("ldm is smaller than the frames of the longest row");
  launch_band_spectra(x, lens, B, ld, longest, lo, hi, J, out, ldm, (hipStream_t)stream);
  return finish();
}

long long buddy_stoi_scores_workspace(int B, int max_frames) {
  if (B < 1 || max_frames < 0) return -1;
  return 16LL * B * at_least_one((long long)max_frames - 29);
}

int buddy_stoi_scores(const float* X, const float* Y, const int* lens_m, int B, int J, long long ldm, double* out, int* flags, void* ws, long long ws_bytes,
                      void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_stoi_scores: ") + why); return BUDDY_ERR_ARG; };
  if (!X || !Y || !lens_m || !out || !flags || !ws) return bad("null pointer");
  if (J < 1 || J > 32) return bad("J must be in 1..32");
  int longest;
  if (int rc = check_rows(lens_m, B, ldm, 0, stream, "buddy_stoi_scores", &longest)) return rc;
  if (ws_bytes < buddy_stoi_scores_workspace(B, longest)) return bad("the workspace is smaller than buddy_stoi_scores_workspace(B, longest row)");
  launch_stoi_scores(X, Y, lens_m, B, J, ldm, longest, out, flags, (double*)ws, (hipStream_t)stream);
  return finish();
}

long long buddy_lsd_workspace(int B, long long max_len) { return buddy_stoi_select_workspace(B, max_len); }

int buddy_frame_power(const float* x, const int* lens, int B, long long ld, double* mean_p, void* ws, long long ws_bytes, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_frame_power: ") + why); return BUDDY_ERR_ARG; };
  if (!x || !lens || !mean_p || !ws) return bad("null pointer");
  int longest;
  if (int rc = check_rows(lens, B, ld, 1, stream, "buddy_frame_power", &longest)) return rc;
  if (ws_bytes < buddy_lsd_workspace(B, longest)) return bad("the workspace is smaller than buddy_lsd_workspace(B, longest row)");
  launch_frame_power(x, lens, B, ld, longest, mean_p, (double*)ws, (hipStream_t)stream);
  return finish();
}

int buddy_lsd(const float* e, const float* x, const int* lens, int B, long long ld, const double* gain, const double* delta, double* out, int* flags, void* ws,
              long long ws_bytes, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_lsd: ") + why); return BUDDY_ERR_ARG; };
  if (!e || !x || !lens || !gain || !delta || !out || !flags || !ws) return bad("null pointer");
  int longest;
  if (int rc = check_rows(lens, B, ld, 1, stream, "buddy_lsd", &longest)) return rc;
  if (ws_bytes < buddy_lsd_workspace(B, longest)) return bad("the workspace is smaller than buddy_lsd_workspace(B, longest row)");
  launch_lsd(e, x, lens, B, ld, longest, gain, delta, out, flags, (double*)ws, (hipStream_t)stream);
  return finish();
}

// ---- time alignment of a pair before it is scored (align.hip) ----
int buddy_align_tile(void) { return align_tile(); }
int buddy_align_lag_tile(void) { return align_lag_tile(); }

long long buddy_xcorr_lag_workspace(int B, long long max_len, int K) {
  if (B < 1 || B > 65535 || max_len < 1 || max_len > (1LL << 30) || K < 0 || K > 65535) return -1;
  return 8LL * xcorr_workspace_doubles(B, max_len, K);
}

int buddy_xcorr_lag(const float* e, const float* x, const int* lens, int B, long long ld, int K, int* lag, double* out, int* flags, double* r_out, void* ws,
                    long long ws_bytes, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_xcorr_lag: ") + why); return BUDDY_ERR_ARG; };
  if (!e || !x || !lens || !lag || !out || !flags || !ws) return bad("null pointer");
  if (K < 0 || K > 65535) return bad("K must be in 0..65535");
  int longest;
  if (int rc = check_rows(lens, B, ld, 1, stream, "buddy_xcorr_lag", &longest)) return rc;
  if (ws_bytes < buddy_xcorr_lag_workspace(B, longest, K)) return bad("the workspace is smaller than buddy_xcorr_lag_workspace(B, longest row, K)");
  launch_xcorr_lag(e, x, lens, B, ld, longest, K, lag, out, flags, r_out, (double*)ws, (hipStream_t)stream);
  return finish();
}

int buddy_align_pair(const float* e, const float* x, const int* lens, const int* lag, int B, long long ld, float* eo, float* xo, long long ldo, int* lens_out,
                     void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_align_pair: ") + why); return BUDDY_ERR_ARG; };
  if (!e || !x || !lens || !lag || !eo || !xo || !lens_out) return bad("null pointer");
  if (B < 1 || B > 65535) return bad("B must be in 1..65535");
  if (ld < 1 || ldo < 1 || ldo > 0x7fffffffLL) return bad("the row strides must be >= 1, ldo below 2^31");
  std::vector<int> len, d;
  if (int rc = fetch_lengths(lens, B, len, stream, "buddy_align_pair")) return rc;
  if (int rc = fetch_lengths(lag, B, d, stream, "buddy_align_pair")) return rc;
  for (int b = 0; b < B; ++b) {
    if (len[b] < 1 || len[b] > (1 << 30)) return bad("every length must be in 1..2^30");
    if (len[b] > ld) return bad("the row stride is smaller than the longest row");
    if (d[b] <= -len[b] || d[b] >= len[b]) return bad("every |lag[b]| must be below lens[b]");
    if (len[b] - (d[b] < 0 ? -d[b] : d[b]) > ldo) return bad("ldo is smaller than the longest overlap");
  }
  launch_align_pair(e, x, lens, lag, B, ld, eo, xo, ldo, lens_out, (hipStream_t)stream);
  return finish();
}

// ---- projection SDR of a pair over filter lengths (sdr.hip) ----
int buddy_sdr_tile(void) { return sdr_tile(); }
int buddy_sdr_lag_tile(void) { return sdr_lag_tile(); }

long long buddy_sdr_products_workspace(int B, long long max_len, int N) {
  if (B < 1 || B > 65535 || max_len < 1 || max_len > (1LL << 30) || N < 1 || N > sdr_max_order()) return -1;
  return 8LL * sdr_products_workspace_doubles(B, max_len, N);
}

int buddy_sdr_products(const float* e, const float* x, const int* lens, int B, long long ld, int N, double* r, double* d, double* ee, void* ws, long long ws_bytes,
                       void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_sdr_products: ") + why); return BUDDY_ERR_ARG; };
  if (!e || !x || !lens || !r || !d || !ee || !ws) return bad("null pointer");
  if (N < 1 || N > sdr_max_order()) return bad("N must be in 1..2048");
  int longest;
  if (int rc = check_rows(lens, B, ld, 1, stream, "buddy_sdr_products", &longest)) return rc;
  if (ws_bytes < buddy_sdr_products_workspace(B, longest, N)) return bad("the workspace is smaller than buddy_sdr_products_workspace(B, longest row, N)");
  launch_sdr_products(e, x, lens, B, ld, longest, N, r, d, ee, (double*)ws, (hipStream_t)stream);
  return finish();
}

int buddy_sdr_solve(const double* r, const double* d, const double* ee, const int* lens, int B, int N, const int* orders, int J, double loading, double* sdr,
                    double* p, int* flags, double* h, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_sdr_solve: ") + why); return BUDDY_ERR_ARG; };
  if (!r || !d || !ee || !lens || !orders || !sdr || !p || !flags) return bad("null pointer");
  if (N < 1 || N > sdr_max_order()) return bad("N must be in 1..2048");
  if (J < 1 || J > sdr_max_orders()) return bad("J must be in 1..8");
  for (int j = 0; j < J; ++j)
    if (orders[j] < 1 || orders[j] > N || (j && orders[j] <= orders[j - 1])) return bad("the orders must be strictly ascending within 1..N");
  if (!(loading >= 0.0) || !std::isfinite(loading)) return bad("the loading must be finite and >= 0");
  int longest;
  if (int rc = check_rows(lens, B, 1LL << 30, 1, stream, "buddy_sdr_solve", &longest)) return rc;
  if (launch_sdr_solve(r, d, ee, lens, B, N, orders, J, loading, sdr, p, flags, h, (hipStream_t)stream)) {
    set_error("buddy_sdr_solve: LDS request refused"); return BUDDY_ERR_HIP;
  }
  return finish();
}

// ---- non-intrusive SRMR of single signals (srmr.hip) ----
int buddy_srmr_tile(void) { return srmr_tile(); }
int buddy_modulation_chunk(void) { return modulation_chunk(); }

int buddy_gammatone_env(const float* x, const int* lens, int B, long long ld, const float* g_re, const float* g_im, const int* tap_off, int J, float* env,
                        long long lde, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_gammatone_env: ") + why); return BUDDY_ERR_ARG; };
  if (!x || !lens || !g_re || !g_im || !tap_off || !env) return bad("null pointer");
  if (J < 1 || J > 32) return bad("J must be in 1..32");
  if (tap_off[0] < 0) return bad("tap_off[0] must be >= 0");
  for (int j = 0; j < J; ++j)
    if (tap_off[j + 1] - tap_off[j] < 1 || tap_off[j + 1] - tap_off[j] > srmr_max_taps()) return bad("every channel must have 1..1536 taps");
  int longest;
  if (int rc = check_rows(lens, B, ld, 1, stream, "buddy_gammatone_env", &longest)) return rc;
  if (lde < longest) return bad("lde is smaller than the longest row");
  launch_gammatone_env(x, lens, B, ld, longest, g_re, g_im, tap_off, J, env, lde, (hipStream_t)stream);
  return finish();
}

int buddy_modulation_energies(const float* env, const int* lens, int B, int J, long long lde, const double* coef, int K, int W, int H, double* E, long long ldm,
                              int* frames, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_modulation_energies: ") + why); return BUDDY_ERR_ARG; };
  if (!env || !lens || !coef || !E || !frames) return bad("null pointer");
  if (J < 1 || J > 32) return bad("J must be in 1..32");
  if (K < 1 || K > 8) return bad("K must be in 1..8");
  if (H < 1 || H % modulation_chunk() != 0 || W != 4 * H || W > modulation_max_window()) return bad("the window must be four hops, the hop a multiple of 256, W <= 4096");
  for (int k = 0; k < K; ++k)
    if (coef[k * 6 + 3] != 1.0) return bad("every filter must be normalised to a0 = 1");
  int longest;
  if (int rc = check_rows(lens, B, lde, 1, stream, "buddy_modulation_energies", &longest)) return rc;
  if (ldm < at_least_one(longest >= W ? (longest - W) / H + 1 : 0)) return bad("ldm is smaller than the frames of the longest row");
  launch_modulation_energies(env, lens, B, J, lde, coef, K, W, H, E, ldm, frames, (hipStream_t)stream);
  return finish();
}

int buddy_srmr_scores(const double* E, const int* frames, int B, int J, int K, long long ldm, const double* erb, const double* l, double* out, double* Ebar,
                      int* flags, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_srmr_scores: ") + why); return BUDDY_ERR_ARG; };
  if (!E || !frames || !erb || !l || !out || !Ebar || !flags) return bad("null pointer");
  if (J < 1 || J > 32) return bad("J must be in 1..32");
  if (K != 8) return bad("K must be 8 (the ratio is bands 0..3 over bands 4..K* - 1, K* in 5..8)");
  int longest;
  if (int rc = check_rows(frames, B, ldm, 0, stream, "buddy_srmr_scores", &longest)) return rc;
  launch_srmr_scores(E, frames, B, J, ldm, erb, l, out, Ebar, flags, (hipStream_t)stream);
  return finish();
}

// ---- blind decay time of single signals (decay.hip) ----
int buddy_decay_regions_tile(void) { return decay_regions_tile(); }

int buddy_decay_energies(const float* x, const int* lens, int B, long long ld, const int* lo_bins, const int* hi_bins, int NB, double* E, long long ldm,
                         int* frames, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_decay_energies: ") + why); return BUDDY_ERR_ARG; };
  if (!x || !lens || !lo_bins || !hi_bins || !E || !frames) return bad("null pointer");
  if (NB < 1 || NB > 8) return bad("NB must be in 1..8");
  for (int i = 0; i < NB; ++i)
    if (lo_bins[i] < 0 || hi_bins[i] < lo_bins[i] || hi_bins[i] > decay_bins()) return bad("every band must be a bin range 0 <= lo <= hi <= 257");
  int longest;
  if (int rc = check_rows(lens, B, ld, 1, stream, "buddy_decay_energies", &longest)) return rc;
  const long long maxF = frames_of(longest, decay_frame(), decay_hop());
  if (ldm < at_least_one(maxF)) return bad("ldm is smaller than the frames of the longest row");
  launch_decay_energies(x, lens, B, ld, maxF, lo_bins, hi_bins, NB, E, ldm, frames, (hipStream_t)stream);
  return finish();
}

int buddy_decay_regions(const double* E, const int* frames, int B, int NB, long long ldm, int K, int lmin, double q, double floor_rel, double* T, int* len,
                        void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_decay_regions: ") + why); return BUDDY_ERR_ARG; };
  if (!E || !frames || !T || !len) return bad("null pointer");
  if (NB < 1 || NB > 8) return bad("NB must be in 1..8");
  if (K < 1 || K > 8) return bad("K must be in 1..8");
  if (lmin < 2) return bad("lmin must be >= 2");
  if (!(q > 0.0 && q <= 1.0)) return bad("q must be in (0, 1]");
  if (!(floor_rel >= 0.0 && floor_rel < 1.0)) return bad("floor_rel must be in [0, 1)");
  int longest;
  if (int rc = check_rows(frames, B, ldm, 0, stream, "buddy_decay_regions", &longest)) return rc;
  launch_decay_regions(E, frames, B, NB, ldm, K, lmin, q, floor_rel, T, len, (hipStream_t)stream);
  return finish();
}

int buddy_decay_select(const double* T, const int* frames, int B, int NB, long long ldm, double* out, int* counts, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_decay_select: ") + why); return BUDDY_ERR_ARG; };
  if (!T || !frames || !out || !counts) return bad("null pointer");
  if (NB < 1 || NB > 8) return bad("NB must be in 1..8");
  int longest;
  if (int rc = check_rows(frames, B, ldm, 0, stream, "buddy_decay_select", &longest)) return rc;
  launch_decay_select(T, frames, B, NB, ldm, out, counts, (hipStream_t)stream);
  return finish();
}

// ---- active speech level of single signals (level.hip) ----
int buddy_level_tile(void) { return level_tile(); }
int buddy_level_counts_tile(void) { return level_counts_tile(); }
static bool level_shape_ok(int B, long long max_len) { return B >= 1 && B <= 65535 && max_len >= 0 && max_len <= (1LL << 30); }
long long buddy_level_stats_workspace(int B, long long max_len) { return level_shape_ok(B, max_len) ? level_stats_ws_bytes(B, max_len) : -1; }
long long buddy_level_classes_workspace(int B, long long max_len) { return level_shape_ok(B, max_len) ? level_classes_ws_bytes(B, max_len) : -1; }
long long buddy_level_counts_workspace(int B, long long max_len) { return level_shape_ok(B, max_len) ? level_counts_ws_bytes(B, max_len) : -1; }

int buddy_level_stats(const float* x, long long ldx, const int* lengths, int B, double* out, void* ws, long long ws_bytes, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_level_stats: ") + why); return BUDDY_ERR_ARG; };
  if (!x || !lengths || !out || !ws) return bad("null pointer");
  int longest;
  if (int rc = check_rows(lengths, B, ldx, 0, stream, "buddy_level_stats", &longest)) return rc;
  if (ws_bytes < level_stats_ws_bytes(B, longest)) return bad("the workspace is smaller than buddy_level_stats_workspace(B, longest row)");
  launch_level_stats(x, ldx, lengths, B, longest, out, ws, (hipStream_t)stream);
  return finish();
}

int buddy_level_classes(const float* x, long long ldx, const int* lengths, const double* offset, const double* ref, int B, double fs, double tc,
                        unsigned char* klass, long long ldk, double* sq, void* ws, long long ws_bytes, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_level_classes: ") + why); return BUDDY_ERR_ARG; };
  if (!x || !lengths || !ref || !klass || !sq || !ws) return bad("null pointer");
  if (!(fs > 0.0) || !std::isfinite(fs)) return bad("fs must be finite and > 0");
  if (!(tc > 0.0) || !std::isfinite(tc)) return bad("tc must be finite and > 0");
  int longest;
  if (int rc = check_rows(lengths, B, ldx, 0, stream, "buddy_level_classes", &longest)) return rc;
  if (ldk < 1 || ldk < longest) return bad("ldk is smaller than the longest row");
  if (ws_bytes < level_classes_ws_bytes(B, longest)) return bad("the workspace is smaller than buddy_level_classes_workspace(B, longest row)");
  std::vector<double> rh((size_t)B * 2, 0.0);  // ref, then offset: device doubles, read like the lengths
  int ndev = 0;
  const bool on_host = hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1;
  if (on_host) {
    (void)hipGetLastError();
    std::memcpy(rh.data(), ref, sizeof(double) * (size_t)B);
    if (offset) std::memcpy(rh.data() + B, offset, sizeof(double) * (size_t)B);
  } else {
    hipError_t e = hipMemcpyAsync(rh.data(), ref, sizeof(double) * (size_t)B, hipMemcpyDefault, (hipStream_t)stream);
    if (e == hipSuccess && offset) e = hipMemcpyAsync(rh.data() + B, offset, sizeof(double) * (size_t)B, hipMemcpyDefault, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { set_error(std::string("buddy_level_classes: reading ref / offset: ") + hipGetErrorString(e)); return BUDDY_ERR_HIP; }
  }
  for (int b = 0; b < B; ++b) {
    if (!(rh[b] > 0.0) || !std::isfinite(rh[b])) return bad("every ref[b] must be finite and > 0");
    if (!std::isfinite(rh[B + b])) return bad("every offset[b] must be finite");
  }
  const double g = std::exp(-1.0 / (fs * tc));
  launch_level_classes(x, ldx, lengths, offset, ref, B, longest, g, klass, ldk, sq, ws, (hipStream_t)stream);
  return finish();
}

int buddy_level_counts(const unsigned char* klass, long long ldk, const int* lengths, int B, int I, long long* counts, void* ws, long long ws_bytes,
                       void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_level_counts: ") + why); return BUDDY_ERR_ARG; };
  if (!klass || !lengths || !counts || !ws) return bad("null pointer");
  if (I < 0) return bad("I must be >= 0");
  int longest;
  if (int rc = check_rows(lengths, B, ldk, 0, stream, "buddy_level_counts", &longest)) return rc;
  if (ws_bytes < level_counts_ws_bytes(B, longest)) return bad("the workspace is smaller than buddy_level_counts_workspace(B, longest row)");
  launch_level_counts(klass, ldk, lengths, B, longest, I, counts, ws, (hipStream_t)stream);
  return finish();
}

// ---- spectral-envelope distortion of (estimate, clean) pairs (spectral.hip) ----
int buddy_frame_spectra(const float* x, const int* lens, int B, long long ld, int frame, int hop, float* S, long long ldf, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_frame_spectra: ") + why); return BUDDY_ERR_ARG; };
  if (!x || !lens || !S) return bad("null pointer");
  if (frame < 1 || frame > 512) return bad("frame must be in 1..512");
  if (hop < 1) return bad("hop must be >= 1");
  int longest;
  if (int rc = check_rows(lens, B, ld, 1, stream, "buddy_frame_spectra", &longest)) return rc;
  const long long maxF = frames_of(longest, frame, hop);
  if (ldf < at_least_one(maxF)) return bad("ldf is smaller than the frames of the longest row");
  launch_frame_spectra(x, lens, B, ld, maxF, frame, hop, S, ldf, (hipStream_t)stream);
  return finish();
}

long long buddy_cepstral_distance_workspace(int B, int max_frames) {
  if (B < 1 || max_frames < 0) return -1;
  return 8LL * B * at_least_one(max_frames) * 2 * spectral_cepstra();
}

int buddy_cepstral_distance(const float* X, const float* E, const int* frames, int B, long long ldf, const double* g, const double* d, double* out, int* flags,
                            void* ws, long long ws_bytes, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_cepstral_distance: ") + why); return BUDDY_ERR_ARG; };
  if (!X || !E || !frames || !g || !d || !out || !flags || !ws) return bad("null pointer");
  int longest;
  if (int rc = check_rows(frames, B, ldf, 0, stream, "buddy_cepstral_distance", &longest)) return rc;
  if (ws_bytes < buddy_cepstral_distance_workspace(B, longest)) return bad("the workspace is smaller than buddy_cepstral_distance_workspace(B, most frames)");
  launch_cepstral_distance(X, E, frames, B, ldf, longest, g, d, out, flags, (double*)ws, (hipStream_t)stream);
  return finish();
}

long long buddy_fwsegsnr_workspace(int B, int max_frames) {
  if (B < 1 || max_frames < 0) return -1;
  return 16LL * B * at_least_one(max_frames);
}

int buddy_fwsegsnr(const float* X, const float* E, const int* frames, int B, long long ldf, const double* g, const double* M, int J, double* out, int* counts,
                   int* flags, void* ws, long long ws_bytes, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_fwsegsnr: ") + why); return BUDDY_ERR_ARG; };
  if (!X || !E || !frames || !g || !M || !out || !counts || !flags || !ws) return bad("null pointer");
  if (J < 1 || J > 64) return bad("J must be in 1..64");
  int longest;
  if (int rc = check_rows(frames, B, ldf, 0, stream, "buddy_fwsegsnr", &longest)) return rc;
  if (ws_bytes < buddy_fwsegsnr_workspace(B, longest)) return bad("the workspace is smaller than buddy_fwsegsnr_workspace(B, most frames)");
  launch_fwsegsnr(X, E, frames, B, ldf, longest, g, M, J, out, counts, flags, (double*)ws, (hipStream_t)stream);
  return finish();
}

long long buddy_llr_workspace(int B, long long max_len, int frame, int hop) {
  if (B < 1 || max_len < 1 || max_len > (1LL << 30) || frame < 1 || frame > 512 || hop < 1) return -1;
  return 16LL * B * at_least_one(frames_of(max_len, frame, hop));
}

int buddy_llr(const float* e, const float* x, const int* lens, int B, long long ld, int frame, int hop, int order, double* out, int* counts, int* flags, void* ws,
              long long ws_bytes, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_llr: ") + why); return BUDDY_ERR_ARG; };
  if (!e || !x || !lens || !out || !counts || !flags || !ws) return bad("null pointer");
  if (frame < 1 || frame > 512) return bad("frame must be in 1..512");
  if (hop < 1) return bad("hop must be >= 1");
  if (order < 1 || order > spectral_max_order() || order >= frame) return bad("order must be in 1..16 and below the frame length");
  int longest;
  if (int rc = check_rows(lens, B, ld, 1, stream, "buddy_llr", &longest)) return rc;
  if (ws_bytes < buddy_llr_workspace(B, longest, frame, hop)) return bad("the workspace is smaller than buddy_llr_workspace(B, longest row, frame, hop)");
  launch_llr(e, x, lens, B, ld, frames_of(longest, frame, hop), frame, hop, order, out, counts, flags, (double*)ws, (hipStream_t)stream);
  return finish();
}

// ---- shoebox room impulse responses, image-source method (ism.hip) ----
int buddy_ism_half_width(void) { return ism_half_width(); }
int buddy_ism_tile(void) { return ism_tile(); }
int buddy_ism_list(void) { return ism_list(); }

int buddy_shoebox_rir(const double* rooms, int B, int fs, int N, int max_order, float* h, long long ldh, int* flags, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_shoebox_rir: ") + why); return BUDDY_ERR_ARG; };
  if (!rooms || !h || !flags) return bad("null pointer");
  if (B < 1 || B > 65535) return bad("B must be in 1..65535");
  if (fs < 1000 || fs > 1000000) return bad("fs must be in 1000..1000000");
  if (N < 1 || N > (1 << 20)) return bad("N must be in 1..2^20");
  if (ldh < N) return bad("ldh is smaller than N");
  if (max_order < -1) return bad("max_order must be >= -1 (-1: no cap)");
  launch_shoebox_rir(rooms, B, fs, N, max_order, h, ldh, flags, (hipStream_t)stream);
  return finish();
}

// ---- banded rooms: per-band responses in double, then the FIR-bank combination (ism.hip) ----
int buddy_ism_max_bands(void) { return ism_max_bands(); }
int buddy_ism_band_list(void) { return ism_band_list(); }
int buddy_band_combine_tile(void) { return band_combine_tile(); }

int buddy_shoebox_bands(const double* rooms, const double* beta, const double* air, int B, int nb, int fs, int N, int max_order, double* u, long long ldu,
                        int* flags, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_shoebox_bands: ") + why); return BUDDY_ERR_ARG; };
  if (!rooms || !beta || !u || !flags) return bad("null pointer");
  if (B < 1 || B > 65535) return bad("B must be in 1..65535");
  if (nb < 1 || nb > ism_max_bands()) return bad("nb must be in 1..buddy_ism_max_bands()");
  if (fs < 1000 || fs > 1000000) return bad("fs must be in 1000..1000000");
  if (N < 1 || N > (1 << 20)) return bad("N must be in 1..2^20");
  if (ldu < N) return bad("ldu is smaller than N");
  if (max_order < -1) return bad("max_order must be >= -1 (-1: no cap)");
  launch_shoebox_bands(rooms, beta, air, B, nb, fs, N, max_order, u, ldu, flags, (hipStream_t)stream);
  return finish();
}

int buddy_band_combine(const double* u, int B, int nb, long long ldu, int N, const double* bank, int Nh, float* h, long long ldh, void* stream) {
  auto bad = [](const char* why) { set_error(std::string("buddy_band_combine: ") + why); return BUDDY_ERR_ARG; };
  if (!u || !bank || !h) return bad("null pointer");
  if (B < 1 || B > 65535) return bad("B must be in 1..65535");
  if (nb < 1 || nb > ism_max_bands()) return bad("nb must be in 1..buddy_ism_max_bands()");
  if (N < 1 || N > (1 << 20)) return bad("N must be in 1..2^20");
  if (ldu < N) return bad("ldu is smaller than N");
  if (ldh < N) return bad("ldh is smaller than N");
  if (Nh < 1 || Nh > 65537 || Nh % 2 == 0) return bad("Nh must be odd and in 1..65537");
  launch_band_combine(u, B, nb, ldu, N, bank, Nh, h, ldh, (hipStream_t)stream);
  return finish();
}

// ---- multichannel WPE ----
static int wpe_mc_args(int D, int taps, int delay, int iterations) {
  if (!wpe_mc_supported(D, taps) || delay < 0 || iterations < 0) {
    set_error("bad multichannel wpe arguments (1 <= D <= 8, taps >= 1, D * taps <= 96, delay >= 0, iterations >= 0)"); return BUDDY_ERR_ARG;
  }
  return BUDDY_OK;
}

int buddy_wpe_mc(const double* Y, double* X, double* scratch, int rows, int D, int T, int taps, int delay, int iterations, void* stream) {
  if (!Y || !X || !scratch || rows < 1 || T < 1) { set_error("bad multichannel wpe arguments (null pointer, rows < 1 or T < 1)"); return BUDDY_ERR_ARG; }
  if (wpe_mc_args(D, taps, delay, iterations)) return BUDDY_ERR_ARG;
  if (launch_wpe_mc(Y, X, scratch, rows, D, T, taps, delay, iterations, (hipStream_t)stream)) { set_error("multichannel wpe: LDS request refused"); return BUDDY_ERR_HIP; }
  return finish();
}

long long buddy_wpe_mc_workspace_bytes(int B, int D, int L) { return (B < 1 || D < 1 || L < 1) ? 0 : (long long)wpe_mc_workspace_bytes(B, D, L); }

int buddy_wpe_mc_dereverb(const float* y, float* out, void* workspace, int B, int D, int L, int taps, int delay, int iterations, void* stream) {
  if (!y || !out || !workspace || B < 1 || L < 1) { set_error("bad multichannel wpe arguments (null pointer, B < 1 or L < 1)"); return BUDDY_ERR_ARG; }
  if (wpe_mc_args(D, taps, delay, iterations)) return BUDDY_ERR_ARG;
  if (launch_wpe_mc_dereverb(y, out, workspace, B, D, L, taps, delay, iterations, (hipStream_t)stream)) { set_error("multichannel wpe: LDS request refused"); return BUDDY_ERR_HIP; }
  return finish();
}

// ---- wMPDR beamformer after multichannel WPE ----
static int mpdr_args(int D, int reference, int iterations, double loading) {
  if (!mpdr_supported(D) || reference < 0 || reference >= D || iterations < 1 || !(loading >= 0.0) || !std::isfinite(loading)) {
    set_error("bad beamformer arguments (1 <= D <= 8, 0 <= reference < D, iterations >= 1, loading >= 0 and finite)"); return BUDDY_ERR_ARG;
  }
  return BUDDY_OK;
}

int buddy_mpdr(const double* X, double* Z, double* scratch, int rows, int D, int T, int reference, int iterations, double loading, void* stream) {
  if (!X || !Z || !scratch || rows < 1 || T < 1) { set_error("bad beamformer arguments (null pointer, rows < 1 or T < 1)"); return BUDDY_ERR_ARG; }
  if (mpdr_args(D, reference, iterations, loading)) return BUDDY_ERR_ARG;
  launch_mpdr(X, Z, scratch, rows, D, T, reference, iterations, loading, (hipStream_t)stream);
  return finish();
}

long long buddy_wpe_mc_mpdr_workspace_bytes(int B, int D, int L) { return buddy_wpe_mc_workspace_bytes(B, D, L); }

int buddy_wpe_mc_mpdr_dereverb(const float* y, float* out, void* workspace, int B, int D, int L, int taps, int delay, int wpe_iterations,
                               int reference, int bf_iterations, double loading, void* stream) {
  if (!y || !out || !workspace || B < 1 || L < 1) { set_error("bad multichannel wpe arguments (null pointer, B < 1 or L < 1)"); return BUDDY_ERR_ARG; }
  if (wpe_mc_args(D, taps, delay, wpe_iterations) || mpdr_args(D, reference, bf_iterations, loading)) return BUDDY_ERR_ARG;
  if (launch_wpe_mc_mpdr_dereverb(y, out, workspace, B, D, L, taps, delay, wpe_iterations, reference, bf_iterations, loading, (hipStream_t)stream)) {
    set_error("multichannel wpe: LDS request refused"); return BUDDY_ERR_HIP;
  }
  return finish();
}

// ---- WPE warm start ----
int buddy_wpe(const double* Y, double* X, double* scratch, int rows, int T, int taps, int delay, int iterations, void* stream) {
  if (!Y || !X || !scratch || rows < 1 || T < 1 || taps < 1 || taps > 56 || delay < 0 || iterations < 0) { set_error("bad wpe arguments (taps <= 56)"); return BUDDY_ERR_ARG; }
  launch_wpe(Y, X, scratch, rows, T, taps, delay, iterations, (hipStream_t)stream);
  return finish();
}

long long buddy_wpe_workspace_bytes(int B, int L) { return (B < 1 || L < 1) ? 0 : (long long)wpe_workspace_bytes(B, L); }

int buddy_wpe_dereverb(const float* y, float* out, void* workspace, int B, int L, int taps, int delay, int iterations, void* stream) {
  if (!y || !out || !workspace || B < 1 || L < 1 || taps < 1 || taps > 56 || delay < 0 || iterations < 0) { set_error("bad wpe arguments (taps <= 56)"); return BUDDY_ERR_ARG; }
  launch_wpe_dereverb(y, out, workspace, B, L, taps, delay, iterations, (hipStream_t)stream);
  return finish();
}

// ---- blind operator ----
int buddy_blindop_create(int U, int L, int Nf, int E, int num_knots, const float* knots, int sample_rate, float comp, float min_decay,
                         float max_decay, float w_lo, float w_hi, int clamp_decay, int long_second, void** handle) {
  // any L >= 1: every kernel clamps its frame / sample index into the T = 1 + (L + 512) / 128 >= 5 frames that exist, and the work buffers are sized by
  // max(T, Td) / max(L, Lr) (tests/test_hip_operator_shapes.py runs L = 100 against float64)
  if (!knots || !handle || U < 1 || L < 1 || num_knots > 64) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  BlindOpCfg c; std::memset(&c, 0, sizeof(c));
  c.n_fft = 1024; c.win = 512; c.hop = 128; c.Nf = Nf; c.E = E; c.num_knots = num_knots; c.sample_rate = sample_rate; c.comp = comp;
  for (int i = 0; i < num_knots; ++i) c.knots[i] = knots[i];
  c.min_decay = min_decay; c.max_decay = max_decay; c.w_lo = w_lo; c.w_hi = w_hi; c.clamp_decay = clamp_decay; c.long2nd = long_second;
  BlindOp* o = nullptr;
  int rc = blindop_create(c, U, L, &o);
  if (rc) return rc;
  *handle = o;
  return BUDDY_OK;
}
int buddy_blindop_destroy(void* h) { blindop_destroy((BlindOp*)h); return BUDDY_OK; }
#define BOP_CHECK(h) if (!(h)) { set_error("null handle"); return BUDDY_ERR_ARG; }
int buddy_blindop_set_params(void* h, const float* decay, const float* weights, const float* phases, int reset_adam, void* stream) {
  BOP_CHECK(h); return blindop_set_params((BlindOp*)h, decay, weights, phases, reset_adam, (hipStream_t)stream);
}
int buddy_blindop_get_params(void* h, float* decay, float* weights, float* phases, void* stream) {
  BOP_CHECK(h); return blindop_get_params((BlindOp*)h, decay, weights, phases, (hipStream_t)stream);
}
int buddy_blindop_set_groups(void* h, const int* group_of_row, void* stream) { BOP_CHECK(h); return blindop_set_groups((BlindOp*)h, group_of_row, (hipStream_t)stream); }
int buddy_blindop_update_H(void* h, const float* noise, void* stream) { BOP_CHECK(h); return blindop_update_H((BlindOp*)h, noise, (hipStream_t)stream); }
int buddy_blindop_get_H(void* h, float* out, void* stream) { BOP_CHECK(h); if (!out) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_get_H((BlindOp*)h, out, (hipStream_t)stream); }
int buddy_blindop_set_y(void* h, const float* y, void* stream) { BOP_CHECK(h); if (!y) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_set_y((BlindOp*)h, y, (hipStream_t)stream); }
int buddy_blindop_degrade(void* h, const float* x, float* y, void* stream) { BOP_CHECK(h); if (!x || !y) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_degrade((BlindOp*)h, x, y, (hipStream_t)stream); }
int buddy_blindop_time_rir(void* h, float* out, void* stream) { BOP_CHECK(h); if (!out) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_time_rir((BlindOp*)h, out, (hipStream_t)stream); }
int buddy_blindop_design_filter(void* h, float* A, void* stream) { BOP_CHECK(h); if (!A) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_design_filter((BlindOp*)h, A, (hipStream_t)stream); }
int buddy_blindop_apply_stft(void* h, const float* x, float* X, void* stream) { BOP_CHECK(h); if (!x || !X) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_apply_stft((BlindOp*)h, x, X, (hipStream_t)stream); }
int buddy_blindop_degrade_vjp(void* h, const float* x, const float* g_y, float* g_x, float* g_H, void* stream) {
  BOP_CHECK(h);
  if (!g_y || (!g_x && !g_H) || (g_H && !x)) { set_error("degrade_vjp: g_y and at least one output; x is needed for g_H"); return BUDDY_ERR_ARG; }
  return blindop_degrade_vjp((BlindOp*)h, x, g_y, g_x, g_H, (hipStream_t)stream);
}
int buddy_blindop_time_rir_vjp(void* h, const float* g_rir, float* g_H, void* stream) { BOP_CHECK(h); if (!g_rir || !g_H) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_time_rir_vjp((BlindOp*)h, g_rir, g_H, (hipStream_t)stream); }
int buddy_blindop_update_H_vjp(void* h, const float* g_H, float* g_decay, float* g_weights, float* g_phases, void* stream) {
  BOP_CHECK(h); if (!g_H) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_update_H_vjp((BlindOp*)h, g_H, g_decay, g_weights, g_phases, (hipStream_t)stream);
}
int buddy_blindop_stft(void* h, const float* x, int len, float* X, void* stream) { BOP_CHECK(h); if (!x || !X) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_stft_len((BlindOp*)h, x, len, X, (hipStream_t)stream); }
int buddy_blindop_stft_adjoint(void* h, const float* G, int len, float* g_x, void* stream) { BOP_CHECK(h); if (!G || !g_x) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_stft_len_adj((BlindOp*)h, G, len, g_x, (hipStream_t)stream); }
int buddy_blindop_stft_loss(void* h, const float* a, const float* b, int len, float weight, float* loss, float* g_a, float* g_b, void* stream) {
  BOP_CHECK(h); if (!a || !b || !loss) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_stft_loss((BlindOp*)h, a, b, len, weight, loss, g_a, g_b, (hipStream_t)stream);
}
int buddy_blindop_set_compression(void* h, float comp) { BOP_CHECK(h); return blindop_set_compression((BlindOp*)h, comp); }
int buddy_blindop_set_loss_norm(void* h, int mode) { BOP_CHECK(h); return blindop_set_loss_norm((BlindOp*)h, mode); }
int buddy_blindop_set_loss(void* h, int slot, int kind, int freq_weighting, float compression) {
  BOP_CHECK(h); return blindop_set_loss((BlindOp*)h, slot, kind, freq_weighting, compression);
}
int buddy_blindop_set_freq_weights(void* h, int freq_weighting, const float* w) { BOP_CHECK(h); return blindop_set_freq_weights((BlindOp*)h, freq_weighting, w); }
int buddy_blindop_lengths(void* h, int* L, int* Lr, int* T, int* Td) { BOP_CHECK(h); return blindop_lengths((BlindOp*)h, L, Lr, T, Td); }
int buddy_blindop_minphase(void* h, const float* hin, float* out, void* stream) { BOP_CHECK(h); if (!hin || !out) { set_error("null"); return BUDDY_ERR_ARG; } return blindop_minphase((BlindOp*)h, hin, out, (hipStream_t)stream); }
int buddy_blindop_project(void* h, void* stream) { BOP_CHECK(h); return blindop_project((BlindOp*)h, (hipStream_t)stream); }
int buddy_blindop_get_adam(void* h, float* m_decay, float* v_decay, float* m_weights, float* v_weights, float* m_phases, float* v_phases, int* step,
                           void* stream) {
  BOP_CHECK(h); return blindop_get_adam((BlindOp*)h, m_decay, v_decay, m_weights, v_weights, m_phases, v_phases, step, (hipStream_t)stream);
}
int buddy_blindop_rec_loss_grad(void* h, const float* x_den, float weight, float* loss, float* g_x, void* stream) {
  BOP_CHECK(h); if (!x_den || !loss) { set_error("null"); return BUDDY_ERR_ARG; }
  return blindop_rec_loss_grad((BlindOp*)h, x_den, weight, loss, g_x, (hipStream_t)stream);
}
int buddy_blindop_fir_loss_grad(void* h, const float* x_den, const float* rir, long long rir_stride, int M, float weight, float* loss, float* g_x,
                                void* stream) {
  BOP_CHECK(h); if (!x_den || !rir || !loss || M < 1) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  return blindop_fir_loss_grad((BlindOp*)h, x_den, rir, rir_stride, M, weight, loss, g_x, (hipStream_t)stream);
}
int buddy_blindop_param_grads(void* h, const float* x_den, const float* noise, float t_op, float w_rec, float w_reg, float* g_decay, float* g_weights,
                              float* g_phases, float* losses, void* stream) {
  BOP_CHECK(h); if (!x_den) { set_error("null"); return BUDDY_ERR_ARG; }
  return blindop_param_grads((BlindOp*)h, x_den, noise, t_op, w_rec, w_reg, g_decay, g_weights, g_phases, losses, (hipStream_t)stream);
}
int buddy_blindop_optimize(void* h, const float* x_den, const float* noise, float t_op, int n_iters, float w_rec, float w_reg, float lr, float beta1,
                           float beta2, float weight_decay, void* stream) {
  BOP_CHECK(h); if (!x_den || n_iters < 0) { set_error("bad arguments"); return BUDDY_ERR_ARG; }
  return blindop_optimize((BlindOp*)h, x_den, noise, t_op, n_iters, w_rec, w_reg, lr, beta1, beta2, weight_decay, (hipStream_t)stream);
}

// ---- parameter-gradient kernels (wgrad.hip) on their own: thin, argument-checked entries for the unit tests; net.hip calls the launchers directly
long long buddy_weight_grad_workspace(long long M, int N, int K) { return (M < 1 || N < 1 || K < 1) ? 0 : wgrad_ws_floats(M, N, K); }
int buddy_weight_grad_chunks(long long M, int N, int K) { return (M < 1 || N < 1 || K < 1) ? 0 : wgrad_chunks(M, N, K); }
static bool src2_ok(const float* x0, const float* x1, int C0, int ld0, int ld1, int C) {
  if (!x0 || C < 1) return false;
  if (!x1) return ld0 >= C;
  return C0 > 0 && C0 < C && ld0 >= C0 && ld1 >= C - C0;
}
static Src2 mk_src2(const float* x0, const float* x1, int C0, int ld0, int ld1, int C) {
  Src2 s; s.p0 = x0; s.p1 = x1; s.C0 = x1 ? C0 : C; s.ld0 = ld0; s.ld1 = x1 ? ld1 : 0;
  return s;
}
int buddy_weight_grad(const float* dy, long long T, long long sb, long long sm, long long sn, const float* x0, const float* x1, int C0, int ld0, int ld1,
                      int H, int W, int Cin, int taps, int rs, const float* stats, const float* gamma, const float* beta, int G, int silu, int B, int N,
                      int layout, float alpha, float* ws, float* out, void* stream) {
  if (!dy || !ws || !out || B < 1 || H < 1 || W < 1 || N < 1 || T < 1 || !src2_ok(x0, x1, C0, ld0, ld1, Cin)) {
    set_error("bad weight-gradient arguments (null pointer, empty shape, or a two-source split outside (0, Cin) / a row stride below its channel count)");
    return BUDDY_ERR_ARG;
  }
  const long long M = (long long)B * H * W;
  if (M % T != 0) { set_error("weight gradient: the dY view's rows per utterance T must divide B * H * W"); return BUDDY_ERR_ARG; }
  if (taps != 1 && taps != 9) { set_error("weight gradient: taps must be 1 or 9"); return BUDDY_ERR_ARG; }
  if (rs < 0 || rs > 2 || (rs == 2 && ((H | W) & 1))) { set_error("weight gradient: rs must be 0, 1 (box, source at 2H x 2W) or 2 (nearest, source at H/2 x W/2: even H, W)"); return BUDDY_ERR_ARG; }
  if (layout < 0 || layout > 2 || (layout == 1 && taps != 9)) { set_error("weight gradient: layout must be 0 [N][K], 1 (torch OIHW, taps = 9 only) or 2 [K][N]"); return BUDDY_ERR_ARG; }
  if (stats && (!gamma || !beta || G < 1 || Cin % G != 0)) { set_error("weight gradient: GroupNorm needs gamma, beta and a group count that divides Cin"); return BUDDY_ERR_ARG; }
  WgY y; y.p = dy; y.T = T; y.sb = sb; y.sm = sm; y.sn = sn;
  WgA a; a.x = mk_src2(x0, x1, C0, ld0, ld1, Cin); a.H = H; a.W = W; a.Cin = Cin; a.taps = taps; a.rs = rs;
  a.stats = stats; a.gamma = stats ? gamma : nullptr; a.beta = stats ? beta : nullptr; a.G = stats ? G : 1; a.silu = silu ? 1 : 0;
  launch_wgrad(y, a, M, N, layout, alpha, ws, out, (hipStream_t)stream);
  return finish();
}

long long buddy_colsum_workspace(int B, long long T, int N) { return (B < 1 || T < 1 || N < 1) ? 0 : colsum_ws_floats(B, T, N); }
int buddy_colsum(const float* dy, long long T, long long sb, long long sm, long long sn, int B, int N, float alpha, float* ws, float* bc, int ld_bc,
                 float* out, float* out2, void* stream) {
  if (!dy || !ws || B < 1 || T < 1 || N < 1 || (!bc && !out && !out2) || (bc && ld_bc < N)) {
    set_error("bad column-sum arguments (null pointer, empty shape, no output, or ld_bc < N)"); return BUDDY_ERR_ARG;
  }
  WgY y; y.p = dy; y.T = T; y.sb = sb; y.sm = sm; y.sn = sn;
  launch_colsum(y, B, N, alpha, ws, bc, ld_bc, out, out2, (hipStream_t)stream);
  return finish();
}
int buddy_basis_bias(const float* x, int K, int B, long long T, const double* bsum, float* ws, float* out, void* stream) {
  if (!x || !bsum || !ws || !out || K < 1 || B < 1 || T < 1) { set_error("bad basis-bias arguments (null pointer or empty shape)"); return BUDDY_ERR_ARG; }
  launch_basis_bias(x, K, B, T, bsum, ws, out, (hipStream_t)stream);
  return finish();
}

long long buddy_gn_param_grads_workspace(int B, int H, int W, int C) { return (B < 1 || H < 1 || W < 1 || C < 1) ? 0 : gn_pgrad_ws_floats(B, H, W, C); }
int buddy_gn_param_grads(const float* x0, const float* x1, int C0, int ld0, int ld1, const float* stats, const float* gamma, const float* beta, int G,
                         int silu, const float* da, int da_mode, int B, int H, int W, int C, float* ws, float* dgamma, float* dbeta, void* stream) {
  if (!stats || !gamma || !beta || !da || !ws || !dgamma || !dbeta || B < 1 || H < 1 || W < 1 || !src2_ok(x0, x1, C0, ld0, ld1, C)) {
    set_error("bad GroupNorm parameter-gradient arguments (null pointer, empty shape, or a two-source split outside (0, C) / a row stride below its channel count)");
    return BUDDY_ERR_ARG;
  }
  if (G < 1 || C % G != 0) { set_error("GroupNorm parameter gradients: the group count must divide C"); return BUDDY_ERR_ARG; }
  if (da_mode < 0 || da_mode > 2 || (da_mode == 1 && ((H | W) & 1))) {
    set_error("GroupNorm parameter gradients: da_mode must be 0, 1 (da at H/2 x W/2: even H, W) or 2 (da at 2H x 2W)"); return BUDDY_ERR_ARG;
  }
  launch_gn_pgrad(mk_src2(x0, x1, C0, ld0, ld1, C), stats, gamma, beta, G, silu ? 1 : 0, da, da_mode, B, H, W, C, ws, dgamma, dbeta, (hipStream_t)stream);
  return finish();
}

int buddy_linear_bwd_w(const float* dy, int ld_dy, const float* x, int silu_in, int B, int N, int K, float* gw, float* gb, float* gb2, void* stream) {
  if (!dy || !x || !gw || B < 1 || N < 1 || K < 1 || ld_dy < N) { set_error("bad linear-backward arguments (null pointer, empty shape, or ld_dy < N)"); return BUDDY_ERR_ARG; }
  launch_linear_bwd_w(dy, ld_dy, x, silu_in ? 1 : 0, B, N, K, gw, gb, gb2, (hipStream_t)stream);
  return finish();
}
int buddy_linear_bwd_x(const float* dy, const float* Wm, const float* x, int silu_in, int B, int N, int K, float* dx, void* stream) {
  if (!dy || !Wm || !dx || (silu_in && !x) || B < 1 || N < 1 || K < 1) { set_error("bad linear-backward arguments (null pointer or empty shape)"); return BUDDY_ERR_ARG; }
  launch_linear_bwd_x(dy, Wm, x, silu_in ? 1 : 0, B, N, K, dx, (hipStream_t)stream);
  return finish();
}

// ---- the small kernels of the network (ops.hip), one thin entry per launcher: argument checks, the launch, finish()
#define SMALL_REFUSE(cond, msg) do { if (cond) { set_error(msg); return BUDDY_ERR_ARG; } } while (0)

int buddy_conv_c2in(const float* x, const float* w, const float* bias, const float* add, int add_ld, float* y, int ldY, int B, int H, int W, int Cout,
                    int taps, int accumulate, void* stream) {
  SMALL_REFUSE(!x || !w || !y || B < 1 || H < 1 || W < 1 || Cout < 1, "conv_c2in: null pointer or empty shape");
  SMALL_REFUSE(taps != 1 && taps != 9, "conv_c2in: taps must be 1 or 9");
  SMALL_REFUSE(Cout % 4 != 0, "conv_c2in: Cout must be a multiple of 4 (a thread writes one channel quad)");
  SMALL_REFUSE(ldY < Cout || ldY % 4 != 0, "conv_c2in: ldY must be a multiple of 4 floats, at least Cout");
  SMALL_REFUSE(add && (add_ld < Cout || add_ld % 4 != 0), "conv_c2in: add_ld must be a multiple of 4 floats, at least Cout");
  launch_conv_c2in(x, w, bias, add, add_ld, y, ldY, B, H, W, Cout, taps, accumulate ? 1 : 0, (hipStream_t)stream);
  return finish();
}

int buddy_conv_c2out(const float* x, int ldX, const float* w, const float* bias, const float* up_add, float* y, int B, int H, int W, int Cin, int taps,
                     int accumulate, int form, void* stream) {
  SMALL_REFUSE(!x || !w || !y || B < 1 || H < 1 || W < 1 || Cin < 1, "conv_c2out: null pointer or empty shape");
  SMALL_REFUSE(taps != 1 && taps != 9, "conv_c2out: taps must be 1 or 9");
  SMALL_REFUSE(Cin % 4 != 0, "conv_c2out: Cin must be a multiple of 4 (a lane reads one channel quad)");
  SMALL_REFUSE(ldX < Cin || ldX % 4 != 0, "conv_c2out: ldX must be a multiple of 4 floats, at least Cin");
  SMALL_REFUSE(up_add && ((H | W) & 1), "conv_c2out: up_add (at H/2 x W/2) needs even H and W");
  SMALL_REFUSE(form < -1 || form > 2, "conv_c2out: form must be -1 (process default), 0 (lane group), 1 (tiled) or 2 (strip)");
  SMALL_REFUSE(form > 0 && (taps != 9 || Cin % 32 != 0), "conv_c2out: the tiled and strip forms compute 9 taps over Cin % 32 == 0 only");
  Options o = default_options();
  if (form >= 0) o.c2out_tiled = form;
  OptScope scope(&o);
  launch_conv_c2out(x, ldX, w, bias, up_add, y, B, H, W, Cin, taps, accumulate ? 1 : 0, (hipStream_t)stream);
  return finish();
}

int buddy_reflect_pad(const float* x, float* xp, int B, int L, int pad, int Lp, float scale, const float* scale_b, void* stream) {
  SMALL_REFUSE(!x || !xp || B < 1 || L < 1 || pad < 0, "reflect_pad: null pointer or empty shape");
  SMALL_REFUSE(pad >= L, "reflect_pad: pad must be below L (one reflection per side)");
  SMALL_REFUSE(Lp < (long long)L + 2LL * pad, "reflect_pad: Lp must be at least L + 2 pad");
  launch_reflect_pad(x, xp, B, L, pad, Lp, scale, scale_b, (hipStream_t)stream);
  return finish();
}

static bool stft_geo_ok(int n_fft, int hop, int frames, int ldF, int B, int L, int pad) {
  return n_fft >= 1 && hop >= 1 && frames >= 1 && ldF >= n_fft && B >= 1 && L >= 1 && pad >= 0;
}

int buddy_ola(const float* frames, int ldF, int Tp, int n_fft, int hop, const float* inv_env, float* y, int B, int L, int pad, const float* xin,
              const float* cskip_b, const float* cout_b, void* stream) {
  SMALL_REFUSE(!frames || !inv_env || !y || !stft_geo_ok(n_fft, hop, Tp, ldF, B, L, pad), "ola: null pointer, empty shape or ldF < n_fft");
  SMALL_REFUSE(xin && (!cskip_b || !cout_b), "ola: xin needs cskip_b and cout_b");
  SMALL_REFUSE((long long)L + pad > (long long)n_fft + (long long)hop * (Tp - 1), "ola: L + pad exceeds the envelope's n_fft + hop (Tp - 1) samples");
  launch_ola(frames, ldF, Tp, n_fft, hop, inv_env, y, B, L, pad, xin, cskip_b, cout_b, (hipStream_t)stream);
  return finish();
}

int buddy_ola_adj(const float* g, int B, int L, int pad, int Tp, int n_fft, int hop, const float* inv_env, const float* cout_b, float* frames, int ldF,
                  void* stream) {
  SMALL_REFUSE(!g || !inv_env || !frames || !stft_geo_ok(n_fft, hop, Tp, ldF, B, L, pad), "ola_adj: null pointer, empty shape or ldF < n_fft");
  launch_ola_adj(g, B, L, pad, Tp, n_fft, hop, inv_env, cout_b, frames, ldF, (hipStream_t)stream);
  return finish();
}

int buddy_unpad_adj(const float* dframes, int ldF, int T, int n_fft, int hop, int B, int L, int pad, float scale, const float* scale_b,
                    const float* g_out, const float* cskip_b, float* dx, void* stream) {
  SMALL_REFUSE(!dframes || !dx || !stft_geo_ok(n_fft, hop, T, ldF, B, L, pad), "unpad_adj: null pointer, empty shape or ldF < n_fft");
  SMALL_REFUSE(pad >= L, "unpad_adj: pad must be below L (one reflection per side)");
  SMALL_REFUSE(g_out && !cskip_b, "unpad_adj: g_out needs cskip_b");
  launch_unpad_adj(dframes, ldF, T, n_fft, hop, B, L, pad, scale, scale_b, g_out, cskip_b, dx, (hipStream_t)stream);
  return finish();
}

int buddy_pool2(const float* src, float* dst, int B, int H, int W, int C, float scale, int accumulate, void* stream) {
  SMALL_REFUSE(!src || !dst || B < 1 || H < 2 || W < 2 || C < 1, "pool2: null pointer or empty shape");
  SMALL_REFUSE((H | W) & 1, "pool2: H and W must be even");
  SMALL_REFUSE(C != 2 && C % 4 != 0, "pool2: C must be 2 or a multiple of 4");
  launch_pool2(src, dst, B, H, W, C, scale, accumulate ? 1 : 0, (hipStream_t)stream);
  return finish();
}

int buddy_up2_acc(const float* src, float* dst, int B, int Hs, int Ws, int C, float scale, int accumulate, void* stream) {
  SMALL_REFUSE(!src || !dst || B < 1 || Hs < 1 || Ws < 1 || C < 1, "up2_acc: null pointer or empty shape");
  SMALL_REFUSE(C % 2 != 0, "up2_acc: C must be even (float2 granularity)");
  launch_up2_acc(src, dst, B, Hs, Ws, C, scale, accumulate ? 1 : 0, (hipStream_t)stream);
  return finish();
}

int buddy_fourier(const float* cnoise, const float* Wf, float* out, int B, int nf, void* stream) {
  SMALL_REFUSE(!cnoise || !Wf || !out || B < 1 || nf < 1, "fourier: null pointer or empty shape");
  launch_fourier(cnoise, Wf, out, B, nf, (hipStream_t)stream);
  return finish();
}

int buddy_linear(const float* x, const float* Wm, const float* bias, float* y, int B, int K, int N, int silu_in, void* stream) {
  SMALL_REFUSE(!x || !Wm || !y || B < 1 || K < 1 || N < 1, "linear: null pointer or empty shape");
  launch_linear(x, Wm, bias, y, B, K, N, silu_in ? 1 : 0, (hipStream_t)stream);
  return finish();
}

int buddy_softmax_rows(float* S, int rows, int cols, void* stream) {
  SMALL_REFUSE(!S || rows < 1 || cols < 1, "softmax_rows: null pointer or empty shape");
  launch_softmax_rows(S, rows, cols, (hipStream_t)stream);
  return finish();
}

int buddy_softmax_bwd_rows(const float* P, float* dP, int rows, int cols, void* stream) {
  SMALL_REFUSE(!P || !dP || rows < 1 || cols < 1, "softmax_bwd_rows: null pointer or empty shape");
  launch_softmax_bwd_rows(P, dP, rows, cols, (hipStream_t)stream);
  return finish();
}

int buddy_transpose_sq(const float* src, float* dst, int batch, int n, void* stream) {
  SMALL_REFUSE(!src || !dst || batch < 1 || n < 1, "transpose_sq: null pointer or empty shape");
  SMALL_REFUSE(n % 32 != 0, "transpose_sq: n must be a multiple of 32 (whole 32 x 32 tiles)");
  SMALL_REFUSE(src == dst, "transpose_sq: not in place");
  SMALL_REFUSE(batch > 65535 || n / 32 > 65535, "transpose_sq: more than 65535 tiles per side or batch entries");
  launch_transpose_sq(src, dst, batch, n, (hipStream_t)stream);
  return finish();
}

int buddy_mix2(const float* x, const float* w, const float* b, float* y, long long npix, int transpose, int accumulate, void* stream) {
  SMALL_REFUSE(!x || !w || !y || npix < 1, "mix2: null pointer or empty shape");
  launch_mix2(x, w, b, y, npix, transpose ? 1 : 0, accumulate ? 1 : 0, (hipStream_t)stream);
  return finish();
}

int buddy_axpy(float* dst, const float* src, float alpha, long long n, int accumulate, void* stream) {
  SMALL_REFUSE(!dst || !src || n < 1, "axpy: null pointer or empty shape");
  SMALL_REFUSE(n % 4 != 0, "axpy: n must be a multiple of 4 (float4 granularity; a tail would be dropped)");
  launch_axpy(dst, src, alpha, n, accumulate ? 1 : 0, (hipStream_t)stream);
  return finish();
}
#undef SMALL_REFUSE

}  // extern "C"
