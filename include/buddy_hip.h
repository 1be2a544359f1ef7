/* C-ABI of libbuddy_hip.so -- the MI355X (gfx950) drop-in boundary for the reverse-diffusion dereverberation
 * sampler path of sp-uhh/buddy.
 *
 * The reference has no FFI boundary on this path: its plug points are Python classes resolved from Hydra
 * `_target_` strings.  This library sits *under* those classes: the Python side
 * (buddy_amd/) keeps the reference's class/constructor/method surface and calls these entry points with raw
 * device pointers (plain pointers and sizes, no torch types).  Each entry point names the reference interface it
 * replaces.  All functions return 0 on success, non-zero on error (text via buddy_last_error()); `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  All tensors are fp32, device-resident, contiguous.
 */
#ifndef BUDDY_HIP_H
#define BUDDY_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

const char* buddy_last_error(void);
int buddy_version(void);

/* ---- score network: replaces networks/ncsnpp.py NCSNppTime (ctor :458-464, forward :498-506) and the torch.autograd
 * backward through it that EulerHeunSamplerDPS.get_likelihood_score needs (testing/EulerHeunSamplerDPS.py:61-69). ---- */

/* number of fp32 parameters for an architecture = size of the flat blob `buddy_ncsnpp_create` expects: every tensor of
 * NCSNppTime.state_dict() (names all_modules.N.*, output_layer.*; reference networks/ncsnpp.py:157-274) concatenated in
 * module-construction order (GroupNorm_0.{weight,bias}, Conv_0.{weight,bias}, Dense_0.{weight,bias}, GroupNorm_1.*,
 * Conv_1.*, [Conv_2.*]) -- buddy_amd/synth.py:module_specs is the Python mirror of that order. */
int buddy_ncsnpp_param_count(int nf, const int* ch_mult, int n_levels, int num_res_blocks, long long* count);

/* build a network handle from a HOST blob: the parameters are uploaded once; the 3x3 convolutions' operand forms (Winograd-domain weights,
 * bf16x3 stage images) are derived ON THE DEVICE, per layer, for the one kernel variant the first forward / VJP of a workload selects.
 * n_fft / hop: conf/network/ncsnpp.yaml:2-5 (510 / 128).  (The reference builds its module with `instantiate(args.network)` and loads a
 * state dict, test.py:60-75; this is the library side of NCSNppTime.load_state_dict + .to(device).) */
int buddy_ncsnpp_create(const float* host_params, long long n_params, int nf, const int* ch_mult, int n_levels,
                        int num_res_blocks, int n_fft, int hop, void** handle);
/* The same two entries for a network with attention sites (reference networks/ncsnpp.py:195-196, 232-233): bit l of attn_mask = an AttnBlock after
 * every down ResnetBlock of level l and one after the up ResnetBlocks of level l (NCSNppTime derives it from attn_resolutions:
 * image_size // 2^l in attn_resolutions).  Its parameters (GroupNorm_0.*, NIN_0..3.*) take their places in the blob in module order and shift the
 * all_modules.N indices after them.  attn_mask = 0 is buddy_ncsnpp_param_count / buddy_ncsnpp_create.  A site runs the attention core of the handle
 * (buddy_ncsnpp_set_attention); a C = 32 site has no 16-bit kernel and runs the fp32 flash kernels in the bf16 / f16 modes too.  A forward whose
 * site has a width without a flash kernel (C not in {32, 64, 128, 256}) and more than 4096 tokens fails with BUDDY_ERR_ARG. */
int buddy_ncsnpp_param_count_attn(int nf, const int* ch_mult, int n_levels, int num_res_blocks, int attn_mask, long long* count);
int buddy_ncsnpp_create_attn(const float* host_params, long long n_params, int nf, const int* ch_mult, int n_levels,
                             int num_res_blocks, int n_fft, int hop, int attn_mask, void** handle);
int buddy_ncsnpp_destroy(void* handle);
/* a second handle on the SAME prepared weights (reference-counted, read-only): own activation arena, VJP tape and attention / gemm / fir
 * settings (copied from `handle`).  For concurrent sub-batches on several streams; no reference counterpart (testing/tester.py:132-153 samples
 * one utterance at a time on one module). */
int buddy_ncsnpp_replica(void* handle, void** replica);
/* device bytes held by the (shared) weight store of a handle: raw parameters, bf16x3 images of the 1x1 / NIN matrices, lazily prepared 3x3
 * operand forms (and their count). */
int buddy_ncsnpp_weight_bytes(void* handle, long long* params, long long* packed, long long* lazy, int* lazy_forms);
/* the device-side weight preparation on its own: raw torch OIHW [O][I][3][3] (device) -> operand form `kind` (61: the sub-pixel up form, see buddy_gn_upconv3x3_winograd6; 0 direct [Co][9][Ci], 2 Winograd
 * F(2x2,3x3) [Ci/8][16][Co][8], 4 F(4x4,3x3) [36][Co][Ci], 6 F(6x6,3x3) [64][Co][Ci]); dgrad != 0: the data-gradient direction (Co = I, Ci = O,
 * taps flipped).  out: conv weight count x (9 | 16 | 36 | 64) floats.  Weights of ddpm_conv3x3, networks/ncsnpp_utils/layers.py:119-126. */
int buddy_conv3_weight_prep(const float* w_oihw, int O, int I, int dgrad, int kind, float* out, void* stream);

/* size the activation arena for batch B, length L samples (done implicitly by forward; exposed to report bytes). */
int buddy_ncsnpp_reserve(void* handle, int B, int L, int with_vjp, long long* bytes);

/* y = cskip[b]*x + cout[b]*net(cin[b]*x, cnoise[b])  if cin/cskip/cout are non-NULL (EDM denoiser,
 * reference diff_params/shared.py:98-120), else y = net(x, cnoise) (NCSNppTime.forward).
 * x, y: [B][L]; cnoise, cin, cskip, cout: [B].  save_for_vjp != 0 keeps activations for buddy_ncsnpp_vjp; 2 also for buddy_ncsnpp_vjp_params. */
int buddy_ncsnpp_forward(void* handle, const float* x, const float* cnoise, const float* cin, const float* cskip,
                         const float* cout, float* y, int B, int L, int save_for_vjp, void* stream);

/* grad_x = (d y / d x)^T cot for the last forward issued with save_for_vjp (includes the EDM scalars if they were given). */
int buddy_ncsnpp_vjp(void* handle, const float* cot, float* grad_x, void* stream);

/* Parameter gradients (training / fine-tuning; reference training/trainer.py:225-243 loss.backward()).  After a forward issued with
 * save_for_vjp = 2 (the activation arena then also holds the gradient kernels' workspaces): grad_params = (d y / d params)^T cot, ONE device
 * buffer of buddy_ncsnpp_param_count(_attn) floats in the flat parameter order that buddy_ncsnpp_create(_attn) takes (attention sites included).
 * accumulate = 0 overwrites it, 1 adds to it.  The Fourier projection W gets zero (the reference registers it with requires_grad=False).
 * output_layer.bias is formed from the column sums of the frame gradient and the bin sums of the inverse-DFT basis, both in double (its real
 * component is exactly 0 for the periodic Hann window; a column sum of the fp32 spectrum gradient leaves rounding noise there).
 * grad_x (nullable) receives the same input gradient as buddy_ncsnpp_vjp, bit for bit.  Exact fp32 arithmetic in every GEMM mode; deterministic
 * (split-K over fixed pixel chunks, reduced in a fixed order, no atomics).  BUDDY_ERR_STATE after a forward with save_for_vjp = 0 / 1. */
int buddy_ncsnpp_vjp_params(void* handle, const float* cot, float* grad_x, float* grad_params, int accumulate, void* stream);

/* Replace the raw weights of the handle's weight store in place (dev_params: device, same flat layout) -- e.g. after an optimizer step.  No new
 * handle: a device copy of the parameters, one copy to the host to rebuild the small packed forms there, and every derived form (lazy 3x3 operand forms, packed 1x1 / NIN images and their stage images, the Dense_0 tables) is rebuilt or
 * dropped.  Replicas share the store: every handle made with buddy_ncsnpp_replica from it sees the new weights at its next forward, and a forward
 * saved by any of them before the update is refused by buddy_ncsnpp_vjp / _vjp_params (BUDDY_ERR_STATE).  No handle on the store may have work in
 * flight on another stream while it runs. */
int buddy_ncsnpp_update_params(void* handle, const float* dev_params, void* stream);

/* ---- the optimizer step of training (optim.hip; reference training/trainer.py:225-258: clip_grad_norm_, Adam.step, update_ema) on flat fp32
 * device buffers in the flat parameter order of buddy_ncsnpp_create / grad_params.  Two launches per step, none per parameter tensor.
 *
 * Sum of squares of n floats (the squared global gradient norm), accumulated in double: workgroup c sums the fixed chunk
 * [c, c + 1) * buddy_optim_sqnorm_chunk() floats into partials[c]; one finalising workgroup adds the partials in a fixed order (thread t takes
 * t, t + 256, ... in chunk order, then a fixed tree).  No atomics: two runs on the same input give the same bits.  partials: at least
 * ceil(n / chunk) doubles of workspace.  The result stays on the device: out[0] is one double that buddy_optim_step reads there. */
long long buddy_optim_sqnorm_chunk(void);
int buddy_optim_sqnorm(const float* g, long long n, double* partials, double* out, void* stream);
/* One pass over p, g, m, v, ema (n floats each, 16-byte aligned; 36 bytes per parameter):
 *   clip  coef = min(1, max_norm / (sqrt(*sqnorm) + 1e-6)) as torch.nn.utils.clip_grad_norm_ (max_norm <= 0: coef = 1, sqnorm may be NULL);
 *         the gradient used is coef * g.  g is NOT written: after the call it still holds the unclipped gradient.
 *   Adam  torch.optim.Adam's defaults (no amsgrad, no weight decay) in the order of its single-tensor form: m = beta1 m + (1 - beta1) g,
 *         v = beta2 v + (1 - beta2) g g, denom = sqrt(v) / bias2_sqrt + eps, p -= step_size * m / denom, with the host's
 *         step_size = lr / (1 - beta1^t) and bias2_sqrt = sqrt(1 - beta2^t).  Every element is computed in double from the fp32 inputs and
 *         rounded to fp32 once per stored value; the p update reads the stored (rounded) m and v.
 *   EMA   ema = ema * ema_s + p_new * (1 - ema_s) (trainer.py:245-258); ema == NULL skips it.
 * frozen: n_frozen <= 8 half-open element ranges [frozen[2 i], frozen[2 i + 1]) (host array; any alignment) inside which p, m, v are left
 * untouched bit for bit -- the Fourier projection W, which torch's Adam never sees -- while the EMA still runs there. */
int buddy_optim_step(float* p, const float* g, float* m, float* v, float* ema, long long n, const double* sqnorm, double max_norm, double beta1,
                     double beta2, double eps, double step_size, double bias2_sqrt, double ema_s, const long long* frozen, int n_frozen,
                     void* stream);
/* buddy_optim_step for data-parallel training: g holds the SUM of the ranks' gradients and grad_scale = 1 / world makes the step use their
 * average without another pass over the buffer: gc = coef * grad_scale * g with coef = min(1, max_norm / (grad_scale * sqrt(*sqnorm) + 1e-6)),
 * i.e. clip_grad_norm_ on the averaged gradient; *sqnorm is still the squared norm of the buffer as it is (of the sum), and g is not written.
 * grad_scale must be finite and > 0 (else BUDDY_ERR_ARG).  buddy_optim_step is this entry with grad_scale = 1, which is exact. */
int buddy_optim_step_scaled(float* p, const float* g, float* m, float* v, float* ema, long long n, const double* sqnorm, double max_norm,
                            double beta1, double beta2, double eps, double step_size, double bias2_sqrt, double ema_s, double grad_scale,
                            const long long* frozen, int n_frozen, void* stream);
/* Checksum of n floats by their bit patterns, for comparing the replicas of data-parallel training:
 *   out[0] = sum_i bits(x[i]) * (2 i + 1) mod 2^64   (bits = the 32-bit pattern, zero-extended; i = the element's index).
 * An integer sum, so independent of the reduction order; every multiplier is odd, hence invertible mod 2^64, so a change of one element
 * changes the result, and it depends on the position, so does a swap of two differing elements.  Same form as buddy_optim_sqnorm: x needs
 * 4-byte alignment only, partials is ceil(n / buddy_optim_sqnorm_chunk()) 64-bit words of workspace, no atomics, the result stays on the device. */
int buddy_optim_checksum(const float* x, long long n, unsigned long long* partials, unsigned long long* out, void* stream);
/* the EMA on its own (Trainer.update_ema outside a fused step): ema = ema * ema_s + p * (1 - ema_s), n floats, 16-byte aligned */
int buddy_optim_ema(float* ema, const float* p, long long n, double ema_s, void* stream);

/* ---- the parameter-gradient kernels of training on their own (wgrad.hip; the network reaches them through buddy_ncsnpp_vjp_params).  Every
 * result is ADDED into its output, as gradients accumulate over micro-batches; no atomics, so two runs give the same bits.  All tensors are
 * fp32 device buffers unless stated; workspaces are in floats (4 bytes) and need no initialisation.
 *
 * dY view (weight gradient and column sums): dY[m][n] = dy[(m / T) * sb + (m % T) * sm + n * sn], m < M.  A row-major [M][ld] gradient is
 * T = rows per utterance, sb = T * ld, sm = ld, sn = 1; a per-utterance transposed one [B][N][T] (the attention's dV^T) is sb = T * N, sm = 1, sn = T.
 *
 * Weight gradient G[n][k] = sum_m dY[m][n] A[m][k], M = B * H * W pixels on the (H, W) grid of the convolution's output (NHWC, H = time = kx,
 * W = frequency = ky), k = tap * Cin + c, tap = 3 (dh + 1) + (dw + 1) over the zero-padded 3 x 3 neighbourhood (taps = 9) or the pixel itself
 * (taps = 1).  A is evaluated by the loader from the channel concatenation x = cat[x0 (C0 channels, row stride ld0), x1 (Cin - C0, ld1)] (x1 NULL:
 * x0 alone, Cin channels): act(GroupNorm(x)) with stats [B][G][2] = (mean, rstd), gamma, beta [Cin] and SiLU if silu (stats NULL: no
 * normalisation), then rs = 0: x on the (H, W) grid; rs = 1: x at (2H, 2W), the 2 x 2 box mean of the activated values; rs = 2: x at (H/2, W/2),
 * nearest (H, W even).  out += alpha * G in layout 0 = [N][K], 1 = torch OIHW of a 3 x 3 convolution [N][Cin][ky = dw + 1][kx = dh + 1]
 * (taps = 9), 2 = [K][N].  Exact fp32 products on the matrix cores; split over fixed pixel chunks (buddy_weight_grad_chunks of them, each a
 * multiple of 32 pixels) that a second pass adds in chunk order.  ws: buddy_weight_grad_workspace(M, N, K = taps * Cin) floats. */
long long buddy_weight_grad_workspace(long long M, int N, int K);
int buddy_weight_grad_chunks(long long M, int N, int K);
int buddy_weight_grad(const float* dy, long long T, long long sb, long long sm, long long sn, const float* x0, const float* x1, int C0, int ld0, int ld1,
                      int H, int W, int Cin, int taps, int rs, const float* stats, const float* gamma, const float* beta, int G, int silu, int B, int N,
                      int layout, float alpha, float* ws, float* out, void* stream);
/* Column sums of a dY view of B utterances of T rows, accumulated in double: bc[b * ld_bc + n] = sum_t dY[b T + t][n] (overwritten, ld_bc >= N);
 * out[n] and out2[n] += alpha * the sum over all rows.  bc, out, out2 are each optional (NULL), at least one is given.
 * ws: buddy_colsum_workspace(B, T, N) floats, 8-byte aligned. */
long long buddy_colsum_workspace(int B, long long T, int N);
int buddy_colsum(const float* dy, long long T, long long sb, long long sm, long long sn, int B, int N, float alpha, float* ws, float* bc, int ld_bc,
                 float* out, float* out2, void* stream);
/* output_layer.bias: out[c] += sum_k bsum[c][k] * (sum over the B * T rows of x[row][k]), c = 0, 1; x [B * T][K] fp32, bsum [2][K] double (device);
 * all in double, rounded once.  ws: buddy_colsum_workspace(B, T, K) floats, 8-byte aligned. */
int buddy_basis_bias(const float* x, int K, int B, long long T, const double* bsum, float* ws, float* out, void* stream);
/* GroupNorm affine gradients of a = act(GroupNorm(x)) given da: dgamma[c] += sum dz * xhat, dbeta[c] += sum dz, dz = da_eff * act'(z),
 * z = xhat * gamma + beta, over the B * H * W pixels of x = cat[x0, x1] (as above) at (H, W); accumulated in double.  da [.][C] dense NHWC at
 * (H, W) (da_mode 0), at (H/2, W/2) and scaled by 1/4 (da_mode 1: the box downsample's adjoint; H, W even) or at (2H, 2W) and summed over the four
 * children (da_mode 2: the nearest upsample's).  ws: buddy_gn_param_grads_workspace(B, H, W, C) floats, 8-byte aligned. */
long long buddy_gn_param_grads_workspace(int B, int H, int W, int C);
int buddy_gn_param_grads(const float* x0, const float* x1, int C0, int ld0, int ld1, const float* stats, const float* gamma, const float* beta, int G,
                         int silu, const float* da, int da_mode, int B, int H, int W, int C, float* ws, float* dgamma, float* dbeta, void* stream);
/* Backward of y[b][j] = sum_k act(x[b][k]) W[j][k] + bias[j] (the time-embedding MLP; act = SiLU if silu_in, else the identity), B utterances:
 * gw[j][k] += sum_b dy[b * ld_dy + j] act(x[b][k]); gb[j] and gb2[j] += sum_b dy[b * ld_dy + j] (each optional);
 * dx[b][k] = act'(x[b][k]) * sum_j dy[b * N + j] W[j][k] (overwritten; dy dense).  x [B][K], W [N][K]. */
int buddy_linear_bwd_w(const float* dy, int ld_dy, const float* x, int silu_in, int B, int N, int K, float* gw, float* gb, float* gb2, void* stream);
int buddy_linear_bwd_x(const float* dy, const float* W, const float* x, int silu_in, int B, int N, int K, float* dx, void* stream);

/* debugging / per-module parity: device pointer + NHWC dims ([B][frames][bins][C]) of the output of all_modules[idx]. */
int buddy_ncsnpp_tap(void* handle, int module_idx, const float** ptr, int dims[4]);

/* device-to-device copy on `stream` (used to read taps without touching another HIP runtime handle) */
int buddy_copy_d2d(void* dst, const void* src, long long bytes, void* stream);

/* ---- measurement: time every matrix-core (igemm) launch with HIP events on its own launch stream.  collect() waits for
 * the recorded events and returns, per class (index 0: 3x3 convolutions, index 1: 1x1 convs / attention / DFT GEMMs),
 * the summed kernel time [ms], the algorithmic FLOPs (2*M*N*K, zero padding counted like torch's flop counter) and
 * the number of launches since the last collect, and the algorithmic bytes (A once + weights once + C once). ---- */
/* level: 0 off; 1 only the dominant kernel (the 36 batched GEMMs of the three-pass convolutions; collect with buddy_prof_collect_wino4, only its
 * GEMM entries are filled) -- every event pair costs a dispatch bubble of several microseconds, so a throughput measurement brackets nothing
 * else; 2 every instrumented class (attribution). */
int buddy_prof_enable(int level);
int buddy_prof_collect(double* ms /*[2]*/, double* flops /*[2]*/, long long* launches /*[2]*/, double* bytes /*[2]*/,
                       double* executed_flops /*[2]: = flops except for Winograd launches (4/9 of the direct-conv flops)*/);
/* same for the HBM-bound GroupNorm launch groups (statistics; apply + SiLU + resample; backward sums + apply): summed time [ms],
 * algorithmic bytes (each pass reads its inputs once and writes its output once) and launch-group count since the last collect. */
int buddy_prof_collect_hbm(double* ms, double* bytes, long long* launches);
/* per-pass totals of the three-pass F(4x4,3x3) convolutions since the last collect: ms[3] = {input transform, 36 batched GEMMs, output
 * transform}, executed FLOPs of the GEMM pass (2 * 36 * tiles * Cin * Cout), algorithmic bytes of the two transform passes and of the GEMM pass. */
int buddy_prof_collect_wino4(double* ms /*[3]*/, double* gemm_flops, double* bytes_in, double* bytes_out, double* bytes_gemm, long long* launches);

/* calibration: `blocks` workgroups x 4 waves issue 4*iters fp32 MFMAs (32x32x2) each on operands from seed[1024] with no
 * memory traffic; out[blocks*256] keeps the result live; clk[0] = shader clocks, clk[1] = 100 MHz wall ticks of block 0.
 * FLOPs = blocks * 4 waves * 4 * iters * 4096. */
int buddy_mfma_ubench(const float* seed, float* out, int blocks, int iters, unsigned long long* clk, void* stream);
/* the same loop on v_mfma_f32_32x32x16_bf16 with random operand bits (12 MFMAs = 393 216 FLOP per wave and iteration): the bf16 matrix rate this box
 * sustains under its power budget, the ceiling of the bf16x3 GEMM */
int buddy_mfma_ubench_bf16(const float* seed, float* out, int blocks, int iters, unsigned long long* clk, void* stream);

/* calibration: one streaming pass over `bytes` (a multiple of 16, 16-byte aligned device buffers): mode 0 copy src -> dst (bytes read + bytes written),
 * 1 read src (summed in registers), 2 write dst; nt != 0 uses the non-temporal loads / stores.  blocks >= 1: that many workgroups of 256 threads stride
 * over the array in contiguous chunks of 8 x 256 sixteen-byte words (eight independent requests per thread); blocks = -1 | -2 | -4 | -8: the one-shot
 * form, one chunk of that many words per thread and workgroup (-1 = the classic one-float4-per-thread copy).  mode 3 / 4: READ in the access pattern of
 * the batched GEMM's A operand (rows of nt = 512 | 1024 | 2048 bytes, 64 bytes per lane and K-stage in four 16-byte loads, 64 rows per wave): all stages'
 * loads in flight (3) or one stage ahead with a stand-in for the matrix work between them (4); `blocks` is ignored.  The HBM rate a plain kernel reaches on THIS box, next to the nominal 8 TB/s (MI355X_MICROARCH.md records 6.29 TB/s for a
 * float4 copy): the second denominator of every HBM-bound roofline in bench.py. */
int buddy_hbm_ubench(const void* src, void* dst, long long bytes, int mode, int nt, int blocks, void* stream);

/* ---- unit-level kernels (the pieces the network is made of; used by the parity tests) ---- */
/* C[b] = alpha * op(A[b]) op(Bt[b])^T (+ bias_n), row-major; transX = operand stored k-major. replaces torch.einsum/bmm
 * in AttnBlockpp (networks/ncsnpp_utils/layerspp.py:82-86) and NIN (layers.py:548-557). */
int buddy_gemm(const float* A, int ldA, int transA, const float* Bt, int ldB, int transB, float* C, int ldC, int M, int N,
               int K, float alpha, const float* bias_n, int accumulate, int batch, long long strideA, long long strideB,
               long long strideC, void* stream);
/* The batched Winograd-domain products of the three-pass 3x3 convolutions on their own (benchmarks, tools/gemm36.py):
 * M[p] (tiles x Cout) = V[p] (tiles x Cin) . U[p]^T (Cout x Cin), p < positions (36 = F(4x4,3x3), 64 = F(6x6,3x3)), dense strides.
 * Same arithmetic as buddy_gemm; this entry point selects the instantiation the convolutions use (own name in profiles). */
int buddy_gemm_winograd_domain(const float* V, const float* U, float* M, int tiles, int Cout, int Cin, int positions, void* stream);
/* The same products in "bf16x3" arithmetic (csrc/wgemm.hip): every fp32 operand split exactly into three bf16 terms, six bf16 MFMA products,
 * fp32 accumulation -- the accuracy of the fp32 kernel at 2.67x fewer matrix-pipe cycles.  The weights are split once into the kernel's LDS
 * stage image: U3 = buddy_wgemm_packed_bytes(...) bytes of device memory filled by buddy_wgemm_pack_weights from U [positions][Cout][Cin]
 * (device).  Cout % 128 == 0, Cin % 32 == 0 (packed_bytes returns 0 otherwise). */
long long buddy_wgemm_packed_bytes(int positions, int Cout, int Cin);
int buddy_wgemm_pack_weights(const float* U, void* U3, int positions, int Cout, int Cin, void* stream);
int buddy_gemm_winograd_domain_bf16x3(const float* V, const void* U3, float* M, int tiles, int Cout, int Cin, int positions, void* stream);
/* The same products in "f16x2" arithmetic (csrc/wgemm.hip; network option gemm = "f16x2"): every fp32 operand scaled by a power of two and split into
 * two f16 terms (22 significant bits), three f16 MFMA products (lo*hi + hi*lo + hi*hi), fp32 accumulation -- half the matrix-pipe cycles of bf16x3 for operands
 * good to 2^-22 instead of 2^-24.  U2 = buddy_wgemm_f16x2_packed_bytes(...) bytes filled by buddy_wgemm_f16x2_pack_weights (one power of two per position;
 * positions <= 64, Cout % 128 == 0, Cin % 64 == 0, else 0).
 * The rows of V are `tiles` = utterances * tiles_per_utt (tiles_per_utt >= 32); vmax holds the abs-max of V per utterance (over all positions) as 64
 * partial maxima, float bit patterns, one per 128-byte line: unsigned [utterances][64][32], word 0 of each line used (buddy_abs_max_bits fills it; the
 * three-pass convolutions collect it inside their input transform with one atomic max per tile): the power of two of V's scale is derived from the exponent
 * field of the largest, so an utterance's result does not depend on the rest of the batch. */
long long buddy_wgemm_f16x2_packed_bytes(int positions, int Cout, int Cin);
int buddy_wgemm_f16x2_pack_weights(const float* U, void* U2, int positions, int Cout, int Cin, void* stream);
int buddy_gemm_winograd_domain_f16x2(const float* V, const void* U2, float* M, int tiles, int Cout, int Cin, int positions, const unsigned* vmax,
                                     int tiles_per_utt, void* stream);
/* The same products in plain "f16" arithmetic (csrc/wgemm16.hip; network option gemm = "f16", the opt-in fast mode): ONE f16 term per operand element,
 * one v_mfma_f32_32x32x16_f16 per 16 k, fp32 accumulation.  Operand format (positions <= 64, Cout % 128 == 0, Cin % 32 == 0, else 0 / an error):
 *   V16  [positions][tiles][Cin] _Float16: V16[p][t][c] = f16_rn(V[p][t][c] * 2^vexp[t]), round to nearest even;
 *   vexp [tiles] int8: one power of two per ROW (the F(6x6,3x3) tile, shared by all positions), in [-112, 126]; the convolutions choose it inside their
 *        input transform from the tile's abs-max m over all positions and channels: vexp = 141 - clamp(exponent field of m, 15, 253), so m * 2^vexp lies
 *        in [2^14, 2^15) (an all-zero tile: 126);
 *   U1   = buddy_wgemm_f16_packed_bytes(...) bytes filled by buddy_wgemm_f16_pack_weights from U [positions][Cout][Cin] (device): per position
 *        eu[p] = 141 - clamp(exponent field of max |U[p]|, 15, 253) and the elements f16_rn(U[p][n][c] * 2^eu[p]) in the kernel's stage order, then
 *        positions floats u_inv[p] = 2^-eu[p];
 *   M[p][t][n] = 2^-vexp[t] * u_inv[p] * sum_c V16[p][t][c] * f16_rn(U[p][n][c] * 2^eu[p])   (fp32 accumulation). */
long long buddy_wgemm_f16_packed_bytes(int positions, int Cout, int Cin);
int buddy_wgemm_f16_pack_weights(const float* U, void* U1, int positions, int Cout, int Cin, void* stream);
int buddy_gemm_winograd_domain_f16(const void* V16, const signed char* vexp, const void* U1, float* M, int tiles, int Cout, int Cin, int positions, void* stream);
/* out [segments][64][32]: partial maxima (bit patterns, word 0 of each 128-byte line) of |x| over segment u of every one of `groups` equally spaced blocks:
 * x is [groups][segments][seg_len] floats (V: groups = positions, segments = utterances, seg_len = tiles_per_utt * Cin); out is overwritten. */
int buddy_abs_max_bits(const float* x, int groups, int segments, long long seg_len, unsigned* out, void* stream);
/* The 1x1 convolutions / NIN layers (layers.py:100-106, 548-557) on the same kernel: C (M x N, row stride ldC) = alpha * [A0 | A1] W^T + bias_n
 * (+ C if accumulate); the K input channels come from A0 (first C0, row stride ldA0) and, if A1 != NULL, A1 (the rest, ldA1) -- the U-Net's
 * channel concatenation is never materialised.  W3 = buddy_wgemm_pack_weights(W [N][K], ., 1, N, K).  N % 128, K % 32, C0 % 32 == 0. */
int buddy_gemm_bf16x3(const float* A0, int ldA0, const float* A1, int ldA1, int C0, const void* W3, float* C, int ldC, long long M, int N, int K,
                      const float* bias_n, float alpha, int accumulate, void* stream);
/* A ResBlock's input gradient in one GEMM launch (layerspp.py:242-274 backward): dx = alpha * A W^T + the input-gradient of act(GroupNorm(cat[x0, x1]))
 * for the incoming da -- the skip path's 1x1 data-gradient (Conv_2^T; A = the block's output gradient, M = B * HW rows, K channels; W3 =
 * buddy_wgemm_pack_weights(W [N][K], ., 1, N, K)) with the GroupNorm backward's apply pass as the GEMM's epilogue: neither the 1x1 result nor a separate
 * apply pass reaches HBM.  x / dx: channel-concatenated views split at C0 (x1 = dx1 = NULL: one tensor); accK != 0: that destination accumulates.
 * stats: forward (mean, rstd) [B][G][2]; red [B][G][2] out; stat_scratch >= B*256*N*16 bytes.  N % 128, K % 32, C0 % 128 == 0. */
int buddy_gemm_bf16x3_gn_bwd(const float* A, int ldA, const void* W3, const float* x0, const float* x1, int C0, const float* da, const float* stats,
                             const float* gamma, const float* beta, int G, int silu, float alpha, float* dx0, float* dx1, int acc0, int acc1,
                             double* stat_scratch, float* red, int B, int HW, int N, int K, void* stream);
/* The two general forms above in f16x2 arithmetic (round 6; what a handle with gemm = f16x2 runs where option gen_f16x2 says so): W2 =
 * buddy_wgemm_f16x2_pack_weights(W, ., 1, N, K) (one power of two for the matrix); the A operand's power of two is taken PER ROW inside the kernel,
 * found on the way along K (a stage that leaves the current scale's range rescales the row's accumulators by an exact power of two: no pre-pass), so a
 * row's result depends on nothing but the row.  K % 64 == 0; everything else as the bf16x3 entries.  Options gen_f16x2 (1: the network's 1x1 / NIN /
 * skip-path launches use these; 0: the exact bf16x3 split), gen_rows (0 by size | 32 | 64 rows per wave), gen_cp (two column blocks per workgroup). */
int buddy_gemm_f16x2(const float* A0, int ldA0, const float* A1, int ldA1, int C0, const void* W2, float* C, int ldC, long long M, int N, int K,
                     const float* bias_n, float alpha, int accumulate, void* stream);
int buddy_gemm_f16x2_gn_bwd(const float* A, int ldA, const void* W2, const float* x0, const float* x1, int C0, const float* da, const float* stats,
                            const float* gamma, const float* beta, int G, int silu, float alpha, float* dx0, float* dx1, int acc0, int acc1,
                            double* stat_scratch, float* red, int B, int HW, int N, int K, void* stream);
/* NHWC 3x3 stride-1 pad-1 conv, packed weights wt[Cout][9*Cin] (tap-major, channel-minor); replaces ddpm_conv3x3
 * (networks/ncsnpp_utils/layers.py:119-126). */
int buddy_conv3x3(const float* x, const float* wt, const float* bias, float* y, int B, int H, int W, int Cin, int Cout,
                  void* stream);
/* the same convolution through the fused Winograd F(2x2,3x3) kernel (4*Cin instead of 9*Cin MACs per output, fp32):
 * transform_weights (host -> host): wt[Cout][9*Cin] -> U[Cin/8][16 positions][Cout][8]; conv takes U on the device. */
int buddy_winograd_transform_weights(const float* wt_host, int Cout, int Cin, float* U_host);
int buddy_conv3x3_winograd(const float* x, const float* U, const float* bias, float* y, int B, int H, int W, int Cin, int Cout,
                           void* stream);
/* F(4x4,3x3) three-pass variant (input transform, 36 batched GEMMs, output transform) used for the large layers: U4[36][Cout][Cin];
 * scratch: 36 * (B*H*W/16) * (Cin + Cout) floats. */
int buddy_winograd4_transform_weights(const float* wt_host, int Cout, int Cin, float* U4_host);
int buddy_conv3x3_winograd4(const float* x, const float* U4, const float* bias, float* y, float* scratch, int B, int H, int W, int Cin, int Cout,
                            void* stream);
/* F(6x6,3x3) three-pass variant for the large layers (64 positions, 8x8 input patch per 6x6 output tile: 1.78 instead of 2.25 multiply-adds per
 * output, any H, W >= 6 -- tiles may overhang): U6[64][Cout][Cin]; scratch: 64 * B * ceil(H/6) * ceil(W/6) * (Cin + Cout) floats. */
int buddy_winograd6_transform_weights(const float* wt_host, int Cout, int Cin, float* U6_host);
int buddy_conv3x3_winograd6(const float* x, const float* U6, const float* bias, float* y, float* scratch, int B, int H, int W, int Cin, int Cout,
                            void* stream);
/* the same convolution with the Winograd-domain GEMM in plain f16 (network option gemm = "f16"): U1 = buddy_wgemm_f16_pack_weights of U6 (positions 64),
 * Cout % 128 == 0, Cin % 32 == 0; scratch as above.  On return the first 64 * tiles * Cin * 2 bytes of scratch hold V16 and the next `tiles` bytes vexp
 * (format of buddy_gemm_winograd_domain_f16; tiles = B * ceil(H/6) * ceil(W/6)). */
int buddy_conv3x3_winograd6_f16(const float* x, const void* U1, const float* bias, float* y, float* scratch, int B, int H, int W, int Cin, int Cout,
                                void* stream);
/* The three GroupNorm-fused forms and the sub-pixel data-gradient below with the GEMM in plain f16: the same arguments with the f16 image U1 (positions 64,
 * buddy_wgemm_f16_pack_weights of the fp32 form: [64][Cout][Cin], kind 61 [64][4 Cout][Cin] for the up form, [64][Cout][4 C] for its data-gradient) in
 * place of U6; the GEMM's Cout % 128 == 0 and K % 32 == 0.  V16 and vexp in scratch as for buddy_conv3x3_winograd6_f16 (K = 4 C channels in the
 * data-gradient of the up form; tiles of the sub-pixel forms: B * (H / 7 + 1) * (W / 7 + 1) forward, B * ceil(H / 7) * ceil(W / 7) data-gradient). */
int buddy_gn_conv3x3_winograd6_f16(const float* x0, const float* x1, int C0, const float* gamma, const float* beta, int G, int silu, const void* U1,
                                   const float* bias, float* y, float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W,
                                   int Cin, int Cout, void* stream);
int buddy_gnbwd_conv3x3_winograd6_f16(const float* x, const float* gamma, const float* beta, const float* stats, const float* da, int G, int silu,
                                      const void* U1, float* y, float* scratch, double* stat_scratch, float* red, int B, int H, int W, int C, int Cout,
                                      void* stream);
int buddy_gn_upconv3x3_winograd6_f16(const float* x, const float* gamma, const float* beta, int G, int silu, const void* U1up, const float* bias, float* y,
                                     float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W, int Cin, int Cout, void* stream);
int buddy_gnbwd_upconv3x3_winograd6_f16(const float* h, const float* gamma, const float* beta, const float* stats, const float* da, int G, int silu,
                                        const void* U1upT, float* y, float* scratch, double* stat_scratch, float* red, int B, int H, int W, int C,
                                        int Cout, void* stream);
/* act(GroupNorm(cat[x0, x1])) -> conv3x3 as ONE three-pass convolution: the normalisation and SiLU are applied inside the input transform
 * (the activated tensor never reaches HBM) and, with csum != NULL, the output transform leaves the per-(utterance, channel) sum and sum of
 * squares of y (csum[B][Cout][2], float64) -- the statistics the NEXT GroupNorm needs (layerspp.py:243-245, 257-259).  x1 may be NULL (single
 * source; C0 ignored).  stats: [B][G][2] out.  scratch as for buddy_conv3x3_winograd4; stat_scratch: >= B*256*1024*16 bytes. */
int buddy_gn_conv3x3_winograd4(const float* x0, const float* x1, int C0, const float* gamma, const float* beta, int G, int silu, const float* U4,
                               const float* bias, float* y, float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W,
                               int Cin, int Cout, void* stream);
/* the same through the F(6x6,3x3) passes (scratch as for buddy_conv3x3_winograd6) */
int buddy_gn_conv3x3_winograd6(const float* x0, const float* x1, int C0, const float* gamma, const float* beta, int G, int silu, const float* U6,
                               const float* bias, float* y, float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W,
                               int Cin, int Cout, void* stream);
/* The data-gradient side of the same fusion: da = conv3x3(g) (U6 = the transposed / flipped weights in the F(6x6,3x3) domain) is the gradient
 * w.r.t. act(GroupNorm(cat[x0, x1])) (Cout channels); the output transform also leaves that GroupNorm's per-(utterance, channel) backward sums
 * chsum[B][Cout][2] = (sum dxhat, sum dxhat * xhat), dxhat = da * act'(z) * gamma, float64 -- what buddy_groupnorm_act_bwd otherwise obtains
 * with a reduction pass over (x, da).  stats: the forward (mean, rstd) [B][G][2]. */
int buddy_conv3x3_winograd6_gn_bwd_sums(const float* g, const float* U6, float* da, float* scratch, const float* x0, const float* x1, int C0,
                                        const float* stats, const float* gamma, const float* beta, int G, int silu, double* stat_scratch,
                                        double* chsum, int B, int H, int W, int Cin, int Cout, void* stream);
/* ... and the input side of the backward: y = conv3x3(dx), dx = the input-gradient of act(GroupNorm(x)) for the incoming gradient da, with the
 * GroupNorm backward's apply pass evaluated inside the F(6x6,3x3) input transform (dx never reaches HBM).  stats: forward (mean, rstd) [B][G][2];
 * red: [B][G][2] out (the two per-group backward means); stat_scratch: >= B*256*C*16 bytes. */
int buddy_gnbwd_conv3x3_winograd6(const float* x, const float* gamma, const float* beta, const float* stats, const float* da, int G, int silu,
                                  const float* U6, float* y, float* scratch, double* stat_scratch, float* red, int B, int H, int W, int C, int Cout,
                                  void* stream);
/* The up ResBlock's first convolution, Conv_0(naive_upsample_2d(act(GroupNorm_0(x)))) (layerspp.py:243-257, up_or_down_sampling.py:172-176), as ONE
 * three-pass F(6x6,3x3) convolution on the LOW-resolution grid ("sub-pixel" form): x (B, H, W, Cin) -> y (B, 2H, 2W, Cout).  Output pixel
 * (2i + py, 2j + px) reads a 2x2 subset of the upsampled taps, so each of the four phases is a 3x3 convolution of x with summed taps; U6up
 * [64][4 Cout][Cin] = buddy_conv3_weight_prep(kind 61, dgrad 0).  Neither the activated nor the upsampled tensor reaches HBM.  csum (optional):
 * per-(utterance, channel) (sum, sum of squares) of y, float64.  scratch: 64 * B * ceil(H/6) * ceil(W/6) * (Cin + 4 Cout) floats; stats [B][G][2]
 * out; stat_scratch >= B*256*1024*16 bytes. */
int buddy_gn_upconv3x3_winograd6(const float* x, const float* gamma, const float* beta, int G, int silu, const float* U6up, const float* bias, float* y,
                                 float* scratch, float* stats, double* stat_scratch, double* csum, int B, int H, int W, int Cin, int Cout, void* stream);
/* Its data-gradient with the GroupNorm_1 backward in front (the up block's backward between Conv_1 and Conv_0): y (B, H, W, Cout) = the gradient
 * w.r.t. the LOW-resolution input of conv3x3(upsample(.)) for the high-resolution gradient dx, dx = input-gradient of act(GroupNorm(h)) for the
 * incoming da; h, da: (B, 2H, 2W, C), read space-to-depth inside the input transform.  U6upT [64][Cout][4 C] = buddy_conv3_weight_prep(kind 61,
 * dgrad 1) of the OIHW tensor [C][Cout][3][3].  stats: forward (mean, rstd) of h [B][G][2]; red [B][G][2] out; scratch: 64 * tiles * (4 C + Cout)
 * floats; stat_scratch >= B*256*C*16 bytes. */
int buddy_gnbwd_upconv3x3_winograd6(const float* h, const float* gamma, const float* beta, const float* stats, const float* da, int G, int silu,
                                    const float* U6upT, float* y, float* scratch, double* stat_scratch, float* red, int B, int H, int W, int C,
                                    int Cout, void* stream);
/* GroupNorm(G, C, eps=1e-6) [+SiLU] [+2x down(mode 1)/up(mode 2)] forward; replaces nn.GroupNorm + nn.SiLU +
 * naive_{up,down}sample_2d (layerspp.py:243-258). stats: [B][G][2] out; scratch: >= B*256*C*16 bytes. */
int buddy_groupnorm_act(const float* x, const float* gamma, const float* beta, float* y, float* stats, void* scratch, int B,
                        int H, int W, int C, int G, int mode, int silu, void* stream);
/* input-gradient of the above given dy (at the resampled resolution). red: [B][G][2] scratch. */
int buddy_groupnorm_act_bwd(const float* x, const float* gamma, const float* beta, const float* stats, const float* dy, float* dx,
                            void* scratch, float* red, int B, int H, int W, int C, int G, int mode, int silu, void* stream);
/* The same two operations with everything the network's GroupNorm launchers take (unit tests).  Source view: channels [0, C0) from x0 at a row
 * stride of ld0 floats, and with x1 != NULL channels [C0, C0 + C1) from x1 at ld1 (C = C0 + C1; x1 NULL: C = C0, ld1 and C1 unused).  route 0:
 * statistics by one reduction over the view; route 1: per-source channel sums csum0 [B][C0][2] / csum1 [B][C1][2] (sum, sum of squares, float64,
 * outputs) and the statistics from them, as the network does.  pooled_raw (optional, mode 1 only): the 2x2 mean of x itself, (B, H/2, W/2, C).
 * y dense at the resampled resolution; stats [B][G][2] out; scratch >= B*256*C*16 bytes.
 * All four GroupNorm entries refuse (BUDDY_ERR_ARG, before any launch): a null required pointer; B, H, W, C, G < 1; C % G; (C / G) % 4; C > 1024;
 * C0 % 4 (Cd0 % 4); a row stride below its width or not a multiple of 4; odd H or W with mode 1 or extra_mode 2; pooled_raw outside mode 1; a
 * mode, extra_mode or route out of range. */
int buddy_groupnorm_view_fwd(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, const float* gamma, const float* beta, int G,
                             int mode, int silu, float* y, float* pooled_raw, float* stats, int route, double* csum0, double* csum1,
                             double* scratch, int B, int H, int W, void* stream);
/* Input-gradient: dx = GroupNorm backward of dy (dense, at the resampled resolution) + the extra gradient: extra_mode 1: extra_scale * extra
 * (B, H, W, C); extra_mode 2: 0.25 * extra_scale * extra (B, H/2, W/2, C) at (h >> 1, w >> 1); extra_mode 0: extra NULL.  Destination view:
 * channels [0, Cd0) to dx0 at a row stride of ldd0, the rest to dx1 at ldd1 (dx1 NULL: Cd0 = C); a part whose acc flag is set is added to,
 * the other overwritten.  stats: the forward's; red [B][G][2] out; scratch >= B*256*C*16 bytes. */
int buddy_groupnorm_view_bwd(const float* x0, int ld0, int C0, const float* x1, int ld1, int C1, const float* gamma, const float* beta,
                             const float* stats, const float* dy, int G, int mode, int silu, const float* extra, int extra_mode,
                             float extra_scale, float* dx0, int ldd0, int acc0, float* dx1, int ldd1, int acc1, int Cd0, double* scratch,
                             float* red, int B, int H, int W, void* stream);

/* fir=True resampling (networks/ncsnpp_utils/up_or_down_sampling.py:195-257 upsample_2d / downsample_2d -> upfirdn2d, op/upfirdn2d_kernel.cu)
 * with the (1,3,3,1) kernel, factor 2, NHWC: up != 0: (H,W) -> (2H,2W), else (H,W) -> (H/2,W/2); y = (accumulate ? y : 0) + scale * resample(x).
 * The transposes are the other direction times 4 resp. 1/4.  buddy_ncsnpp_set_fir switches a network handle to this resampling (no parameters). */
int buddy_fir_resample2(const float* x, float* y, int B, int H, int W, int C, int up, float scale, int accumulate, void* stream);
int buddy_ncsnpp_set_fir(void* handle, int fir);
/* Per-handle launcher options -- "no hidden global state" (SURVEY.md 8(b)): every switch a launcher consults (attention core, GEMM arithmetic, the
 * fusions and kernel forms the tests compare) is a field of the handle's option struct; two handles in one process may differ.  Keys (csrc/options.hip): conv, gemm,
 * attention, gn_fuse, upconv, c2_fuse, attn_split, attn_nw, wgemm_rt, wgemm_cb, gen_f16x2, gen_rows, gen_cp, gnb_nt, c2out_tiled, op_graph.  An unknown key (the
 * retired A/B switches included) or a value out of range is BUDDY_ERR_ARG.  A handle starts from the process defaults = the BUDDY_<KEY> environment variables, parsed and validated in ONE place at handle
 * creation: a bad value, or an unknown BUDDY_* name within edit distance 2 of a switch (a misspelling), makes buddy_ncsnpp_create fail with a message naming it;
 * the environment name of a retired A/B switch fails the same way ("... has been retired; unset it"); BUDDY_* names that resemble no switch are not this
 * library's and are left alone.  Set options before the first forward or between calls: the
 * activation arena is sized again and a saved forward is dropped (buddy_ncsnpp_vjp returns BUDDY_ERR_STATE until the next forward with save = 1). */
int buddy_options_check(void);   /* the environment check alone (no GPU needed): BUDDY_OK, or BUDDY_ERR_ARG with buddy_last_error() naming the variable */
int buddy_option_validate(const char* key, int value);   /* would buddy_ncsnpp_set_option accept (key, value)?  no handle, no GPU, nothing changed */
int buddy_ncsnpp_set_option(void* handle, const char* key, int value);
int buddy_ncsnpp_get_option(void* handle, const char* key, int* value);
/* attention core of a network handle: 4 = auto (default; fp32: the materialised T x T form while T <= 4096, the online-softmax kernels beyond -- a
 * function of T alone); 0 = online-softmax kernels, fp32 operands; 1 / 2 = the same with bf16 / f16 MFMA operands (opt-in fast mode, fp32 accumulate
 * + fp32 softmax); 3 = always the materialised T x T matrix.  Initial value from BUDDY_ATTN = auto | flash | bf16 | f16 | matrix. */
int buddy_ncsnpp_set_attention(void* handle, int mode);
/* Arithmetic of the Winograd-domain GEMMs of the 3x3 convolutions (94 % of the FLOPs):
 *   2 (default) = "f16x2": both fp32 operands scaled by a power of two and split by round-to-nearest into TWO f16 terms (22 significant bits instead of
 *       fp32's 24), three f16 MFMA products, fp32 accumulation; measured against float64 it is as close as the exact forms (one denoiser evaluation +
 *       VJP 117.2 / 113.0 dB), but it is NOT bit-for-bit the fp32 product;
 *   1 = "bf16x3": every fp32 operand split EXACTLY into three bf16 terms, six bf16 MFMA products, fp32 accumulation: the fp32 kernel's accuracy;
 *   0 = v_mfma_f32_32x32x2_f32 (bit-exact fp32 FMA chains; the reference run);
 *   3 = "f16", the OPT-IN FAST MODE (not the default, never the headline): the batched F(6x6,3x3) / sub-pixel GEMMs and their input transforms in plain f16
 *       -- V stored as ONE f16 term with a power of two per tile, U as one f16 term per position scale, one f16 MFMA per 16 k (buddy_gemm_winograd_domain_f16);
 *       everything else as mode 2, and shapes the f16 GEMM refuses run what mode 2 runs.  11 operand bits instead of 22: one denoiser evaluation + VJP
 *       against float64 55.3 / 51.6 dB at sigma 0.5 and 67.5 / 63.3 dB at sigma 0.02 (mode 2: 117 / 113 dB); one F(6x6,3x3) convolution 0.7-1.8e-2 of the
 *       abs-max by form; against mode 2 on the same noise streams |delta SI-SDR to clean| <= 0.0022 dB over informed T = 50 chains and a median of 0.50 dB
 *       over the blind T = 50 headline batch (two float64 runs of that chaotic chain: 0.74 dB).
 * The general GEMMs (1x1 / NIN / skip path / DFT) run in bf16x3 in mode 1 and in f16x2 in modes 2 and 3 where their shape allows (bf16x3 with option
 * gen_f16x2 = 0).
 * Env BUDDY_GEMM=fp32|bf16x3|f16x2|f16 sets the process default. */
int buddy_ncsnpp_set_gemm(void* handle, int mode);

/* single-head attention over T tokens without the T x T matrix (online softmax, fp32 MFMA), token-major q, k, v, O [B][T][C], C in {32,64,128,256}:
 * O = softmax(scale * q k^T) v, lse [B][T] = row log-sum-exp; replaces the einsum / softmax / einsum of AttnBlockpp.forward
 * (networks/ncsnpp_utils/layerspp.py:82-86).  bwd: gradients of the same three steps given dO (delta [B][T] is scratch).
 * prec must be 0 (fp32 operands, the reference arithmetic); the 16-bit-operand kernels take a workspace and are the next three entries. */
int buddy_flash_attention_fwd(const float* q, const float* k, const float* v, float* O, float* lse, int B, int T, int C, float scale, int prec, void* stream);
int buddy_flash_attention_bwd(const float* q, const float* k, const float* v, const float* O, const float* dO, const float* lse, float* delta,
                              float* dq, float* dk, float* dv, int B, int T, int C, float scale, int prec, void* stream);
/* The same three steps with 16-bit MFMA operands, C in {64,128,256} only (C = 32: the fp32 entries) (prec 1 = bf16, 2 = f16; v_mfma_f32_32x32x16_*), fp32 accumulation and fp32 softmax statistics --
 * the opt-in fast mode of buddy_ncsnpp_set_attention(handle, 1 | 2) (BASELINE configs[4] "fp16 MFMA attention path"; not the reference's arithmetic).
 * A pre-pass converts q (times scale log2 e), k, v, dO once into 16-bit operand arrays in `ws` (buddy_flash_attention16_workspace floats: token-major
 * rows and channel-major transposes, T padded to 128); the kernels stream them through LDS by DMA and keep the softmax in registers (csrc/attn16.hip). */
long long buddy_flash_attention16_workspace(int B, int T, int C);
int buddy_flash_attention16_fwd(const float* q, const float* k, const float* v, float* O, float* lse, int B, int T, int C, float scale, int prec,
                                float* ws, void* stream);
int buddy_flash_attention16_bwd(const float* q, const float* k, const float* v, const float* O, const float* dO, const float* lse, float* delta,
                                float* dq, float* dk, float* dv, int B, int T, int C, float scale, int prec, float* ws, void* stream);
/* The same fp32 kernels with their sequential loop (keys in fwd / dq, queries in dk / dv) split over `splits` workgroups per row block and the partial
 * results combined in fixed split order (no atomics): what the network uses when T / 64 workgroups per utterance would leave most of the 256 CUs idle
 * -- ONE utterance at a time is the reference's own shape (testing/tester.py:132-153).  buddy_flash_attention_splits = the count the network picks: a
 * function of T alone (B is ignored), so that a row's result does not depend on the batch it is computed in,
 * buddy_flash_attention_workspace = floats of `ws` for a count (splits <= 0: for the picked one); every split must own at least one 32-row block. */
int buddy_flash_attention_splits(int B, int T);
long long buddy_flash_attention_workspace(int B, int T, int C, int splits);
int buddy_flash_attention_fwd_split(const float* q, const float* k, const float* v, float* O, float* lse, int B, int T, int C, float scale, int splits,
                                    float* ws, void* stream);
int buddy_flash_attention_bwd_split(const float* q, const float* k, const float* v, const float* O, const float* dO, const float* lse, float* delta,
                                    float* dq, float* dk, float* dv, int B, int T, int C, float scale, int splits, float* ws, void* stream);

/* ---- sampler elementwise / reductions (replace the tensor expressions of testing/EulerHeunSampler.py:41-72,
 * testing/EulerHeunSamplerDPS.py:61-69,115-157, diff_params/edm.py:83-96), per-utterance (row) semantics.  Every entry returns BUDDY_ERR_ARG
 * before any launch for B, L, n or M < 1; buddy_dps_update also for a t that is not > 0 (NaN included), buddy_fir for B > 65535 ---- */
/* out[b][i] = a[b]*x[b][i] + c[b]*y[b][i] (y may be NULL) */
int buddy_axpby_rows(const float* x, const float* y, const float* a, const float* c, float* out, int B, int L, void* stream);
/* stochastic churn: out = x + scale * eps (EulerHeunSampler.py:41-45, scale = sqrt(t_hat^2 - t^2)) */
int buddy_perturb(const float* x, const float* eps, float scale, float* out, long long n, void* stream);
/* ---- per-utterance Philox noise streams (seeded sampling, csrc/rng.hip): Philox4x32-10, stream b has the key keys[b] = (k0, k1) (device, (B, 2)
 * uint32); sample i of draw d of purpose p is word i & 3 of the block with counter (i >> 2, d, p, 0), a pure function of (key, p, d, i).
 * uniform = (w >> 8) 2^-24 in [0, 1); normals = Box-Muller per word pair (w0, w1) -> (z0, z1), (w2, w3) -> (z2, z3) with u1 = ((w_even >> 8) + 0.5) 2^-24,
 * u2 = (w_odd >> 8) 2^-24, r = sqrt(-2 log u1), z_even = r cospi(2 u2), z_odd = r sinpi(2 u2); |z| <= 5.887.
 * fill: out (R, B, n) fp32 contiguous, row (r, b) = draw draw0 + r of stream b; kind 0 normals, 1 uniforms, 2 the raw words bit-cast. */
int buddy_philox_fill(float* out, int R, int B, int n, const unsigned* keys, unsigned purpose, unsigned draw0, int kind, void* stream);
/* stochastic churn with the noise generated in registers: out = x + scale * eps, eps = normals of purpose 0, draw `draw` of stream b for row b of
 * x (B, L); the bits of the perturb entry above applied to the kind-0 fill of the same draw */
int buddy_perturb_philox(const float* x, const unsigned* keys, unsigned draw, float scale, float* out, int B, int L, void* stream);
/* fused Euler / Heun update of the DPS sampler (EulerHeunSamplerDPS.py:128-157, edm.py:83-96), per-utterance rows:
 *   x_den' = x_den * den_scale[b] (NULL = 1);  d = -t * (x_den' - x_hat) / t^2 + lh_scale[b] (NULL = 1) * lh (NULL = 0);
 *   out = base + dt * (w_prev * d_prev (NULL = 0) + w_cur * d);   d_out / x_den_out optional.
 * lh_scale (round 6): the guidance normaliser zeta / (||grad||_2 / sqrt(audio_len) + 1e-8) per utterance (:66-69, buddy_row_scale mode 1), so the raw
 * likelihood gradient goes in and no scaled copy of it is materialised. */
int buddy_dps_update(const float* x_hat, const float* x_den, const float* lh, const float* lh_scale, const float* den_scale, const float* base,
                     const float* d_prev, float t, float dt, float w_prev, float w_cur, float* out, float* d_out, float* x_den_out, int B, int L, void* stream);
/* one scalar per utterance row of x (B, L), one launch, fp64 accumulation: mode 0: out[b] = p0 / std(x_b) (unbiased, Tensor.std(): the speech-magnitude
 * constraint, :127-129); mode 1: out[b] = p0 / (||x_b||_2 / p1 + 1e-8) (the guidance normaliser with p0 = zeta, p1 = sqrt(audio_len)) */
int buddy_row_scale(const float* x, float* out, int B, int L, int mode, float p0, float p1, void* stream);
/* out[k][b] = v_k, k < 4, b < B: the four EDM preconditioning scalars of one sigma (evaluated on the host in fp32) broadcast over the batch */
int buddy_fill_rows4(float* out, int B, float v0, float v1, float v2, float v3, void* stream);
/* per-row sum and sum of squares in double precision: out[b] = {sum, sumsq} */
int buddy_row_moments(const float* x, double* out, int B, int L, void* stream);
/* time-domain FIR (direct form) y[b][n] = sum_m h_b[m] x[b][n-m], n < L, h_b = h + b*h_stride (h_stride 0 = shared RIR):
 * replaces utils/reverb_utils.py:25-61 fast_apply_RIR (same linear convolution, no FFT); adjoint != 0 computes the
 * correlation (its transpose) for the VJP. */
int buddy_fir(const float* x, const float* h, long long h_stride, float* y, int B, int L, int M, int adjoint, void* stream);

/* ---- WPE warm start (`wpe_scaled`, testing/EulerHeunSamplerDPS.py:32-54 -> nara_wpe.wpe.wpe(Y, taps, delay, iterations,
 * statistics_mode='full'), single channel): Y, X are (rows, T) complex128 as interleaved doubles, one row per (utterance, frequency bin);
 * scratch: rows*T doubles.  Per row and iteration: inverse power, correlation matrix/vector, Cholesky solve, prediction filter. ---- */
int buddy_wpe(const double* Y, double* X, double* scratch, int rows, int T, int taps, int delay, int iterations, void* stream);
/* The whole warm-start estimate of testing/EulerHeunSamplerDPS.py:36-49 in one call: y (B, L) float32 -> out (B, L) float32 =
 * istft(wpe(stft(y)))[..., :L] with nara_wpe.utils.stft / istft conventions (size 512, shift 128, periodic Blackman window, fading,
 * bi-orthogonal synthesis window), every utterance on its own, complex128 inside.  workspace: buddy_wpe_workspace_bytes(B, L) bytes of
 * device memory.  The rescaling to scaling_factor / std (:51) and the noise (:52) stay with the caller. */
long long buddy_wpe_workspace_bytes(int B, int L);
int buddy_wpe_dereverb(const float* y, float* out, void* workspace, int B, int L, int taps, int delay, int iterations, void* stream);

/* ---- multichannel WPE (oracle/wpe_ref.py:91-120 for any channel count D; Nakatani et al. 2010, Drude et al. 2018, batch "full
 * statistics" form): the front end for microphone-array recordings and the WPE-alone baseline.  Y, X: (rows, D, T) complex128 as interleaved
 * doubles, one problem per row (= utterance x frequency bin); scratch: rows*T doubles.  Per problem and iteration, N = D*taps:
 * lambda_t = max(mean_d |x_dt|^2, 1e-10 max_t), R = sum_t yt yt^H / lambda_t (N x N), P = sum_t yt y_t^H / lambda_t (N x D), G = R^-1 P by
 * Cholesky, X = Y - G^H Yt; everything in double, fixed-order sums, a problem's bits independent of the other rows.  A pivot <= 0 (silent
 * channel or bin) gives a zero row of G.  Shapes: 1 <= D <= 8, taps >= 1, delay >= 0, iterations >= 0, D*taps <= 96 (R and P of one problem
 * stay in the LDS of a workgroup); anything else: BUDDY_ERR_ARG before any launch. ---- */
int buddy_wpe_mc(const double* Y, double* X, double* scratch, int rows, int D, int T, int taps, int delay, int iterations, void* stream);
/* y (B, D, L) float32 -> out (B, D, L) float32 = istft(wpe(stft(y))) with the transforms of buddy_wpe_dereverb (size 512, shift 128), every
 * item on its own, all D channels out.  workspace: buddy_wpe_mc_workspace_bytes(B, D, L) = B * 257 * T * (32 * D + 8) bytes with T the frame
 * count of the STFT for L samples: it grows linearly with D * L, the whole file goes in one call. */
long long buddy_wpe_mc_workspace_bytes(int B, int D, int L);
int buddy_wpe_mc_dereverb(const float* y, float* out, void* workspace, int B, int D, int L, int taps, int delay, int iterations, void* stream);

/* ---- wMPDR beamformer after multichannel WPE (weighted-power minimisation distortionless response; with the WPE weights reused the factorised
 * form of Nakatani & Kinoshita's convolutional beamformer, 2019/2020).  X: (rows, D, T) complex128 as interleaved doubles,
 * Z: (rows, T), one problem per row (= item x frequency bin); scratch: rows*T doubles.  Per problem: Phi = sum_t x x^H; its principal
 * eigenvector by TEN normalised squarings (A <- A / max|A_ij|, A <- A A, A <- (A + A^H) / 2), v = A[:, reference] / A[reference][reference];
 * then `iterations` times lambda_t = max(p_t, 1e-10 max_t p_t) with p_t = mean_d |x_dt|^2 first and |z_t|^2 afterwards,
 * R = sum_t x x^H / lambda_t + loading * tr(R) / D * I, u = R^-1 v by Cholesky, w = u / (v^H u), z_t = w^H x_t.  Pass-through z = x_reference
 * where Phi is zero, |v_r|^2 < 1e-12 |v|^2 (or v_r = 0), a pivot is <= 0 or v^H u is 0 or not finite; z = 0 where max_t p_t = 0; D = 1 copies.
 * Everything in double, fixed-order sums, a problem's bits independent of the other rows.  1 <= D <= 8, 0 <= reference < D, iterations >= 1,
 * loading >= 0 and finite, rows >= 1, T >= 1; anything else: BUDDY_ERR_ARG before any launch. ---- */
int buddy_mpdr(const double* X, double* Z, double* scratch, int rows, int D, int T, int reference, int iterations, double loading, void* stream);
/* y (B, D, L) float32 -> out (B, L) float32 = istft(mpdr(wpe(stft(y)))): the transforms and the WPE kernel of buddy_wpe_mc_dereverb (the same
 * bits), then the beamformer, one channel out.  workspace: buddy_wpe_mc_mpdr_workspace_bytes(B, D, L) = buddy_wpe_mc_workspace_bytes(B, D, L)
 * (the beamformer's output takes the place of the observed spectra, which are no longer needed by then). */
long long buddy_wpe_mc_mpdr_workspace_bytes(int B, int D, int L);
int buddy_wpe_mc_mpdr_dereverb(const float* y, float* out, void* workspace, int B, int D, int L, int taps, int delay, int wpe_iterations,
                               int reference, int bf_iterations, double loading, void* stream);

/* ---- blind subband-filtering reverb operator, batched over U utterances; replaces testing/operators/subband_filtering.py
 * (BlindSubbandFiltering :142-351 incl. SubbandFiltering :8-136), utils/reverb_utils.py:3-23, utils/losses.py:59-64 and the
 * torch.optim.Adam loop of EulerHeunSamplerDPS.optimize_op (testing/EulerHeunSamplerDPS.py:71-113) with hand-written
 * forward + analytic backward kernels.  STFT is fixed to NFFT 1024 / win 512 / hop 128 (op_hp of the conf/tester yaml files).
 * Tensor shapes follow the reference: decay/weights (U,E,bands), phases (U,513,Nf), H (U,513,Nf) complex64 interleaved. ---- */
int buddy_blindop_create(int U, int L, int Nf, int E, int num_knots, const float* knots_hz /*host*/, int sample_rate, float compression,
                         float min_decay, float max_decay, float w_lo, float w_hi, int clamp_decay, int long_second, void** handle);
int buddy_blindop_destroy(void* handle);
int buddy_blindop_set_params(void* handle, const float* decay, const float* weights, const float* phases, int reset_adam, void* stream);
int buddy_blindop_get_params(void* handle, float* decay, float* weights, float* phases, void* stream);
/* rows of one group share ONE parameter set (decay, weights, phases), one Adam state and hence one H.
 * group_of_row: host, U ints, group_of_row[0] == 0, non-decreasing, steps of 0 or 1 (groups are contiguous row ranges).
 * NULL = every row its own group (the state after create).  Anything else: BUDDY_ERR_ARG, nothing changed.
 * The leader of a group is its first row.  This call and every later buddy_blindop_set_params copy the leader's decay, weights, phases and
 * the six Adam moment arrays to the members; buddy_blindop_update_H(noise != NULL) reads the leader's noise row for every member.  In
 * param_grads / optimize every row runs its own forward and backward chain (own x_den, y and regulariser noise row); the phase and knot
 * gradients of the members are then replaced by their mean (summed in ascending row order in float32, times 1.0f / n, the same bits stored
 * to every member) before Adam, so members receive equal updates and stay bit-for-bit equal without any copy.  The mean, not the sum: the
 * balance between w_rec and w_reg stays that of a single row.  Losses, the likelihood entries and everything else stay per row.  Only
 * parameters and moments are copied: the members' H is that of their OLD parameters until the next buddy_blindop_update_H (optimize and
 * param_grads rebuild H themselves).  update_H_vjp stays per row (no mean): tied fitting goes through param_grads / optimize.  Drops the
 * captured optimize graph.  With no group of more than one row, every call launches exactly what it launches without this entry. */
int buddy_blindop_set_groups(void* handle, const int* group_of_row /*host*/, void* stream);
/* update_H (:253-285): H = cons(A exp(j phases)); noise != NULL (U, 128*Nf samples) = use_noise=True (phases := angle(H)). */
int buddy_blindop_update_H(void* handle, const float* noise, void* stream);
int buddy_blindop_get_H(void* handle, float* H_out, void* stream);
int buddy_blindop_set_y(void* handle, const float* y /*(U,L)*/, void* stream);            /* caches comp(STFT(y)) for the losses */
int buddy_blindop_degrade(void* handle, const float* x, float* y, void* stream);           /* degradation (:82-101) with the current H */
int buddy_blindop_time_rir(void* handle, float* rir /*(U, 128*Nf+1024)*/, void* stream);   /* get_time_RIR (:103-113) */
/* per-function views (what optimize_op / the likelihood run internally), used by the parity tests against reference fixtures:
 * design_filter (subband_filtering.py:241-251) -> A (U,513,Nf); apply_stft (:41-52) of x (U,L) -> (U,513,T,2), T = 1+(L+512)/128;
 * minimum_phase_version (utils/reverb_utils.py:9-23) of h (U, 128*(Nf+1)); project_params (:298-331) on the current decay/weights;
 * Adam moments (torch.optim.Adam exp_avg / exp_avg_sq; any pointer may be NULL) and the step count. */
int buddy_blindop_design_filter(void* handle, float* A, void* stream);
int buddy_blindop_apply_stft(void* handle, const float* x, float* X, void* stream);
int buddy_blindop_minphase(void* handle, const float* h, float* out, void* stream);
/* ---- the differentiable surface (round 6): vector-Jacobian products of the pieces the REFERENCE's own sampler autograds through -- operator.degradation
 * in get_likelihood_score (testing/EulerHeunSamplerDPS.py:61-69), update_H / degradation / get_time_RIR in optimize_op (:71-113), apply_stft inside
 * get_loss(...)(y, y_hat) (utils/losses.py:26-71).  buddy_amd/testing/operators wraps each as a torch.autograd.Function, so an unmodified torch-loop
 * sampler (oracle/sampler_ref.py = the reference's control flow) runs on the HIP operator.  H-shaped gradients are (U, 513, Nf, 2) = (d/dRe, d/dIm). */
/* degradation^T for the CURRENT H: g_x (U, L) and / or g_H from g_y (U, L); x (U, L) is needed for g_H only; either output may be NULL (not both) */
int buddy_blindop_degrade_vjp(void* handle, const float* x, const float* g_y, float* g_x, float* g_H, void* stream);
int buddy_blindop_time_rir_vjp(void* handle, const float* g_rir /*(U, 128*Nf+1024)*/, float* g_H, void* stream);      /* get_time_RIR^T */
/* update_H^T (H = cons(design_filter(decay, weights) exp(j phases)), subband_filtering.py:253-285): gradients of the three parameter tensors in the
 * reference layouts from g_H, using the state the LAST buddy_blindop_update_H left in the handle; any output may be NULL */
int buddy_blindop_update_H_vjp(void* handle, const float* g_H, float* g_decay, float* g_weights, float* g_phases, void* stream);
/* apply_stft (:41-52) of signals of the bound length L (T = 1 + (L + 512) / 128 frames) or of the time-RIR length 128 * Nf + 1024, X (U, 513, frames, 2),
 * and its adjoint g_x (U, len) from G (U, 513, frames, 2); other lengths are BUDDY_ERR_ARG */
int buddy_blindop_stft(void* handle, const float* x, int len, float* X, void* stream);
int buddy_blindop_stft_adjoint(void* handle, const float* G, int len, float* g_x, void* stream);
/* loss[u] = weight * l2_comp_stft_summean(a_u, b_u) (utils/losses.py:59-64) for two signals of length len (as above) with the gradient w.r.t. either
 * argument (g_a / g_b (U, len), NULL = not wanted) */
int buddy_blindop_stft_loss(void* handle, const float* a, const float* b, int len, float weight, float* loss, float* g_a, float* g_b, void* stream);
/* compression exponent of the spectral losses, (0, 1] (the handle is created with one; the shipped configs use 0.667); call buddy_blindop_set_y again
 * afterwards: the cached compressed observation depends on it */
int buddy_blindop_set_compression(void* handle, float compression_factor);
/* which member of the reference's compressed-spectrum family every loss entry of the handle evaluates (utils/losses.py:46-64):
 * 0 = l2_comp_stft_summean (default, the shipped configs), 1 = l2_comp_stft_sum, 2 = l2_comp_stft_mean */
int buddy_blindop_set_loss_norm(void* handle, int mode);
/* which loss each term of the handle evaluates (utils/losses.py:26-93), one descriptor per slot.  set_compression / set_loss_norm above set all slots.
 *   slot  0 likelihood (rec_loss_grad, fir_loss_grad)     1 operator fit (rec_loss_params; param_grads, optimize)
 *         2 RIR-noise regulariser (param_grads, optimize)  3 the callable buddy_blindop_stft_loss
 *   kind  0 l2_comp_stft_summean  1 l2_comp_stft_sum  2 l2_comp_stft_mean  3 l2_stft_sum  4 l2_stft_mag_sum  5 l2_stft_logmag_sum
 *         6 l2_log_stft_sum  7 l2_sum  8 l2_mean (time domain: on the signals themselves)  9 none (slot 1 only: the term is dropped)
 *   freq_weighting  0 none  1 sqrt  2 exp  3 log  4 linear (STFT kinds only; the table must have been uploaded with set_freq_weights)
 *   compression     (0, 1], read by kinds 0..2 only
 * Kinds 0..2 without weighting run the same kernels as before this entry existed.  Changing slot 0 or 1 requires buddy_blindop_set_y again (the cached
 * targets phi(w_f STFT(y)) / y depend on them); changing slots 0..2 drops the captured optimize graph.  Invalid arguments: BUDDY_ERR_ARG. */
int buddy_blindop_set_loss(void* handle, int slot, int kind, int freq_weighting, float compression);
/* per-bin weight table w[513] (host memory, float32) of freq_weighting 1..4: the reference's get_frequency_weighting(linspace(0, 1, 513) + 1);
 * copied into the handle (synchronously) and kept */
int buddy_blindop_set_freq_weights(void* handle, int freq_weighting, const float* w);
int buddy_blindop_lengths(void* handle, int* L, int* L_rir, int* frames, int* frames_rir);
int buddy_blindop_project(void* handle, void* stream);
int buddy_blindop_get_adam(void* handle, float* m_decay, float* v_decay, float* m_weights, float* v_weights, float* m_phases, float* v_phases,
                           int* step /*host*/, void* stream);
/* loss[u] = weight * l2_comp_stft_summean(y_u, degrade(x_den_u)); g_x = d sum_u loss / d x_den (NULL to skip) */
int buddy_blindop_rec_loss_grad(void* handle, const float* x_den, float weight, float* loss, float* g_x, void* stream);
/* informed counterpart (RIROperator, testing/operators/reverb.py:33-35 + utils/losses.py:59-64): degradation = time-domain FIR with the
 * known RIR(s) rir[u * rir_stride + m], m < M (fast_apply_RIR semantics: first L output samples); same loss, same cached y (set_y). */
int buddy_blindop_fir_loss_grad(void* handle, const float* x_den, const float* rir, long long rir_stride, int M, float weight, float* loss,
                                float* g_x, void* stream);
/* one gradient evaluation of optimize_op's objective (H rebuilt from the parameters first); losses = [rec (U), reg (U)].
 * With groups set (buddy_blindop_set_groups) every member row of a group holds the group-MEAN gradients; the losses stay per row. */
int buddy_blindop_param_grads(void* handle, const float* x_den, const float* noise, float t_op, float w_rec, float w_reg, float* g_decay,
                              float* g_weights, float* g_phases, float* losses, void* stream);
/* n_iters iterations of optimize_op: update_H, rec + RIR-noise losses, backward, Adam on [decay, weights, phases], projection.
 * noise: (n_iters, U, 128*Nf+1024) N(0,1) draws (NULL = no regulariser) */
int buddy_blindop_optimize(void* handle, const float* x_den, const float* noise, float t_op, int n_iters, float w_rec, float w_reg, float lr,
                           float beta1, float beta2, float weight_decay, void* stream);

/* ---- any-rate input: batched rational polyphase resampler (buddy_amd/utils/resample.py; the reference's loaders assert samplerate == fs and
 * have no resampler).  x (B, Lin), h: odd-length symmetric FIR of Nh taps with centre c = (Nh-1)/2 and DC gain `up`, y (B, Lout):
 *
 *   y[b][n] = sum over m in [0, Lin) with 0 <= n*down - m*up + c < Nh  of  x[b][m] * h[n*down - m*up + c],   n in [0, Lout),
 *   Lout = ceil(Lin * up / down)
 *
 * i.e. zero-stuffing by `up`, filtering with h, keeping every `down`-th sample, zero extension at both ends (scipy.signal.resample_poly
 * with window = h / up and padtype = 'constant').  fp32 accumulation in ascending m; nothing is written outside y[b][0 .. Lout-1].
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer; B < 1 or Lin < 1; up or down outside 1..1024; gcd(up, down) != 1; Nh even or
 * above 65 537; Lout != ceil(Lin * up / down); Lin above 2^40 or more than 2^31 - 1 tiles of 1024 outputs over all rows. */
int buddy_resample(const float* x, int B, long long Lin, const float* h, int Nh, int up, int down, float* y, long long Lout, void* stream);

/* ---- room-acoustic analysis of room impulse responses (buddy_amd/utils/acoustics.py; the reference writes its RIR estimates
 * to wav files and analyses nothing).  RIR rows h (B, <= ldh) are ragged inside a common stride: lens[b] samples of row b are valid, nothing is
 * read past h[b][lens[b] - 1].  lens, lens_g and n0 are DEVICE arrays of int32; every entry copies its length array to the host once (after the
 * work queued on `stream`) to check it.  BUDDY_ERR_ARG, with nothing launched, for: a null pointer (edc_db may be NULL); B or nb outside
 * 1..65535; Nh even or above 65 537; a length below 1 or above 2^30; a stride smaller than the longest row it holds; fs < 1.
 *
 * buddy_row_argmax_abs: n0[b] = the FIRST index of max |h[b][n]|, n < lens[b] (fp32 compare): the direct path of a peak-aligned RIR.
 *
 * buddy_fir_bank: zero-phase band signals g (B, nb, ldg) of a bank (nb, Nh) of odd-length FIR rows sharing one Nh, centre P = (Nh - 1) / 2:
 *   g[b][k][n] = sum_j bank[k][j] * h[b][n - j + P],   n in [0, lens[b] + P),   zero extension
 * (the tail of P samples past the end of h is kept, the pre-ringing before index 0 is dropped).  fp32 accumulation in ascending input index;
 * zero taps are skipped, so a unit impulse at j = P copies h bit for bit.  ldg >= max lens[b] + P; nothing is written past g[b][k][lens[b] + P - 1].
 *
 * buddy_decay_metrics: per (row, band) of g with lens_g[b] (= lens[b] + P) valid samples and the row's direct-path index n0[b] (clamped to the
 * row): w = round(0.0025 fs) = (fs + 200) / 400, analysis start ns = max(n0 - w, 0), t = (n - ns) / fs; Schroeder curve
 * D[n] = 10 log10(sum_{m >= n} g[m]^2 / sum_{m >= ns} g[m]^2), n >= ns; least-squares lines D ~ a + s t over the samples with lo <= D[n] <= hi.
 *   out (B, nb, 6) doubles: EDT (0..-10 dB), T20 (-5..-25), T30 (-5..-35), each -60 / s [s]; C50 [dB], split at ns + round(0.05 fs) = ns + (fs + 10) / 20;
 *     DRR [dB], direct part ns <= n <= n0 + w; centre time Ts [s].  NaN where undefined: fewer than two samples in a range or s >= 0, a zero
 *     denominator, an all-zero row (every value NaN, which disturbs no other row).
 *   flags (B, nb) int32: bit q (0..5) = out[..][q] is defined; bit 6 + q (q = 0..2) = the fit of decay time q is VALID: the decay left between
 *     its last fitted sample n_hi and the end of the row at the fitted slope, |s| (lens_g[b] - 1 - n_hi) / fs, is at least 10 dB (a truncated
 *     response bends the curve down by 10 log10(1 - 10^(-R/10)) dB, below 0.5 dB for R >= 9.6 dB).  The value is written either way.
 *   edc_db (B, nb, ldg) fp32 or NULL: D[n] for ns <= n < lens_g[b], NaN for n < ns, untouched from lens_g[b] on.
 * One workgroup per (row, band); every sum in double; no atomics, no workspace.  buddy_decay_tile: samples per tile of its backward sweep (the
 * lengths around which the unit tests place their rows). */
int buddy_row_argmax_abs(const float* h, const int* lens, int B, long long ldh, int* n0, void* stream);
int buddy_fir_bank(const float* h, const int* lens, int B, long long ldh, const float* bank, int nb, int Nh, float* g, long long ldg, void* stream);
int buddy_decay_metrics(const float* g, const int* lens_g, const int* n0, int B, int nb, long long ldg, int fs, double* out, int* flags, float* edc_db,
                        void* stream);
int buddy_decay_tile(void);

/* ---- objective evaluation of a paired run (buddy_amd/utils/metrics.py; the reference writes its wavs and scores nothing):
 * SI-SDR, STOI, ESTOI and the log-spectral distance of pairs (estimate e, clean reference x).  Rows are ragged inside a common stride: lens[b]
 * samples of row b are valid, nothing behind them is read, nothing outside the declared extents is written.  Every lengths array is a DEVICE array
 * of B ints; each entry copies it to the host once (after the work queued on `stream`) to check it.  Every reduction has a fixed order (no
 * atomics), and a row's result does not depend on the other rows.  Frames are 256 samples at hop 128 under the window
 * w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), all FULL frames: frames(len) = (len - 256) / 128 + 1 for len >= 256, else 0; the transform has 512 points.
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer; B outside 1..65535; a length outside 1..2^30 (0..2^30 for the frame counts of buddy_stoi_scores and the rebuilt rows of buddy_band_spectra); a stride
 * smaller than the longest row it holds; J outside 1..32 or a band outside the bins 0..257; a workspace below the size stated.
 *
 * buddy_pair_moments: out (B, 4) doubles = zero-mean ||e||^2, ||x||^2, <e,x>, and SI-SDR [dB] = 10 log10(||a x||^2 / max(||a x - e||^2, 1e-30)) with
 *   a = <e,x> / max(||x||^2, 1e-30), both means removed; every sum in double, the two energies element by element.  flags[b] = 1 unless
 *   ||x||^2 = 0 or lens[b] < 2 (the value is the clamped formula's either way).  buddy_metrics_tile: samples per step of its reductions (the
 *   lengths around which the unit tests place their rows).
 *
 * buddy_stoi_select: silent-frame removal at 10 kHz, decided on the clean rows x alone.  E[f] = 20 log10(||w x_f||_2 + 2^-52) in double; frame f is
 *   kept when E[f] > max_f E - 40; F[b] = frames(lens[b]), K[b] kept frames, src (B, ldf): src[b][j] = the frame that became kept frame j (j < K[b],
 *   ascending; the rest of the row is untouched).  xo, eo (B, ldo): both signals rebuilt by overlap-adding their kept windowed frames at hop 128,
 *   lens_out[b] = (K[b] - 1) 128 + 256 samples (0 for K[b] = 0); each sample is w x of the earlier covering frame plus w x of the later one, fp32.
 *   ldf >= max(frames of the longest row, 1); ldo >= its full-frame extent; ws: 8 B ldf bytes (buddy_stoi_select_workspace(B, longest row) for
 *   ldf = its frames).
 *
 * buddy_band_spectra: out (B, J, ldm) fp32, out[b][j][m] = sqrt(sum_{lo[j] <= k < hi[j]} |X[k, m]|^2) of frame m < frames(lens[b]), X the 512-point
 *   transform (fp32, radix 2) of the windowed, zero-padded frame; the band sums in double.  lo, hi: HOST arrays of J ints.  ldm >= max(frames, 1).
 *
 * buddy_stoi_scores: X, Y (B, J, ldm) band spectra of the clean and the estimated rows with lens_m[b] frames.  One segment per run of 30
 *   consecutive frames, S = lens_m[b] - 29.  out (B, 2) doubles = STOI (scale to the clean row's norm, clip at x (1 + 10^(15/20)), correlation of the
 *   mean-removed rows, / (J S)) and ESTOI (rows, then columns, mean-removed and normalised; sum of products / (30 S)); every norm + 2^-52; all in
 *   double.  S < 1: NaN and flags[b] = 0, else flags[b] = 1.  ws: buddy_stoi_scores_workspace(B, longest frame count) bytes.
 *
 * buddy_frame_power: mean_p[b] = mean over frames m and bins k = 0..256 of |X[k, m]|^2, by Parseval from the windowed frames in double (NaN without a
 *   full frame).  buddy_lsd: out[b] = mean_m sqrt(mean_{k = 0..256} (10 log10((P + d) / (Q + d)))^2) with P = |X|^2, Q = gain[b]^2 |E|^2, d = delta[b]
 *   (device doubles), means in double.  No full frame, or delta[b] not above zero: NaN and flags[b] = 0.  ws of both: buddy_lsd_workspace(B, longest row). */
int buddy_metrics_tile(void);
int buddy_pair_moments(const float* e, const float* x, const int* lens, int B, long long ld, double* out, int* flags, void* stream);
long long buddy_stoi_select_workspace(int B, long long max_len);
int buddy_stoi_select(const float* x, const float* e, const int* lens, int B, long long ld, float* xo, float* eo, long long ldo, int* lens_out, int* K, int* F,
                      int* src, long long ldf, void* ws, long long ws_bytes, void* stream);
int buddy_band_spectra(const float* x, const int* lens, int B, long long ld, const int* lo /*host*/, const int* hi /*host*/, int J, float* out, long long ldm,
                       void* stream);
long long buddy_stoi_scores_workspace(int B, int max_frames);
int buddy_stoi_scores(const float* X, const float* Y, const int* lens_m, int B, int J, long long ldm, double* out, int* flags, void* ws, long long ws_bytes,
                      void* stream);
long long buddy_lsd_workspace(int B, long long max_len);
int buddy_frame_power(const float* x, const int* lens, int B, long long ld, double* mean_p, void* ws, long long ws_bytes, void* stream);
int buddy_lsd(const float* e, const float* x, const int* lens, int B, long long ld, const double* gain, const double* delta, double* out, int* flags, void* ws,
              long long ws_bytes, void* stream);

/* ---- time alignment of a pair before it is scored (buddy_amd/utils/metrics.py align; no reference counterpart): one integer lag
 * per pair (estimate e, clean reference x) from a windowed cross-correlation, and the pair trimmed to its overlap.  The conventions of the evaluation
 * entries above hold: ragged rows inside a common stride, DEVICE length (and lag) arrays copied to the host once to be checked, nothing behind
 * lens[b] - 1 read, nothing outside the declared extents written, fixed-order sums without atomics, a row's result independent of its batch.
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer (r_out may be NULL); B outside 1..65535; a length outside 1..2^30; a stride smaller than the
 * longest row it holds; K outside 0..65535; a workspace below the size stated; a lag with |lag[b]| >= lens[b].
 *
 * buddy_xcorr_lag: for row b with n = lens[b]: e~ = e - mean(e), x~ = x - mean(x) in double; r[k] = sum_m e~[m + k] x~[m] over the m with 0 <= m < n and
 *   0 <= m + k < n (zero where there is none), k = -K..K, every product and sum in double: a direct correlation, no FFT, so
 *   |r[k] - exact| <= about (n + 4) 2^-53 sum_m |e~[m + k]| |x~[m]|.  A positive k means the estimate is late.  d = the k of the largest |r[k]|; ties go to the
 *   smallest |k|, then to k >= 0.  lag[b] = d; out (B, 2) doubles = (rho, frac): rho = r[d] / sqrt(||e~||^2 ||x~||^2), signed; frac = 0.5 (a - c) / (a - 2 b + c)
 *   with a, b, c = |r[d - 1]|, |r[d]|, |r[d + 1]| where |d| < K and the denominator is negative, else 0 (the vertex of the parabola through the three
 *   points: reported, never applied).  flags[b]: bit 0 = defined (n >= 2, both energies > 0, every input finite; else d = 0, rho = NaN, frac = 0); bit 1 = the
 *   peak lies on the edge of the window (|d| = K, K > 0); bit 2 = rho < 0 (inverted polarity).  r_out: (B, 2K + 1) doubles, r_out[b][k + K] = r[k], or NULL
 *   (there for the unit tests; for a row that is not defined it holds whatever the sums gave).  K >= n is allowed (those lags have r = 0).
 *   ws: buddy_xcorr_lag_workspace(B, longest row, K) bytes (-1 for arguments out of range).  Work: n (2K + 1) multiply-adds per row.
 *   buddy_align_tile: samples per chunk, buddy_align_lag_tile: lags per tile of the correlation kernel (the sizes around which the unit tests place
 *   their rows and windows).
 *
 * buddy_align_pair: lens_out[b] = lens[b] - |d|, d = lag[b] (DEVICE ints); eo[b][m] = e[b][m + max(d, 0)], xo[b][m] = x[b][m + max(-d, 0)] for m < lens_out[b],
 *   zeros from there to ldo - 1.  eo, xo: (B, ldo), ldo >= the longest overlap. */
int buddy_align_tile(void);
int buddy_align_lag_tile(void);
long long buddy_xcorr_lag_workspace(int B, long long max_len, int K);
int buddy_xcorr_lag(const float* e, const float* x, const int* lens, int B, long long ld, int K, int* lag, double* out, int* flags, double* r_out, void* ws,
                    long long ws_bytes, void* stream);
int buddy_align_pair(const float* e, const float* x, const int* lens, const int* lag, int B, long long ld, float* eo, float* xo, long long ldo, int* lens_out,
                     void* stream);

/* ---- projection SDR of a pair over filter lengths (buddy_amd/utils/sdr.py; no reference counterpart): the BSS-Eval SDR of one
 * source (Vincent et al. 2006) -- the estimate e projected onto the clean signal x and its delayed copies 0..m - 1 -- at up to 8 filter lengths m from
 * one Levinson recursion.  The conventions of the evaluation entries above hold: ragged rows inside a common stride, DEVICE length arrays copied to the
 * host once to be checked, nothing behind lens[b] - 1 read, nothing outside the declared extents written, fixed-order sums without atomics, a row's
 * result independent of its batch.  BUDDY_ERR_ARG, with nothing launched, for: a null pointer (h may be NULL); B outside 1..65535; a length outside
 * 1..2^30; a stride smaller than the longest row it holds; N outside 1..2048; J outside 1..8 or orders not strictly ascending within 1..N; a loading
 * that is negative or not finite; a workspace below the size stated.
 *
 * buddy_sdr_products: for row b with n = lens[b], k = 0..N - 1: r[b][k] = sum_{t = 0}^{n - 1 - k} x[t] x[t + k], d[b][k] = sum_{t = 0}^{n - 1 - k} e[t + k] x[t]
 *   (zero where there is no term: n < N is allowed), ee[b] = sum_t e[t]^2.  No means are removed.  r, d: (B, N) doubles, ee: (B) doubles.  Every product
 *   and sum in double on the exact fp32 inputs: a direct correlation, no FFT, so |r[k] - exact| <= about (n + 4) 2^-53 sum_t |x[t]| |x[t + k]|, and the
 *   same for d and ee with their own factors.  ws: buddy_sdr_products_workspace(B, longest row, N) bytes (-1 for arguments out of range).  Work:
 *   2 n N multiply-adds per row.  buddy_sdr_tile: samples per chunk, buddy_sdr_lag_tile: lags per tile of the kernel (the sizes around which the unit
 *   tests place their rows and orders).
 *
 * buddy_sdr_solve: r, d (B, N) and ee (B) DEVICE doubles as above, lens (B) DEVICE ints (only n >= 2 is taken from them), orders: J HOST ints, strictly
 *   ascending within 1..N.  R_m = the m x m symmetric Toeplitz matrix of r with r[0] replaced by r[0] (1 + loading); h_m = R_m^-1 d[0..m - 1] by the
 *   symmetric Levinson recursion from f = (1 / R[0][0]), h = (d[0] / R[0][0]): at step n = 1..N - 1, eps_f = sum_{i < n} r[n - i] f[i],
 *   eps_x = sum_{i < n} r[n - i] h[i], f <- (f (+) 0 - eps_f rev(f (+) 0)) / (1 - eps_f^2), h <- h (+) 0 + (d[n] - eps_x) rev(f).  For each order m asked:
 *   p[b][j] = p_m = sum_{i < m} h_m[i] d[i], the energy of the projection, and sdr[b][j] = 10 log10(p_m / max(ee - p_m, 1e-12 ee)).  sdr, p: (B, J) doubles.
 *   flags[b]: bit 0 = defined (n >= 2, r[0] > 0, ee > 0, both finite, every pivot 1 - eps_f^2 > 0, every p_m > 0; else every sdr and p of the row is NaN
 *   and h is zeros); bit 1 = ee - p_m < 4 loading ee at some order asked (the ceiling the loading sets: e = x reads about -10 log10(loading) dB);
 *   bit 2 = a pivot fell below 2^-26 (h is ill-determined; the values are reported all the same).  h: (B, N) doubles, the filter of order N, or NULL.
 *   One workgroup per row and N dependent steps: latency-bound by construction. */
int buddy_sdr_tile(void);
int buddy_sdr_lag_tile(void);
long long buddy_sdr_products_workspace(int B, long long max_len, int N);
int buddy_sdr_products(const float* e, const float* x, const int* lens, int B, long long ld, int N, double* r, double* d, double* ee, void* ws, long long ws_bytes,
                       void* stream);
int buddy_sdr_solve(const double* r, const double* d, const double* ee, const int* lens, int B, int N, const int* orders, int J, double loading, double* sdr,
                    double* p, int* flags, double* h, void* stream);

/* ---- non-intrusive score of single signals (buddy_amd/utils/srmr.py): the speech-to-reverberation modulation energy ratio.
 * The conventions of the evaluation entries above hold: ragged rows inside a common stride, DEVICE length arrays copied to the host once to be checked,
 * nothing behind lens[b] read, nothing outside the declared extents written, fixed-order sums without atomics, a row's result independent of its batch.
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer; B outside 1..65535; a length outside 1..2^30 (0..2^30 for the frame counts of
 * buddy_srmr_scores); a stride smaller than the longest row it holds; J outside 1..32; the limits named per entry.
 *
 * buddy_gammatone_env: env (B, J, lde) fp32, env[b][j][n] = |sum_{t < N_j} g_j[t] x[b][n - t]| for n < lens[b], x zero before the row's start; nothing is
 *   written at or behind lens[b].  g_re, g_im: the taps of all channels one behind the other (device, fp32); tap_off: HOST array of J + 1 ints, channel j
 *   is the taps tap_off[j] .. tap_off[j + 1] - 1, 1..1536 of them.  Order of the fp32 arithmetic, the same for every output: real and imaginary sum start
 *   at zero and take one fused multiply-add per tap, t ascending; the magnitude is sqrt(fma(re, re, im * im)).  The grid runs the channels by descending
 *   tap count.  buddy_srmr_tile: outputs per workgroup (the lengths around which the unit tests place their rows).
 *
 * buddy_modulation_energies: K <= 8 second-order filters (coef: HOST array (K, 6) doubles b0 b1 b2 a0 a1 a2 with a0 = 1; direct form II transposed, zero
 *   initial state, double) run along each envelope row env (B, J, lde) with lens[b] samples; E (B, J, K, ldm) doubles,
 *   E[b][j][k][m] = sum_{i < W} (h[i] v_jk[m H + i])^2 for the full frames m < frames[b] = (lens[b] - W) / H + 1 (0 below W), h[i] = 0.54 - 0.46 cos(2 pi
 *   (i + 1) / (W + 1)); the filtered signals v are not stored.  W = 4 H, H a multiple of buddy_modulation_chunk() = 256, W <= 4096.  ldm >= max(frames, 1).
 *
 * buddy_srmr_scores: Ebar (B, J, 8) doubles = mean over the frames of E (NaN without a frame); A[j] = sum_k Ebar[j][k]; the channels are visited in index
 *   order, which the caller makes the order of ascending centre frequency: BW = erb[j] of the first j whose running sum of A is strictly above 0.9 sum_j A[j];
 *   K* = 5 + #{k in 5..7: BW >= l[k]}; out (B, 3) doubles = (sum_j sum_{k < 4} Ebar / sum_j sum_{4 <= k < K*} Ebar, K*, BW).  erb (J), l (8): HOST doubles.
 *   flags[b] = 1 where the ratio is defined.  No frame or no energy: three NaN and flag 0; a zero denominator: NaN, K*, BW and flag 0.  K must be 8.
 *   One workgroup per row. */
int buddy_srmr_tile(void);
int buddy_modulation_chunk(void);
int buddy_gammatone_env(const float* x, const int* lens, int B, long long ld, const float* g_re, const float* g_im, const int* tap_off /*host*/, int J, float* env,
                        long long lde, void* stream);
int buddy_modulation_energies(const float* env, const int* lens, int B, int J, long long lde, const double* coef /*host*/, int K, int W, int H, double* E,
                              long long ldm, int* frames, void* stream);
int buddy_srmr_scores(const double* E, const int* frames, int B, int J, int K, long long ldm, const double* erb /*host*/, const double* l /*host*/, double* out,
                      double* Ebar, int* flags, void* stream);

/* ---- blind decay time of single signals (buddy_amd/utils/decay.py, csrc/decay.hip; no reference counterpart): the decay time,
 * extrapolated to 60 dB, of a signal's own free decays after speech offsets, per band.  The conventions of the evaluation entries above hold: ragged rows
 * inside a common stride, DEVICE length and frame-count arrays copied to the host once to be checked, nothing behind a row's end read, nothing outside the
 * declared extents written, fixed-order double sums without floating-point atomics, a row's bits independent of its batch.  The analysis is defined at
 * 16 kHz: frames of 512 samples at hop 128.
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer; B outside 1..65535; a length outside 1..2^30 (0..2^30 for frame counts); a stride smaller
 * than the longest row it holds; NB outside 1..8; the limits named per entry.
 *
 * buddy_decay_energies: frames[b] = M = (lens[b] - 512) / 128 + 1 full frames (0 below 512 samples); E (B, NB, ldm) doubles, E[b][i][m] = sum over the bins
 *   lo_bins[i] <= k < hi_bins[i], ascending in one double accumulator, of |X[k]|^2, X the 512-point transform (fp32, radix 2, the transform and window of
 *   buddy_frame_spectra) of frame m < M; the squares are taken in double.  lo_bins, hi_bins: HOST arrays of NB ints, 0 <= lo <= hi <= 257 (lo = hi: an
 *   empty band, E = 0).  ldm >= max(frames, 1).  Four frames per workgroup; entries m >= M are not written.
 *
 * buddy_decay_regions: S[m] = (((E[m] + E[m+1]) + E[m+2]) + ...) + E[m+K-1] for m <= M - K; floor = floor_rel * max_m S[m]; frame m steps down when
 *   S[m+1] < S[m] and S[m+1] > floor.  A region is a maximal run of steps at frames m0 .. m1 - 1; it spans the m1 - m0 + 1 values S[m0] .. S[m1] and is
 *   kept when that number is >= lmin, S[m0] > floor and S[m1] <= S[m0] * q (doubles compared, no logarithm).  Its slope is the least-squares fit of
 *   d[j] = 10 log10(S[m0+j] / S[m0]) against j = 0 .. m1 - m0, the sums in double in ascending j, no product fused into a sum; its value is
 *   -60 / slope * 128 / 16000 seconds (dropped should the slope not be negative).  T, len (B, NB, ldm): T[b][i][m0] = the value and len[b][i][m0] =
 *   m1 - m0 + 1 where a kept region starts, NaN and 0 at every other frame m < M; nothing at m >= M.  K in 1..8, lmin >= 2, 0 < q <= 1,
 *   0 <= floor_rel < 1.  buddy_decay_regions_tile: the frames per LDS tile of the walk (the frame counts around which the unit tests place their
 *   rows; buddy_decay_tile above belongs to buddy_decay_metrics).
 *
 * buddy_decay_select: counts (B, NB) ints = n, the entries of T[b][i][0 .. frames[b] - 1] that are not NaN; out (B, NB, 3) doubles = their order statistics
 *   of rank (n - 1) / 2, (n - 1) / 4 and 3 (n - 1) / 4 (integer divisions; 0-based, ascending): the lower median and the quartiles, by an exact radix
 *   select; three NaN where n = 0.  B * NB workgroups per rank. */
int buddy_decay_regions_tile(void);
int buddy_decay_energies(const float* x, const int* lens, int B, long long ld, const int* lo_bins /*host*/, const int* hi_bins /*host*/, int NB, double* E,
                         long long ldm, int* frames, void* stream);
int buddy_decay_regions(const double* E, const int* frames, int B, int NB, long long ldm, int K, int lmin, double q, double floor_rel, double* T, int* len,
                        void* stream);
int buddy_decay_select(const double* T, const int* frames, int B, int NB, long long ldm, double* out, int* counts, void* stream);

/* ---- active speech level of single signals (buddy_amd/utils/level.py; ITU-T P.56 method B as restated there; no reference
 * counterpart).  The conventions of the evaluation entries above hold: ragged rows inside a common stride, DEVICE length arrays copied to the host once
 * to be checked, nothing at or behind lengths[b] read or written, fixed-order sums without atomics, a row's result independent of B, of the grid and of
 * the run.  A length may be 0 (the row then gives sq = 0 and zero counts).
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer (offset may be NULL: zeros); B outside 1..65535; a length outside 0..2^30; a stride smaller
 * than the longest row (or below 1); fs or tc not finite and above zero; I < 0; a ref[b] that is not finite and positive or an offset[b] that is not
 * finite; a workspace below the size its query states (the queries give -1 for B outside 1..65535 or max_len outside 0..2^30).
 *
 * buddy_level_stats: out (B, 2) doubles = (sum of x[b][i], max |x[b][i]|), i < lengths[b]; the sum in double in a fixed order (a NaN sample gives a NaN
 *   sum; the maximum skips it).
 *
 * buddy_level_classes: offset, ref: DEVICE doubles (B), copied to the host once to be checked.  With o = offset[b], R = ref[b], g = exp(-1 / (fs tc))
 *   (formed once, on the host), v_i = |x_i - o| in double: p_i = g p_(i-1) + (1 - g) v_i, q_i = g q_(i-1) + (1 - g) p_i from p = q = 0, all in double;
 *   klass[b][i] = #{j in 0..15 : q_i >= R 2^(j - 15)} for i < lengths[b]; sq[b] = sum_i (x_i - o)^2 in double in a fixed order.  The recurrence runs
 *   as a scan over tiles of buddy_level_tile() samples; q differs from the sequential evaluation by no more than the bound of section 23.  A sample
 *   that is not finite makes sq[b] not finite and the row's classes meaningless, and disturbs no other row.
 *
 * buddy_level_counts: counts (B, 16) int64, counts[b][j] = #{i < lengths[b] : some i' in [max(0, i - I), i] has klass[b][i'] >= j + 1}: the P.56
 *   hangover of I samples.  Integer arithmetic throughout; any I >= 0.  buddy_level_counts_tile(): samples per workgroup.
 * buddy_level_tile / buddy_level_counts_tile: the sizes around which the unit tests place their rows. */
int buddy_level_tile(void);
int buddy_level_counts_tile(void);
long long buddy_level_stats_workspace(int B, long long max_len);
long long buddy_level_classes_workspace(int B, long long max_len);
long long buddy_level_counts_workspace(int B, long long max_len);
int buddy_level_stats(const float* x, long long ldx, const int* lengths, int B, double* out, void* ws, long long ws_bytes, void* stream);
int buddy_level_classes(const float* x, long long ldx, const int* lengths, const double* offset /* NULL: zeros */, const double* ref, int B, double fs, double tc,
                        unsigned char* klass, long long ldk, double* sq, void* ws, long long ws_bytes, void* stream);
int buddy_level_counts(const unsigned char* klass, long long ldk, const int* lengths, int B, int I, long long* counts /* (B, 16) */, void* ws, long long ws_bytes,
                       void* stream);

/* ---- spectral-envelope distortion of a paired run (buddy_amd/utils/spectral.py; no reference counterpart): cepstral distance,
 * log-likelihood ratio and frequency-weighted segmental SNR of pairs (estimate e, clean reference x).  The conventions of the evaluation entries above
 * hold: ragged rows inside a common stride, DEVICE length and frame-count arrays copied to the host once to be checked, nothing behind a row's end read,
 * nothing outside the declared extents written, fixed-order sums without atomics, a row's result independent of its batch.  Frames are `frame` <= 512
 * samples at hop `hop` under the window w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / (frame + 1)), all FULL frames: frames(len) = (len - frame) / hop + 1 for
 * len >= frame, else 0.  Spectra are (B, ldf, 257) fp32: S[b][f][k], k = 0..256, the bins of one frame next to each other.
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer; B outside 1..65535; a length outside 1..2^30 or a frame count outside 0..2^30; a stride smaller
 * than the longest row (the most frames) it holds; frame outside 1..512; hop < 1; J outside 1..64; order outside 1..16 or >= frame; a workspace below the
 * size its query states (the queries give -1 for arguments out of range).
 *
 * buddy_frame_spectra: S[b][f][k] = |X[k]| of frame f < frames(lens[b]), X the 512-point transform (fp32, radix 2, the transform of buddy_band_spectra) of
 *   the windowed, zero-padded frame (w rounded to fp32, one fp32 product per sample); the magnitude is formed in double and rounded once.
 *   ldf >= max(frames of the longest row, 1).
 *
 * buddy_cepstral_distance: X, E spectra of the clean and the estimated rows with frames[b] frames; g, d DEVICE doubles (B): the estimate's gain and the
 *   log floor.  Per frame and signal c[n] = (1/512) sum_{k = 0..511} 0.5 ln(|X[k]|^2 + d) cos(2 pi k n / 512), n = 0..24 (bins above 256 by symmetry; the
 *   estimate with g |E[k]|); from each coefficient its mean over the row's frames is taken, per signal; frame value (10 / ln 10) sqrt(dc_0^2 + 2 sum_{n >= 1}
 *   dc_n^2), dc = c_x - c_e, clipped to [0, 10]; out[b] = the mean over the frames, all in double.  No frame, or d[b] not above zero: NaN and flags[b] = 0.
 *
 * buddy_fwsegsnr: M: DEVICE (J, 257) doubles >= 0, the band weights.  X_j = sum_k M[j][k] |X[k]|, E_j = sum_k M[j][k] g |E[k]|; num = X_j^2, den = (X_j -
 *   E_j)^2; band SNR 35 where den <= num 10^-3.5, else -10 where num <= den / 10, else 10 log10(num / den); W_j = X_j^0.2; frame value sum_j W_j snr_j / sum_j
 *   W_j; a frame counts when sum_j W_j > 0.  out[b] = the mean over the counted frames, counts[b] their number; none: NaN and flags[b] = 0.
 *
 * buddy_llr: from the signals.  s = w x in double; r[k] = sum_i s[i] s[i + k], k = 0..order, of both frames; a frame counts when r_x[0] > 0 and r_e[0] > 0;
 *   then r[0] *= 1 + 1e-9, Levinson-Durbin gives a (a[0] = 1) of each; frame value ln((a_e R_x a_e^T) / (a_x R_x a_x^T)), R_x the Toeplitz matrix of r_x,
 *   clipped to [0, 2]; all in double.  out[b] = the mean over the counted frames, counts[b] their number; none: NaN and flags[b] = 0. */
int buddy_frame_spectra(const float* x, const int* lens, int B, long long ld, int frame, int hop, float* S, long long ldf, void* stream);
long long buddy_cepstral_distance_workspace(int B, int max_frames);
int buddy_cepstral_distance(const float* X, const float* E, const int* frames, int B, long long ldf, const double* g, const double* d, double* out, int* flags,
                            void* ws, long long ws_bytes, void* stream);
long long buddy_fwsegsnr_workspace(int B, int max_frames);
int buddy_fwsegsnr(const float* X, const float* E, const int* frames, int B, long long ldf, const double* g, const double* M, int J, double* out, int* counts,
                   int* flags, void* ws, long long ws_bytes, void* stream);
long long buddy_llr_workspace(int B, long long max_len, int frame, int hop);
int buddy_llr(const float* e, const float* x, const int* lens, int B, long long ld, int frame, int hop, int order, double* out, int* counts, int* flags, void* ws,
              long long ws_bytes, void* stream);

/* ---- room impulse responses of shoebox rooms by the image-source method (buddy_amd/utils/rooms.py; Allen & Berkley 1979; no
 * reference counterpart).  rooms: DEVICE (B, 16) doubles per row: L (3) room size [m], s (3) source, r (3) receiver, beta (6) pressure reflection
 * coefficients of the walls x = 0, x = Lx, y = 0, y = Ly, z = 0, z = Lz, c speed of sound [m/s].  Per axis a an image (m, q), m any integer, q in {0, 1}:
 * offset X_a = 2 m L_a + (1 - 2 q) s_a - r_a, gain g_a = beta_a0^|m - q| beta_a1^|m| (0^0 = 1), order o_a = |m - q| + |m|.  An image triple has
 * d = sqrt(X^2 + Y^2 + Z^2), A = g_x g_y g_z / (4 pi d), tau = d fs / c, o = o_x + o_y + o_z.
 *   h[b][n] = sum A sinc(x) (1 + cos(pi x / Hw)) / 2,  x = n - Hw - tau,  n = 0..N - 1,
 * over the images with |x| < Hw (and o <= max_order unless max_order = -1), Hw = buddy_ism_half_width() = 40: sample n sits at time (n - Hw) / fs, the
 * direct peak near tau_direct + Hw.  All arithmetic, the delays included, is double; the sum is rounded once to fp32.  A sample's terms are added in the
 * ascending order of (m_x, q_x, m_y, q_y, q_z, m_z): no atomics, and a row's response does not depend on B, on the grid or on the run.
 * flags[b] = 1 for a valid row.  A row is invalid -- zeros in h[b][0..N - 1], flags[b] = 0, no other row disturbed -- when a value is not finite, an
 * L_a <= 0, s or r is not strictly inside the room, a |beta| > 1, c <= 0, or |s - r| < 0.01 m.
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer; B outside 1..65535; fs outside 1000..1000000; N outside 1..2^20; ldh < N; max_order < -1.
 * Nothing is written outside h[b][0..N - 1] and flags[0..B - 1]; no workspace.  Work: about (4/3) pi (c N / fs)^3 / (Lx Ly Lz) images of 2 Hw taps each
 * per row when no order caps them -- the rooms are device data, so the entry cannot bound it: the CALLER does (rooms.shoebox_rir refuses above
 * max_images).  buddy_ism_tile: output samples per workgroup; buddy_ism_list: images per LDS chunk of a tile's image list (the sizes around which
 * the unit tests place their lengths and rooms). */
int buddy_ism_half_width(void);
int buddy_ism_tile(void);
int buddy_ism_list(void);
int buddy_shoebox_rir(const double* rooms, int B, int fs, int N, int max_order, float* h, long long ldh, int* flags, void* stream);

/* ---- banded rooms: frequency-dependent walls and air absorption (buddy_amd/utils/rooms.py; no reference counterpart).  A banded
 * room is the row of 16 doubles above, whose own six coefficients are NOT read, plus DEVICE beta (B, nb, 6) doubles, pressure reflection coefficients
 * per band k and wall (the walls in the order above), and DEVICE air (B, nb) doubles, pressure attenuations in Np/m (NULL: zeros); nb in
 * 1..buddy_ism_max_bands() = 8.  Images, offsets, d, tau, o, the order cap and the kernel (Hw = 40) are those of buddy_shoebox_rir; per band
 *   A_k = g_x,k g_y,k g_z,k exp(-air[k] d) / (4 pi d),  g_a,k = beta[k][a0]^|m - q| beta[k][a1]^|m| (0^0 = 1),
 *   u[b][k][n] = sum A_k sinc(x) (1 + cos(pi x / Hw)) / 2,  x = n - Hw - tau,  |x| < Hw,  n = 0..N - 1,
 * all in double and stored in double; per band a sample's terms are added in the ascending order of (m_x, q_x, m_y, q_y, q_z, m_z): no atomics, and a
 * row does not depend on B, on the grid or on the run.  The powers are products (repeated squaring), not pow calls: at most o roundings per axis pair.
 * A row is invalid -- zeros in u[b][k][0..N - 1] for every k, flags[b] = 0, no other row disturbed -- for everything buddy_shoebox_rir names, tested on
 * the row without its own six coefficients, a |beta[k][w]| that is not finite or above 1, or an air[k] that is negative or not finite.
 * BUDDY_ERR_ARG, with nothing launched, for: a null rooms, beta, u or flags; B outside 1..65535; nb outside 1..buddy_ism_max_bands(); fs outside
 * 1000..1000000; N outside 1..2^20; ldu < N; max_order < -1.  Nothing is written outside u[b][k][0..N - 1] and flags[0..B - 1]; no workspace.  The
 * work is that of buddy_shoebox_rir plus nb multiply-adds per tap, and again the CALLER bounds it (rooms.shoebox_rir_bands refuses above max_images).
 *   buddy_band_combine: h[b][n] = sum_k sum_j bank[k][j] u[b][k][n - j], n = 0..N - 1, u zero below sample 0; bank DEVICE (nb, Nh) doubles, Nh odd.
 * The application is causal: with P = (Nh - 1) / 2 and zero-phase rows centred on tap P, sample n of h sits at time (n - Hw - P) / fs.  Accumulated in
 * double in the fixed order k ascending, then j ascending, rounded once to fp32.  BUDDY_ERR_ARG, with nothing launched, for: a null u, bank or h; B
 * outside 1..65535; nb outside 1..buddy_ism_max_bands(); N outside 1..2^20; ldu < N; ldh < N; Nh even or outside 1..65537.  Nothing is written
 * outside h[b][0..N - 1].  buddy_ism_band_list: images per LDS chunk of a banded tile's list; buddy_band_combine_tile: outputs per workgroup of the
 * combination (the sizes around which the unit tests place their rooms and lengths). */
int buddy_ism_max_bands(void);
int buddy_ism_band_list(void);
int buddy_band_combine_tile(void);
int buddy_shoebox_bands(const double* rooms, const double* beta, const double* air /* NULL: none */, int B, int nb, int fs, int N, int max_order,
                        double* u /* (B, nb, ldu) */, long long ldu, int* flags, void* stream);
int buddy_band_combine(const double* u, int B, int nb, long long ldu, int N, const double* bank /* (nb, Nh) */, int Nh, float* h, long long ldh, void* stream);

/* ---- diffuse noise fields by plane-wave superposition (buddy_amd/utils/noise.py, csrc/noise.hip; Habets & Gannot 2007; no
 * reference counterpart).  Item b of a call is one file: D microphones, N white plane waves, L output samples.  Wave n of item b is the source
 *   s_{b,n}[j], j = 0 .. L + 2 P - 1 = the kind-0 normals of buddy_philox_fill for (keys[b], purpose, draw0 + n, j), bit for bit,
 * generated inside the kernel and never stored.  taps: DEVICE (B, N, D, W) doubles, first: DEVICE (B, N, D) ints -- per (wave, microphone) the W
 * zero-padded coefficients of its fractional-delay filter and the integer lag of the first one; keys: DEVICE (B, 2) uint32; out: DEVICE (B, D, L) fp32.
 *   out[b][d][i] = scale * sum_n sum_k taps[b][n][d][k] * s_{b,n}[i + P - first[b][n][d] - k],  i = 0 .. L - 1,
 * where a source index outside [0, L + 2 P) contributes zero: that is the definition, so no `first` can make the kernel read out of bounds (a
 * `first` whose filters leave the range is the caller's mistake all the same, and noise.noise_bank_hip refuses it before uploading).  The sum is
 * accumulated in double in the fixed order n ascending, then k ascending, multiplied by scale and rounded once to fp32.  No atomics; a row's bits
 * depend on its own key, taps and first only -- not on B, the grid or the run.  One path serves every L >= 1.
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer; D outside 1..8; N outside 1..4096; W outside 1..buddy_noise_max_taps() = 80; P outside
 * 0..4096; B outside 1..65535; L outside 1..2^33 (a draw's sample index has 34 bits); a scale that is not finite.  Nothing is written outside out;
 * no workspace.  Work: B L N D W multiply-adds in double plus N (T + 2 P) / T normals per output sample, T = buddy_noise_tile() = 256 output
 * samples per workgroup (the size around which the unit tests place their lengths). */
int buddy_noise_tile(void);
int buddy_noise_max_taps(void);
int buddy_noise_bank(const double* taps /* (B,N,D,W) */, const int* first /* (B,N,D) */, const unsigned* keys /* (B,2) */, unsigned purpose, unsigned draw0,
                     float* out /* (B,D,L) */, int B, int D, int N, int W, int P, long long L, double scale, void* stream);

/* ---- diffuse late tail of simulated rooms (buddy_amd/utils/rooms.py, csrc/tail.hip; no reference counterpart).  The
 * image-source response u of a row, computed for len samples only, is cross-faded after a crossover n_x into Gaussian noise z under the exponential
 * envelope exp(-delta t_n), t_n = (n - Hw) / fs, Hw = buddy_ism_half_width(), level-matched to u's energy in the fit window [n_f, n_x).  Rows come in
 * groups of D consecutive rows (the microphones of one room), G = B / D groups; a group shares win, delta and its amplitude.  u: DEVICE, fp32 (f64 = 0)
 * or double (f64 = 1), sample n of band k of row b at u[b ldr + k ldk + n], n < len; win: DEVICE (G, 2) ints (n_f, n_x); delta: DEVICE (G, nb) doubles
 * [1/s]; nu: DEVICE (B,) doubles, the standard deviation of z per row (NULL: ones).
 *   buddy_tail_fit:  E_k = sum_rows sum_{n_f <= n < n_x} u_k[n]^2,  S_k = D sum_{n_f <= n < n_x} exp(-2 delta_k t_n),  amp[b][k] = sqrt(E_k / S_k) / nu[b],
 * amp DEVICE (B, nb) doubles; E_k = 0 gives amp = 0 and flags[g] = 4 (bit 2), else flags[g] = 0; flags DEVICE (G,) ints.  One workgroup per (group,
 * band); both sums in double, each thread adding its elements (flat index d W + j, W = n_x - n_f, stride 256, ascending), then lanes and waves in the
 * fixed order of the evaluation entries: no atomics, a group's bits do not depend on B.
 *   buddy_tail_mix:  th(n) = (pi / 2) clip((n - n_x + 1/2) / R, 0, 1),
 *   out[b][k][n] = u_k[n] for n < n_x (its bits),  cos th(n) u_k[n] + sin th(n) amp[b][k] exp(-delta_k t_n) z_b[n] for n_x <= n < N,  u_k[n] = 0 for n >= n_x + R,
 * in double, rounded once to the type of u, which is the type of out (sample n of band k of row b at out[b ldor + k ldok + n]).  z: DEVICE (B, ldz)
 * fp32, read for n_x <= n < N; or NULL: z_b[n] = kind-0 normal n of draw 0 of `purpose` of the stream keys[b] (DEVICE (B, 2) uint32), the bits
 * buddy_philox_fill stores, generated in the kernel once per four samples and used for every band.  One thread per four consecutive samples; fp32
 * rows whose bases and strides are multiples of 16 bytes move as 16-byte vectors, with the same bits as the element form.  u is read below n_x + R
 * only; nothing is written outside out[b][k][0..N - 1].  No atomics; a row's bits depend on its own u, win, delta, amp and z or key only.
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer (nu may be NULL; z or keys may be NULL, not both); B outside 1..65535; nb outside
 * 1..buddy_ism_max_bands(); D outside 1..8; B % D != 0; fs outside 1000..1000000; len outside 1..2^20; ldr < len, or ldk < len with nb > 1; R outside
 * 1..2^20; N outside 1..2^30; ldz < N; ldok < N with nb > 1, or ldor < (nb - 1) ldok + N; and, read from the device once after the work queued on
 * `stream`: a window without 0 <= n_f < n_x, n_x + R > len (buddy_tail_fit: n_x > len), a delta that is not finite, a nu that is not positive and
 * finite.  No workspace.  buddy_tail_tile: output samples per workgroup of buddy_tail_mix (the size around which the unit tests place their lengths). */
int buddy_tail_tile(void);
int buddy_tail_fit(const void* u, int f64, int B, int nb, int D, long long ldr, long long ldk, int len, const int* win /* (G,2) */,
                   const double* delta /* (G,nb) */, const double* nu /* (B,) or NULL */, int fs, double* amp /* (B,nb) */, int* flags /* (G,) */, void* stream);
int buddy_tail_mix(const void* u, int f64, int B, int nb, int D, long long ldr, long long ldk, int len, const int* win /* (G,2) */, int R,
                   const double* delta /* (G,nb) */, const double* amp /* (B,nb) */, const float* z /* (B,ldz) or NULL */, long long ldz,
                   const unsigned* keys /* (B,2) or NULL */, unsigned purpose, int fs, int N, void* out, long long ldor, long long ldok, void* stream);

/* ---- paired comparison of two runs (buddy_amd/utils/compare.py, csrc/compare.hip; no reference counterpart): the resampling
 * behind bootstrap intervals and the sign-flip randomisation test of columns of paired differences.  A call holds C ragged columns of finite doubles,
 * element j of column c at d[c ld + j], j < lens[c]; lens: DEVICE (C,) ints, read once on the host to be checked; keys: DEVICE (C, 2) uint32, the Philox
 * stream of each column (utils/rng.py: sample i of draw q of purpose p is word i & 3 of the block with counter (i >> 2, q, p, 0)).  A column's bits
 * depend on its own data, length, key and draw0 only: not on C, on its position or on the other columns.  All sums have one association whatever the
 * call.  buddy_compare_max_pairs() = 8192: the longest column (the bootstrap's LDS counters).
 *   buddy_compare_bootstrap: s holds each column SORTED ascending.  Resample r < R draws n = lens[c] ranks, rank j = (w_j n) >> 32 in 64-bit integers
 * with w_j sample j of draw draw0 + r of purpose 11 (bias of a rank's probability at most n / 2^32), counted in cnt[k] (integer LDS atomics).
 * out: DEVICE (C, 2, R) doubles; out[c][0][r] = (sum_k cnt[k] s[k]) / n, thread t of 256 adding k = t, t + 256, ... ascending, then lanes and waves in
 * the fixed order of the evaluation entries; out[c][1][r] = the median of the drawn values by numpy's rule, s[k_m] for odd n and (s[k_a] + s[k_b]) * 0.5
 * for even n, the ranks found in the prefix sum of cnt: integer work, exact.  One workgroup per (resample, column).
 *   buddy_compare_select: out[m][q] = the element of rank ranks[q] (0-based, ascending) of row m of x (M rows of R doubles, row stride ldx), by an
 * 8-bit radix select on the order-preserving 64-bit key: exact, any R; -0 ranks below +0; no NaN.  ranks: DEVICE (K,) ints; out: DEVICE (M, K).
 *   buddy_compare_signflip: T[c][r] = sum_j sigma_rj d[c][j], j ascending in one double accumulator, the sign applied by negation.  modes: DEVICE (C,)
 * ints.  Mode 0 (random): r < P, sigma_rj = -1 where bit j & 31 of sample j >> 5 of draw draw0 + r of purpose 12 is set.  Mode 1 (exhaustive):
 * r < 2^n, sigma_rj = -1 where bit j of r is set; T[c][r] for r >= 2^n is not written.  T: DEVICE (C, P) doubles; tobs: DEVICE (C,) doubles, the same
 * loop with every sign +, the bits of pattern 0 of mode 1.  One thread per pattern.
 *   buddy_compare_count_ge: out[c] = #{r < counts[c] : |T[c][r]| >= thr[c]}, T rows of stride ldt; counts: DEVICE (C,) ints; thr: DEVICE (C,) doubles;
 * out: DEVICE (C,) 64-bit integers.  Exact.
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer; C, M or K outside 1..65535; R outside 1..2^24 (select: R < 1); P outside 1..2^30;
 * draw0 + R (or + P) above 2^32; a length outside 1..buddy_compare_max_pairs(); ld below a length; ldx < R; a rank outside 0..R-1; a mode other than
 * 0 or 1; an exhaustive column with 2^n > P; a count outside 1..ldt.  No workspace; nothing outside the stated extents is written. */
int buddy_compare_max_pairs(void);
int buddy_compare_bootstrap(const double* s /* (C,ld) */, const int* lens /* (C,) */, const unsigned* keys /* (C,2) */, int C, long long ld, int R,
                            unsigned draw0, double* out /* (C,2,R) */, void* stream);
int buddy_compare_select(const double* x /* (M,ldx) */, int M, int R, long long ldx, const int* ranks /* (K,) */, int K, double* out /* (M,K) */, void* stream);
int buddy_compare_signflip(const double* d /* (C,ld) */, const int* lens /* (C,) */, const int* modes /* (C,) */, const unsigned* keys /* (C,2) */, int C,
                           long long ld, int P, unsigned draw0, double* T /* (C,P) */, double* tobs /* (C,) */, void* stream);
int buddy_compare_count_ge(const double* T /* (C,ldt) */, const int* counts /* (C,) */, const double* thr /* (C,) */, int C, long long ldt,
                           long long* out /* (C,) */, void* stream);

/* ---- noise power tracker and spectral post-filter of noisy recordings (buddy_amd/utils/denoise.py, csrc/denoise.hip; Gerkmann &
 * Hendriks 2012, Ephraim & Malah 1984 / 1985; no reference counterpart).  The conventions of the evaluation entries hold: ragged rows inside a common
 * stride, a DEVICE length array copied to the host once to be checked, nothing behind a row's end read, nothing outside the declared extents written,
 * fixed-order sums without atomics, a row's bits independent of its batch.  Frames are N = 512 samples at hop H = 128 and overhang both ends of the
 * row by P = 384 samples: frames(L) = (L - 1 + P) / H + 1 = buddy_denoise_frames(L) (-1 for L outside 1..2^30), frame t covers samples
 * t H - P .. t H - P + 511, zeros outside [0, L); every sample lies in exactly four frames.  Window w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 513).
 * Spectra Y are (B, ldt, 257) pairs of fp32 (re, im); G and sigma2 are (B, ldt, 257) fp32; ldt >= frames of the longest row.
 * BUDDY_ERR_ARG, with nothing launched, for: a null pointer; B outside 1..65535; a length outside 1..2^30; ld below the longest row; ldt below its
 * frames; a gain rule other than 0 or 1; g_min outside (0, 1]; a phi[b] that is negative or not finite; a workspace below the size its query states.
 *
 * buddy_denoise_spectra: Y[b][t][k], k = 0..256: the 512-point transform (fp32, radix 2, the transform of buddy_frame_spectra) of the windowed frame
 *   (w rounded to fp32, one fp32 product per sample).
 * buddy_denoise_gains: phi: DEVICE doubles (B), the row floor (0: an all-zero row, G = 1 and sigma2 = 0 everywhere).  Per bin, frames ascending, all in
 *   double: sigma^2 starts as the mean of |Y|^2 over the first min(8, full frames) frames that lie inside the row (t >= 3; over all frames where none
 *   does), lower-bounded by phi; Pbar = 0.5; A^2 = 0.  Per frame, xi1 = 10^1.5:  p = 1 / (1 + (1 + xi1) exp(-(|Y|^2 / sigma^2) xi1 / (1 + xi1)));
 *   Pbar = 0.9 Pbar + 0.1 p, and p = min(p, 0.99) where Pbar > 0.99;  sigma^2 = max(0.8 sigma^2 + 0.2 (p sigma^2 + (1 - p) |Y|^2), phi);
 *   gamma = clip(|Y|^2 / sigma^2, 1e-6, 1e3);  xi = max(0.98 A^2 / sigma^2 + 0.02 max(gamma - 1, 0), 10^-2.5);  a = xi / (1 + xi);  rule 0 (wiener)
 *   G = a, rule 1 (lsa) G = min(a exp(E1(a gamma) / 2), 1);  G = max(G, g_min);  A^2 = G^2 |Y|^2.  G and the updated sigma^2 are rounded once to fp32.
 *   One thread per (row, bin) and T dependent steps: latency-bound by construction.
 * buddy_denoise_synthesis: x^_t = Re(inverse transform of G[t] Y[t]) (one fp32 product per component, the same fp32 transform on the conjugate, / 512)
 *   into ws; out[b][n] = sum_t w[n - s_t] x^_t[n - s_t] / sum_t w^2[n - s_t] over the four frames that cover n (s_t = t H - P), t ascending, w and the
 *   sums in double, rounded once.  ws: buddy_denoise_synthesis_workspace(B, ldt) bytes (-1 for arguments out of range).
 * buddy_denoise_stats: stats (B, 4) doubles: snr_est_db = 10 log10(sum max(|Y|^2 - sigma2, 0) / sum sigma2) over all frames and bins,
 *   noise_db = 10 log10(mean sigma2 / sum w^2), att_db = 10 log10(sum x^2 / sum out^2), and the flag word (1 ZERO: the row is all zeros, the three
 *   values are NaN; 2 SHORT: no frame lies inside the row, L < 512; 4 NO_SPEECH: the numerator is 0, snr_est_db = -inf).  One workgroup per row. */
long long buddy_denoise_frames(long long L);
int buddy_denoise_spectra(const float* x, const int* lens, int B, long long ld, float* Y /* (B,ldt,257,2) */, long long ldt, void* stream);
int buddy_denoise_gains(const float* Y, const int* lens, const double* phi, int B, long long ldt, int rule, double g_min, float* G, float* sigma2, void* stream);
long long buddy_denoise_synthesis_workspace(int B, long long ldt);
int buddy_denoise_synthesis(const float* Y, const float* G, const int* lens, int B, long long ldt, float* out, long long ld, void* ws, long long ws_bytes,
                            void* stream);
int buddy_denoise_stats(const float* x, const float* out, const int* lens, int B, long long ld, const float* Y, const float* sigma2, long long ldt, double* stats,
                        void* stream);

/* ---- the small fp32 kernels of the network, one entry per launcher (unit tests: tests/test_hip_small_ops.py).  All tensors NHWC with H = time, device
 * pointers, fp32.  Each entry returns BUDDY_ERR_ARG with a message, with nothing launched, for a null required pointer, an empty shape, or a shape its
 * kernels cannot compute (named per entry).
 *
 * conv_c2in:  x (B,H,W,2) -> y rows of ldY floats, Cout live; w [Cout][taps][2], taps 1 or 9 (3 x 3, zero padding, tap = 3 (dh + 1) + (dw + 1));
 *             y = conv + bias (NULL = none) + add (rows of add_ld floats, NULL = none) [+ y if accumulate].  Refused: Cout % 4, ldY / add_ld not a
 *             multiple of 4 or below Cout.
 * conv_c2out: x rows of ldX floats, Cin live -> y (B,H,W,2); w [taps][Cin][2]; y = conv + bias + up_add (B,H/2,W/2,2 nearest-upsampled) [+ y].
 *             form: -1 the process default, 0 lane-group kernel, 1 tiled, 2 strip (1 and 2: 9 taps and Cin % 32 == 0).  Refused: Cin % 4, ldX % 4,
 *             ldX < Cin, odd H or W with up_add. */
int buddy_conv_c2in(const float* x, const float* w, const float* bias, const float* add, int add_ld, float* y, int ldY, int B, int H, int W, int Cout,
                    int taps, int accumulate, void* stream);
int buddy_conv_c2out(const float* x, int ldX, const float* w, const float* bias, const float* up_add, float* y, int B, int H, int W, int Cin, int taps,
                     int accumulate, int form, void* stream);
/* STFT glue.  reflect_pad: xp (B,Lp) = scale * scale_b[b] * reflect(x (B,L), pad), zero from L + 2 pad to Lp; refused: pad >= L, Lp < L + 2 pad.
 * ola: y (B,L)[s] = inv_env[s + pad] * sum_t frames[b][t][s + pad - t hop] over t < Tp (frames rows of ldF floats, n_fft live), then with xin:
 *      y = cskip_b[b] xin + cout_b[b] y.  inv_env has n_fft + hop (Tp - 1) entries; refused: ldF < n_fft, L + pad beyond the envelope.
 * ola_adj: the adjoint of ola in `frames` (every float of the (B,Tp,ldF) buffer is written, the row padding with 0).
 * unpad_adj: dx (B,L) = scale * scale_b[b] * (adjoint of framing(reflect_pad(x))) applied to dframes (B,T,ldF) [+ cskip_b[b] * g_out]; refused: pad >= L. */
int buddy_reflect_pad(const float* x, float* xp, int B, int L, int pad, int Lp, float scale, const float* scale_b, void* stream);
int buddy_ola(const float* frames, int ldF, int Tp, int n_fft, int hop, const float* inv_env, float* y, int B, int L, int pad, const float* xin,
              const float* cskip_b, const float* cout_b, void* stream);
int buddy_ola_adj(const float* g, int B, int L, int pad, int Tp, int n_fft, int hop, const float* inv_env, const float* cout_b, float* frames, int ldF,
                  void* stream);
int buddy_unpad_adj(const float* dframes, int ldF, int T, int n_fft, int hop, int B, int L, int pad, float scale, const float* scale_b,
                    const float* g_out, const float* cskip_b, float* dx, void* stream);
/* pool2: dst (B,H/2,W/2,C) = scale * (sum of the 2 x 2 box) [+ dst]; refused: odd H or W, C neither 2 nor a multiple of 4.
 * up2_acc: dst (B,2Hs,2Ws,C) = scale * nearest(src (B,Hs,Ws,C)) [+ dst]; refused: odd C. */
int buddy_pool2(const float* src, float* dst, int B, int H, int W, int C, float scale, int accumulate, void* stream);
int buddy_up2_acc(const float* src, float* dst, int B, int Hs, int Ws, int C, float scale, int accumulate, void* stream);
/* fourier: out (B,2 nf) = [sin, cos](cnoise[b] * Wf[j] * 2 * pi) (fp32 phase, that product order).  linear: y (B,N) = act(x (B,K)) W^T (N,K) + bias,
 * act = SiLU if silu_in. */
int buddy_fourier(const float* cnoise, const float* Wf, float* out, int B, int nf, void* stream);
int buddy_linear(const float* x, const float* W, const float* bias, float* y, int B, int K, int N, int silu_in, void* stream);
/* materialised attention: row softmax in place; dP <- P * (dP - sum_j P dP) per row; dst[b] = src[b]^T (n x n; refused: n % 32, in place) */
int buddy_softmax_rows(float* S, int rows, int cols, void* stream);
int buddy_softmax_bwd_rows(const float* P, float* dP, int rows, int cols, void* stream);
int buddy_transpose_sq(const float* src, float* dst, int batch, int n, void* stream);
/* mix2: y (npix,2) = x W^T + b with W (2,2) (transpose: y = x W, no bias) [+ y].  axpy: dst = alpha * src [+ dst]; refused: n % 4. */
int buddy_mix2(const float* x, const float* w, const float* b, float* y, long long npix, int transpose, int accumulate, void* stream);
int buddy_axpy(float* dst, const float* src, float alpha, long long n, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
