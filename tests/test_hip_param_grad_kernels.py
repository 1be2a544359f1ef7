"""GPU unit tests of the parameter-gradient kernels (csrc/wgrad.hip) behind their own C-ABI entries, each against a plain torch float64
restatement of the same operation on the same inputs, at the smallest shapes that engage every mechanism of the kernels: chunk seams and a
ragged last chunk of the split-K weight gradient, an utterance boundary inside one 32-pixel step, ragged N / K tiles, the two-source and
resampling loaders, the three output layouts and the transposed dY view.

Axis convention of the network: NHWC with H = time = kx and W = frequency = ky, so torch sees a tensor as (B, C, W, H).

Gates (relative errors against float64):
  weight gradient, plain loader     2e-5 of the abs-max: fp32 MFMA products are exact and accumulate like an fmaf chain, the bound
                                    test_hip_kernels.py states for contractions of up to 4608 terms (every case here has M <= 4608)
  weight gradient, GN / SiLU loader max(2e-5, 4 x e32), e32 = the error of torch's own fp32 autograd of the same composite
  column sums, basis bias           1e-6 of sum |y| (double accumulation, one rounding to float)
  GroupNorm gamma / beta            1e-5 of sum |dz * xhat| and sum |dz|
  linear backward                   2e-5 of the abs-max
Every case prefills the output with a known non-zero tensor and checks out == prefill + alpha * grad; workspaces are prefilled with NaN."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-6
NAN = float("nan")
GUARD = 256           # floats behind every workspace that must stay untouched


@pytest.fixture(scope="module")
def lib():
    from buddy_amd import _lib
    return _lib.require_gpu()


def P(t):
    return None if t is None else t.data_ptr()


def S():
    return torch.cuda.current_stream().cuda_stream


def check(rc):
    from buddy_amd import _lib
    _lib.check(rc)


def workspace(n):
    """NaN-filled workspace of n floats (8-byte aligned) followed by a guard"""
    return torch.full((int(n) + GUARD,), NAN, device="cuda")


def guard_intact(ws):
    return bool(torch.isnan(ws[-GUARD:]).all())


def padded(x, ld):
    """rows of x (..., C) at a row stride of ld >= C floats; the padding columns hold NaN (no kernel may read them)"""
    C = x.shape[-1]
    buf = torch.full((x.numel() // C, ld), NAN)
    buf[:, :C] = x.reshape(-1, C)
    return buf.cuda()


def groups_of(C):
    return min(max(C // 4, 1), 32)


def gn_stats(x, G):
    """(mean, rstd) [B][G][2] of an NHWC tensor in float64, rounded to the float32 the kernels read"""
    B, C = x.shape[0], x.shape[-1]
    xg = x.double().reshape(B, -1, G, C // G)
    mean = xg.mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False) + EPS)
    return torch.stack([mean, rstd], dim=-1).float().contiguous()


# ------------------------------------------------------------------------------------------------ weight gradient: references
def torch_wgrad(dt, x, dY, taps, rs, gn, silu):
    """The weight gradient as torch states it: the .grad of w (torch OIHW) under conv2d(resample(act(group_norm(x))), w) with cotangent dY.
    x (B, Hs, Ws, Cin) and dY (B, H, W, N) are NHWC with H = time; torch gets (B, C, W, H)."""
    X = x.to(dt).permute(0, 3, 2, 1).contiguous()
    if gn is not None:
        G, gamma, beta = gn
        X = F.group_norm(X, G, gamma.to(dt), beta.to(dt), eps=EPS)
    if silu:
        X = F.silu(X)
    if rs == 1:
        X = F.avg_pool2d(X, 2)
    elif rs == 2:
        X = F.interpolate(X, scale_factor=2, mode="nearest")
    N, Cin, k = dY.shape[-1], x.shape[-1], 3 if taps == 9 else 1
    w = torch.zeros(N, Cin, k, k, dtype=dt, requires_grad=True)
    y = F.conv2d(X, w, padding=k // 2)
    gw, = torch.autograd.grad(y, w, dY.to(dt).permute(0, 3, 2, 1).contiguous())
    return gw


def to_layout(gw, layout):
    """torch OIHW [N][Cin][ky = dw + 1][kx = dh + 1] -> the kernel's layout: 0 = [N][K], k = (3 (dh + 1) + (dw + 1)) Cin + c; 1 = OIHW; 2 = [K][N]"""
    if layout == 1:
        return gw
    g0 = gw.permute(0, 3, 2, 1).reshape(gw.shape[0], -1)
    return g0 if layout == 0 else g0.t()


def im2col(a, taps):
    """A[m][tap * Cin + c] of an NHWC tensor on its own grid, tap = 3 (dh + 1) + (dw + 1) over the zero-padded neighbourhood: the index-exact
    tests' reference, stated without a convolution"""
    B, H, W, C = a.shape
    if taps == 1:
        return a.reshape(B * H * W, C)
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    cols = [ap[:, 1 + dh:1 + dh + H, 1 + dw:1 + dw + W, :] for dh in (-1, 0, 1) for dw in (-1, 0, 1)]
    return torch.stack(cols, dim=3).reshape(B * H * W, 9 * C)


class WgCase:
    """inputs of one weight-gradient case from a seeded CPU generator, with its float64 and float32 torch gradients (computed once)"""

    def __init__(self, B, H, W, Cin, N, taps, rs=0, C0=0, ld0=0, ld1=0, gn=False, silu=False, seed=0):
        self.B, self.H, self.W, self.Cin, self.N, self.taps, self.rs, self.C0, self.silu = B, H, W, Cin, N, taps, rs, C0, silu
        g = torch.Generator(device="cpu").manual_seed(1000 * seed + B * H * W + Cin + N)
        Hs, Ws = (2 * H, 2 * W) if rs == 1 else (H // 2, W // 2) if rs == 2 else (H, W)
        self.x = torch.randn(B, Hs, Ws, Cin, generator=g) * 1.5 + 0.3
        self.dY = torch.randn(B, H, W, N, generator=g)
        self.gn = None
        if gn:
            self.gn = (groups_of(Cin), 1 + 0.2 * torch.randn(Cin, generator=g), 0.2 * torch.randn(Cin, generator=g))
        self.ld0 = ld0 or (C0 if C0 else Cin)
        self.ld1 = ld1 or (Cin - C0 if C0 else 0)
        self.ref = torch_wgrad(torch.float64, self.x, self.dY, taps, rs, self.gn, silu)
        g32 = torch_wgrad(torch.float32, self.x, self.dY, taps, rs, self.gn, silu)
        self.e32 = float((g32.double() - self.ref).abs().max() / self.ref.abs().max())

    def device_inputs(self, b0=0, b1=None):
        """device tensors of the utterances [b0, b1)"""
        b1 = self.B if b1 is None else b1
        x = self.x[b0:b1]
        d = {"B": b1 - b0, "dy": self.dY[b0:b1].contiguous().cuda()}
        if self.C0:
            d["x0"], d["x1"] = padded(x[..., :self.C0], self.ld0), padded(x[..., self.C0:], self.ld1)
        else:
            d["x0"], d["x1"] = padded(x, self.ld0), None
        if self.gn is not None:
            d["stats"] = gn_stats(self.x, self.gn[0])[b0:b1].contiguous().cuda()
            d["gamma"], d["beta"] = self.gn[1].cuda(), self.gn[2].cuda()
        return d


def run_wgrad(lib, c, d, layout, alpha, out, dy=None, view=None):
    """one buddy_weight_grad call of case c on the device inputs d, into out; view = (T, sb, sm, sn) of dy (default: row-major NHWC)"""
    B, M = d["B"], d["B"] * c.H * c.W
    K = c.taps * c.Cin
    T, sb, sm, sn = view or (c.H * c.W, c.H * c.W * c.N, c.N, 1)
    ws = workspace(lib.buddy_weight_grad_workspace(M, c.N, K))
    assert lib.buddy_weight_grad_workspace(M, c.N, K) == lib.buddy_weight_grad_chunks(M, c.N, K) * c.N * K
    G = c.gn[0] if c.gn is not None else 1
    check(lib.buddy_weight_grad(P(d["dy"] if dy is None else dy), T, sb, sm, sn, P(d["x0"]), P(d["x1"]), c.C0, c.ld0, c.ld1, c.H, c.W, c.Cin, c.taps,
                                c.rs, P(d.get("stats")), P(d.get("gamma")), P(d.get("beta")), G, int(c.silu), B, c.N, layout, alpha, P(ws), P(out),
                                S()))
    torch.cuda.synchronize()
    assert guard_intact(ws), "wrote behind the workspace"
    return out


def prefill(shape, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) + 3.0)


def wgrad_error(lib, c, layout, alpha=1.0):
    """error of out == prefill + alpha * grad against float64, relative to the gradient's abs-max"""
    ref = to_layout(c.ref, layout)
    pre = prefill(ref.shape)
    out = run_wgrad(lib, c, c.device_inputs(), layout, alpha, pre.cuda())
    want = pre.double() + alpha * ref
    return float((out.cpu().double() - want).abs().max() / (abs(alpha) * ref.abs().max()))


def wgrad_gate(c):
    return 2e-5 if (c.gn is None and not c.silu) else max(2e-5, 4 * c.e32)


def report_and_check(name, c, e):
    print(f"wgrad {name}: B={c.B} H={c.H} W={c.W} Cin={c.Cin} N={c.N} taps={c.taps} rs={c.rs} gn={int(c.gn is not None)} silu={int(c.silu)}: "
          f"kernel {e:.2e}, torch fp32 (e32) {c.e32:.2e}, gate {wgrad_gate(c):.2e}")
    assert e < wgrad_gate(c)


@functools.lru_cache(maxsize=None)
def seam_case():
    # M = 720: 3 chunks of 256 / 256 / 208 pixels, seams mid-row (W = 18), the utterance boundary (pixel 360) inside the step [352, 384), a last
    # step of 16 pixels
    return WgCase(2, 20, 18, 32, 64, 9, gn=True, silu=True, seed=1)


# ------------------------------------------------------------------------------------------------ weight gradient: tests
def test_wgrad_chunk_seams_and_ragged_tail(lib):
    c = seam_case()
    assert lib.buddy_weight_grad_chunks(720, 64, 288) == 3
    for layout, alpha in ((1, 1.0), (0, 1 / math.sqrt(2))):
        report_and_check(f"seams (layout {layout})", c, wgrad_error(lib, c, layout, alpha))


@pytest.mark.parametrize("gn", [0, 1])
def test_wgrad_less_than_one_step(lib, gn):
    """M = 30 < one 32-pixel step, every tap of a 6 x 5 grid touches a border; N = 4 and K = 72 leave most of the tile empty"""
    c = WgCase(1, 6, 5, 8, 4, 9, gn=bool(gn), silu=bool(gn), seed=2)
    assert lib.buddy_weight_grad_chunks(30, 4, 72) == 1
    report_and_check("M < 32", c, wgrad_error(lib, c, 1))


@pytest.mark.parametrize("N", [2, 96])
def test_wgrad_ragged_n_and_k(lib, N):
    """K = 360: a second K block with 104 live columns; N = 2 (the C -> 2 heads) and N = 96 (a second, half-empty N block); M = 260: chunks of
    160 / 100 pixels, a last step of 4"""
    c = WgCase(2, 10, 13, 40, N, 9, gn=True, silu=True, seed=3)
    assert lib.buddy_weight_grad_chunks(260, N, 360) == 2
    report_and_check(f"ragged N={N}", c, wgrad_error(lib, c, 1))
    report_and_check(f"ragged N={N} (layout 2)", c, wgrad_error(lib, c, 2, -0.5))


def test_wgrad_training_size_two_sources(lib):
    """4 x 14 tiles: N = 256, Cin = 384 from two sources split at 256 with different row strides, M = 576 in 3 chunks of 192"""
    c = WgCase(2, 16, 18, 384, 256, 9, C0=256, ld0=256, ld1=160, gn=True, silu=True, seed=4)
    assert lib.buddy_weight_grad_chunks(576, 256, 3456) == 3
    report_and_check("two sources", c, wgrad_error(lib, c, 1, 1 / math.sqrt(2)))


def test_wgrad_training_size_1x1(lib):
    """the NIN form at training width: N = 128, Cin = 512, one tap, layout 0, GroupNorm without SiLU (the attention block's loader)"""
    c = WgCase(2, 16, 18, 512, 128, 1, gn=True, silu=False, seed=5)
    report_and_check("1x1", c, wgrad_error(lib, c, 0))


@pytest.mark.parametrize("gn", [0, 1])
@pytest.mark.parametrize("taps", [9, 1])
@pytest.mark.parametrize("rs", [1, 2])
def test_wgrad_resampling_loaders(lib, rs, taps, gn):
    """rs = 1: source at (2H, 2W), the box mean of the activated values, odd W = 9 on the output grid; rs = 2: source at (H/2, W/2) = (7, 5),
    nearest; two sources split at 32 of 64 channels with padded rows; M = 270 / 280: two chunks"""
    B, H, W = (3, 10, 9) if rs == 1 else (2, 14, 10)
    c = WgCase(B, H, W, 64, 64, taps, rs=rs, C0=32, ld0=40, ld1=32, gn=bool(gn), silu=bool(gn), seed=6 + rs)
    assert lib.buddy_weight_grad_chunks(B * H * W, 64, taps * 64) == 2
    report_and_check(f"resample rs={rs}", c, wgrad_error(lib, c, 1 if taps == 9 else 0))


def test_wgrad_two_channel_inputs(lib):
    """conv_in (Cin = 2, 3 x 3, K = 18) and output_layer (Cin = 2, 1 x 1, N = 2, layout 0)"""
    c = WgCase(2, 11, 13, 2, 32, 9, seed=9)
    report_and_check("conv_in", c, wgrad_error(lib, c, 1))
    c = WgCase(2, 11, 13, 2, 2, 1, seed=10)
    report_and_check("output_layer", c, wgrad_error(lib, c, 0))


def test_wgrad_layout2_transposed_dy_view(lib):
    """the attention's dV^T per utterance ([B][C][T]: sb = T C, sm = 1, sn = T) at C = 64, T = 144, B = 3, layout 2: bit for bit the result of the
    row-major view, and within the gate of float64"""
    c = WgCase(3, 16, 9, 64, 64, 1, gn=True, silu=False, seed=11)
    T, C = 144, 64
    d = c.device_inputs()
    ref = to_layout(c.ref, 2)
    pre = prefill(ref.shape)
    o_row = run_wgrad(lib, c, d, 2, 1.0, pre.cuda())
    dyT = d["dy"].reshape(3, T, C).transpose(1, 2).contiguous()
    o_tr = run_wgrad(lib, c, d, 2, 1.0, pre.cuda(), dy=dyT, view=(T, T * C, 1, T))
    assert torch.equal(o_row, o_tr)
    e = float((o_tr.cpu().double() - (pre.double() + ref)).abs().max() / ref.abs().max())
    report_and_check("transposed dY", c, e)


@pytest.mark.parametrize("taps", [9, 1])
def test_wgrad_index_exact_layouts(lib, taps):
    """dY selects one (pixel, n) with the value 1 and x holds small distinct integers: the gradient is row n = the neighbourhood of that pixel,
    exactly representable, so every layout must EQUAL the float64 result.  Pixels: the corners, both sides of the utterance boundary (359, 360: an
    image border), both sides of the chunk seams (255 / 256, 511 / 512: mid-row) and the last, 16-pixel step (704, 719)."""
    B, H, W, Cin, N = 2, 20, 18, 5, 3
    M, K = B * H * W, taps * Cin
    assert lib.buddy_weight_grad_chunks(M, N, K) == 3
    x = (torch.arange(M * Cin, dtype=torch.float32) + 1).reshape(B, H, W, Cin)
    A = im2col(x.double(), taps)
    xd = x.cuda()
    ws = workspace(lib.buddy_weight_grad_workspace(M, N, K))
    for i, pix in enumerate([0, 17, 255, 256, 342, 359, 360, 511, 512, 704, 719]):
        n = i % N
        dy = torch.zeros(M, N)
        dy[pix, n] = 1.0
        dyd = dy.cuda()
        g0 = torch.zeros(N, K, dtype=torch.float64)
        g0[n] = A[pix]
        for layout in ((0, 1, 2) if taps == 9 else (0, 2)):
            want = g0 if layout == 0 else g0.t() if layout == 2 else g0.reshape(N, 3, 3, Cin).permute(0, 3, 2, 1)   # [n][dh][dw][c] -> [n][c][dw][dh]
            pre = (torch.arange(want.numel(), dtype=torch.float32) % 11 + 1).reshape(want.shape)
            out = pre.cuda()
            ws.fill_(NAN)
            check(lib.buddy_weight_grad(P(dyd), H * W, H * W * N, N, 1, P(xd), None, 0, Cin, 0, H, W, Cin, taps, 0, None, None, None, 1, 0, B, N,
                                        layout, 1.0, P(ws), P(out), S()))
            torch.cuda.synchronize()
            assert torch.equal(out.cpu().double(), pre.double() + want), f"pixel {pix}, n {n}, layout {layout}"
    assert guard_intact(ws)


def test_wgrad_deterministic_and_additive_over_utterances(lib):
    """two runs of the seam case give the same bits; the B = 2 result is the sum of its two B = 1 runs within the GEMM gate (2e-5 of the abs-max)"""
    c = seam_case()
    d = c.device_inputs()
    shape = c.ref.shape
    o1 = run_wgrad(lib, c, d, 1, 1.0, prefill(shape).cuda())
    o2 = run_wgrad(lib, c, d, 1, 1.0, prefill(shape).cuda())
    assert torch.equal(o1, o2)
    acc = prefill(shape).cuda()
    for b in range(c.B):
        run_wgrad(lib, c, c.device_inputs(b, b + 1), 1, 1.0, acc)
    e = float((acc.double() - o1.double()).abs().max() / c.ref.abs().max())
    print(f"wgrad B = 2 against the sum of its B = 1 runs: {e:.2e}")
    assert e < 2e-5


# ------------------------------------------------------------------------------------------------ column sums, basis bias
@pytest.mark.parametrize("N", [2, 64, 100])
def test_colsum(lib, N):
    """T = 2048 + 37 rows per utterance (two chunks, the second ragged), B = 3, values that cancel (zero mean, a 1e-3 offset, as the pyramid heads'
    gradients); per-utterance sums bc at ld_bc > N, out and out2 with alpha = 1 / sqrt 2, each output on its own, a padded row stride, and the
    transposed view [B][N][T], which must give the same bits.  1e-6 of sum |y|."""
    B, T, ld, ld_bc, alpha = 3, 2048 + 37, N + 3, N + 5, 1 / math.sqrt(2)
    g = torch.Generator(device="cpu").manual_seed(40 + N)
    y = torch.randn(B, T, N, generator=g) + 1e-3
    yd = y.double()
    per_utt, tot = yd.sum(dim=1), yd.sum(dim=(0, 1))
    den_b, den = yd.abs().sum(dim=1), yd.abs().sum(dim=(0, 1))
    assert lib.buddy_colsum_workspace(B, T, N) == 2 * B * 2 * N
    ws = workspace(lib.buddy_colsum_workspace(B, T, N))
    y_row = padded(y, ld)
    y_tr = y.transpose(1, 2).contiguous().cuda()
    p1, p2 = prefill((N,), 6), prefill((N,), 7)
    results = []
    for dy, view in ((y_row, (T, T * ld, ld, 1)), (y_tr, (T, T * N, 1, T))):
        bc = torch.full((B, ld_bc), 9.0, device="cuda")
        o1, o2 = p1.cuda(), p2.cuda()
        ws.fill_(NAN)
        check(lib.buddy_colsum(P(dy), *view, B, N, alpha, P(ws), P(bc), ld_bc, P(o1), P(o2), S()))
        torch.cuda.synchronize()
        assert torch.equal(bc[:, N:], torch.full((B, ld_bc - N), 9.0, device="cuda"))
        e_bc = float(((bc[:, :N].cpu().double() - per_utt).abs() / den_b).max())
        e1 = float(((o1.cpu().double() - (p1.double() + alpha * tot)).abs() / den).max())
        e2 = float(((o2.cpu().double() - (p2.double() + alpha * tot)).abs() / den).max())
        print(f"colsum N={N} view sm={view[2]}: bc {e_bc:.2e}, out {e1:.2e}, out2 {e2:.2e}")
        assert e_bc < 1e-6 and e1 < 1e-6 and e2 < 1e-6
        results.append((bc, o1, o2))
    for a, b in zip(*results):
        assert torch.equal(a, b)
    # every output on its own gives the bits it has beside the others
    bc0, o10, o20 = results[0]
    bc = torch.full((B, ld_bc), 9.0, device="cuda")
    o1, o2 = p1.cuda(), p2.cuda()
    v = (T, T * ld, ld, 1)
    check(lib.buddy_colsum(P(y_row), *v, B, N, alpha, P(ws), P(bc), ld_bc, None, None, S()))
    check(lib.buddy_colsum(P(y_row), *v, B, N, alpha, P(ws), None, 0, P(o1), None, S()))
    check(lib.buddy_colsum(P(y_row), *v, B, N, alpha, P(ws), None, 0, None, P(o2), S()))
    torch.cuda.synchronize()
    assert torch.equal(bc, bc0) and torch.equal(o1, o10) and torch.equal(o2, o20)
    assert guard_intact(ws)


def test_basis_bias(lib):
    """output_layer.bias: K = 130 bins (three 64-column blocks, the last with 2 live columns) against sum_k colsum_k * bsum[c][k] in float64;
    1e-6 of sum_k |bsum[c][k]| sum |x_k|"""
    K, B, T = 130, 2, 2048 + 37
    g = torch.Generator(device="cpu").manual_seed(50)
    x = torch.randn(B * T, K, generator=g) + 1e-3
    bsum = torch.randn(2, K, generator=g, dtype=torch.float64)
    ref = (x.double().sum(dim=0)[None] * bsum).sum(dim=1)
    den = (x.double().abs().sum(dim=0)[None] * bsum.abs()).sum(dim=1)
    pre = torch.tensor([2.5, -1.25])
    out = pre.cuda()
    ws = workspace(lib.buddy_colsum_workspace(B, T, K))
    xc, bc = x.cuda(), bsum.cuda()
    check(lib.buddy_basis_bias(P(xc), K, B, T, bc.data_ptr(), P(ws), P(out), S()))
    torch.cuda.synchronize()
    e = float(((out.cpu().double() - (pre.double() + ref)).abs() / den).max())
    print(f"basis bias K={K}: {e:.2e}")
    assert e < 1e-6 and guard_intact(ws)


# ------------------------------------------------------------------------------------------------ GroupNorm gamma / beta
@pytest.mark.parametrize("da_mode", [0, 1, 2])
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("C,C0", [(32, 0), (96, 0), (384, 256)])
def test_gn_param_grads(lib, C, C0, silu, da_mode):
    """dgamma / dbeta of resample(act(GroupNorm(x))) under the cotangent da, against float64 autograd.  B = 2 and M = 1024 + 300 pixels (a ragged
    second chunk, the utterance boundary inside the first) on a 2 x 331 grid (odd W) for da_mode 0 and 2; da_mode 1 needs even H and W, so no grid
    has 662 pixels: 22 x 30 there (M = 1320, a second chunk of 296).  C = 96 leaves half of the second channel block empty; C = 384 reads two
    sources with padded rows.  1e-5 of sum |dz * xhat| and sum |dz|."""
    B, (H, W) = 2, (22, 30) if da_mode == 1 else (2, 331)
    G = groups_of(C)
    g = torch.Generator(device="cpu").manual_seed(60 + C + 2 * silu + da_mode)
    x = torch.randn(B, H, W, C, generator=g) * 1.5 + 0.3
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    Hd, Wd = (H // 2, W // 2) if da_mode == 1 else (2 * H, 2 * W) if da_mode == 2 else (H, W)
    da = torch.randn(B, Hd, Wd, C, generator=g)
    # float64 autograd of the composite (channels first for torch, as contiguous copies; no convolution here, so H and W keep their places)
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a = F.group_norm(x.double().permute(0, 3, 1, 2).contiguous(), G, gm, bt, eps=EPS)
    if silu:
        a = F.silu(a)
    if da_mode == 1:
        a = F.avg_pool2d(a, 2)
    elif da_mode == 2:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
    rg, rb = torch.autograd.grad(a, (gm, bt), da.double().permute(0, 3, 1, 2).contiguous())
    # the denominators: sum |dz * xhat| and sum |dz| with dz = da_eff * act'(z)
    st = gn_stats(x, G)
    mean_c = st[..., 0].double().repeat_interleave(C // G, dim=1)[:, None, None, :]
    rstd_c = st[..., 1].double().repeat_interleave(C // G, dim=1)[:, None, None, :]
    xh = (x.double() - mean_c) * rstd_c
    z = xh * gamma.double() + beta.double()
    sg = torch.sigmoid(z)
    d = da.double()
    if da_mode == 1:
        d = 0.25 * d.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    elif da_mode == 2:
        d = d.reshape(B, H, 2, W, 2, C).sum(dim=(2, 4))
    dz = d * (sg * (1 + z * (1 - sg))) if silu else d
    den_g, den_b = (dz * xh).abs().sum(dim=(0, 1, 2)), dz.abs().sum(dim=(0, 1, 2))

    if C0:
        x0, x1, ld0, ld1 = padded(x[..., :C0], C0 + 8), padded(x[..., C0:], C - C0 + 4), C0 + 8, C - C0 + 4
    else:
        x0, x1, ld0, ld1 = x.cuda(), None, C, 0
    pg, pb = prefill((C,), 8), prefill((C,), 9)
    dg, db = pg.cuda(), pb.cuda()
    assert lib.buddy_gn_param_grads_workspace(B, H, W, C) == 2 * C * 4
    ws = workspace(lib.buddy_gn_param_grads_workspace(B, H, W, C))
    stc, gmc, btc, dac = st.cuda(), gamma.cuda(), beta.cuda(), da.cuda()
    check(lib.buddy_gn_param_grads(P(x0), P(x1), C0, ld0, ld1, P(stc), P(gmc), P(btc), G, silu, P(dac), da_mode, B, H, W, C, P(ws), P(dg), P(db), S()))
    torch.cuda.synchronize()
    eg = float(((dg.cpu().double() - (pg.double() + rg)).abs() / den_g).max())
    eb = float(((db.cpu().double() - (pb.double() + rb)).abs() / den_b).max())
    print(f"gn param grads C={C} silu={silu} da_mode={da_mode}: dgamma {eg:.2e}, dbeta {eb:.2e}")
    assert eg < 1e-5 and eb < 1e-5 and guard_intact(ws)


# ------------------------------------------------------------------------------------------------ time-embedding MLP backward
@pytest.mark.parametrize("gb2", [0, 1])
@pytest.mark.parametrize("silu_in", [0, 1])
@pytest.mark.parametrize("N,K", [(128, 512), (512, 256), (96, 40)])
@pytest.mark.parametrize("B", [1, 8])
def test_linear_bwd(lib, B, N, K, silu_in, gb2):
    """backward of y = act(x) W^T + bias against float64 autograd: gw, gb (and gb2) accumulate, dx is overwritten; dy rows at ld_dy > N for the
    weight side (the per-utterance bias sums of every ResNet block share one buffer).  2e-5 of the abs-max."""
    ld_dy = N + 7
    g = torch.Generator(device="cpu").manual_seed(70 + B + N + K + silu_in)
    x, Wm, dy = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(B, N, generator=g)
    xd, Wd, bd = x.double().requires_grad_(True), Wm.double().requires_grad_(True), torch.zeros(N, dtype=torch.float64, requires_grad=True)
    y = F.linear(F.silu(xd) if silu_in else xd, Wd, bd)
    rx, rw, rb = torch.autograd.grad(y, (xd, Wd, bd), dy.double())
    pw, pb, pb2 = prefill((N, K), 10), prefill((N,), 11), prefill((N,), 12)
    gw, gb, g2 = pw.cuda(), pb.cuda(), pb2.cuda() if gb2 else None
    dx = torch.full((B, K), NAN, device="cuda")
    xc, dyc, dyp, Wc = x.cuda(), dy.cuda(), padded(dy, ld_dy), Wm.cuda()
    check(lib.buddy_linear_bwd_w(P(dyp), ld_dy, P(xc), silu_in, B, N, K, P(gw), P(gb), P(g2), S()))
    check(lib.buddy_linear_bwd_x(P(dyc), P(Wc), P(xc), silu_in, B, N, K, P(dx), S()))
    torch.cuda.synchronize()
    ew = float((gw.cpu().double() - (pw.double() + rw)).abs().max() / rw.abs().max())
    eb = float((gb.cpu().double() - (pb.double() + rb)).abs().max() / rb.abs().max())
    ex = float((dx.cpu().double() - rx).abs().max() / rx.abs().max())
    print(f"linear bwd B={B} N={N} K={K} silu_in={silu_in}: gw {ew:.2e}, gb {eb:.2e}, dx {ex:.2e}")
    assert ew < 2e-5 and eb < 2e-5 and ex < 2e-5
    if gb2:
        assert float((g2.cpu().double() - (pb2.double() + rb)).abs().max() / rb.abs().max()) < 2e-5
