"""GPU unit tests of the small fp32 kernels of the network (csrc/ops.hip) behind their own C-ABI entries: the 2-channel convolutions at the
network's entry and exit, the STFT glue, the pyramid pool / upsample, the time embedding, the materialised attention's softmax and transpose,
the 2 x 2 output mix and the axpy.  Every case compares with a plain float64 torch / numpy restatement of the same operation on the same
inputs, at the smallest shapes that reach each kernel branch (named per test).

Tensors are NHWC with H = time and W = frequency; the restatements hand torch (B, C, H, W), tap = 3 (dh + 1) + (dw + 1).

Gates, u = 2^-24:
  copies and permutations (reflect_pad with scale 1, transpose, up2 with a power-of-two scale)   bit equality
  sums of n products                  per element |out - ref| <= (n + 4) u A, A = the same operation in float64 on the absolute values of all
                                      operands (bias, add and prefill included): the forward bound of an fp32 sum of n terms in any order, with
                                      or without FMA; the 4 covers the roundings of the bias / add / prefill / scale terms.  (Each rounding adds
                                      2^-149 for a subnormal result, where fp32 has no relative accuracy: softmax tails around e^-90.)
  convolutions of more than 512 terms 2e-5 of the output's abs-max (the contraction gate of test_hip_kernels.py / test_hip_param_grad_kernels.py)
  outputs through sinf / cosf / expf / SiLU   per element max(the sum bound, 4 x e32), e32 = the largest error against float64 of the same
                                      operation done with torch's own fp32 ops on the device (never from the kernel under test)
Every output is prefilled with a known tensor and followed by a NaN guard that must stay intact; row padding and whatever a kernel must not
read hold NaN; accumulate = 1 is checked as out == prefill + result.  The measured figures are printed (pytest -s) as lines starting with
"small_ops" (profiles/small_ops_accuracy.txt)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 256           # floats behind every output that must stay untouched
U = 2.0 ** -24
TINY = 2.0 ** -149      # one rounding into the subnormal range is off by at most half of this
CONTRACTION = 2e-5


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


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def prefill(shape, seed=5):
    return torch.randn(shape, generator=gen(seed)) + 3.0


def guarded(t):
    """device copy of the float32 tensor t followed by a NaN guard; returns (flat buffer, view of t's shape)"""
    buf = torch.cat([t.reshape(-1).float(), torch.full((GUARD,), NAN)]).cuda()
    return buf, buf[:t.numel()].view(t.shape)


def guard_intact(buf):
    return bool(torch.isnan(buf[-GUARD:]).all())


def padded(x, ld):
    """rows of x (..., C) at a row stride of ld >= C floats; the padding columns hold NaN (no kernel may read them)"""
    C = x.shape[-1]
    buf = torch.full((x.numel() // C, ld), NAN)
    buf[:, :C] = x.reshape(-1, C)
    return buf.cuda()


def sum_bound(A, n):
    """(n + 4) (u A + 2^-149): the relative bound, plus the absolute error of a rounding whose result is subnormal (softmax tails)"""
    return (n + 4) * (U * A + TINY)


def sum_bound_ratio(out, ref, A, n):
    """max over the elements of |out - ref| / sum_bound; <= 1 passes"""
    err = (out.detach().cpu().double() - ref).abs()
    return float((err / sum_bound(A, n)).max())


def report(line):
    print("small_ops " + line)


# ------------------------------------------------------------------------------------------------ conv_c2in
def ref_c2in(x, w, bias, add, pre, taps):
    """float64: x (B,H,W,2), w [Cout][taps][2] -> (B,H,W,Cout)"""
    Cout, k = w.shape[0], 3 if taps == 9 else 1
    wt = w.reshape(Cout, k, k, 2).permute(0, 3, 1, 2)
    y = F.conv2d(x.permute(0, 3, 1, 2), wt, bias, padding=k // 2).permute(0, 2, 3, 1)
    if add is not None:
        y = y + add
    if pre is not None:
        y = y + pre
    return y


def run_c2in(lib, B, H, W, Cout, taps, bias_on, add_on, acc, ldpad, seed):
    """one launch; returns (sum-bound ratio, kernel error relative to the abs-max)"""
    g = gen(seed)
    x = torch.randn(B, H, W, 2, generator=g)
    w = torch.randn(Cout, taps, 2, generator=g)
    bias = torch.randn(Cout, generator=g) if bias_on else None
    add = torch.randn(B, H, W, Cout, generator=g) if add_on else None
    ldY, add_ld = Cout + (8 if ldpad else 0), Cout + (4 if ldpad else 0)
    pre = prefill((B * H * W, ldY), seed + 1)
    pre_live = pre[:, :Cout].reshape(B, H, W, Cout)
    d = lambda t: None if t is None else t.double()
    ref = ref_c2in(d(x), d(w), d(bias), d(add), d(pre_live) if acc else None, taps)
    a = lambda t: None if t is None else t.double().abs()
    A = ref_c2in(a(x), a(w), a(bias), a(add), a(pre_live) if acc else None, taps)
    buf, y = guarded(pre)
    xc, wc, bc = x.cuda(), w.cuda(), None if bias is None else bias.cuda()
    ac = None if add is None else padded(add, add_ld)
    check(lib.buddy_conv_c2in(P(xc), P(wc), P(bc), P(ac), add_ld if add_on else 0, P(y), ldY, B, H, W, Cout, taps, acc, S()))
    torch.cuda.synchronize()
    assert guard_intact(buf), "wrote behind the output"
    out = y.cpu()
    assert torch.equal(out[:, Cout:], pre[:, Cout:]), "wrote into the row padding of y"
    out = out[:, :Cout].reshape(B, H, W, Cout)
    return sum_bound_ratio(out, ref, A, 2 * taps), float((out.double() - ref).abs().max() / ref.abs().max())


C2IN_OPTS = [(1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 1, 0)]      # (bias, add, accumulate, padded rows)


@pytest.mark.parametrize("Cout", [12, 32, 128, 384, 512])
@pytest.mark.parametrize("taps", [1, 9])
def test_conv_c2in(lib, taps, Cout):
    """Cout = 12 and 384 (q = 3, 96: 256 % q != 0) run conv_c2in_kernel<taps>; Cout = 32, 128, 512 (q = 8, 32, 128) the register kernels:
    conv_c2in_reg_kernel<1>, and for 9 taps conv_c2in_reg4_kernel at W in {4, 8} and conv_c2in_reg_kernel<9> at W in {6, 7}.  H in {1, 3} (every
    tap row of H = 1 but the centre is outside), B = 2, bias / add (add_ld > Cout) / accumulate / ldY > Cout in four combinations."""
    worst = 0.0
    for H in (1, 3):
        for W in ((4, 8, 6, 7) if taps == 9 else (4, 7)):
            for i, (b, a, acc, ldp) in enumerate(C2IN_OPTS):
                r, e = run_c2in(lib, 2, H, W, Cout, taps, b, a, acc, ldp, seed=100 + Cout + 7 * H + W + i)
                worst = max(worst, r)
                assert r <= 1.0, f"H={H} W={W} bias={b} add={a} acc={acc} padded={ldp}: {r:.2f} of the sum bound (rel {e:.2e})"
    report(f"conv_c2in taps={taps} Cout={Cout}: worst {worst:.3f} of the (n + 4) u A bound, n = {2 * taps}")


@pytest.mark.parametrize("taps,H,W", [(1, 33, 63), (9, 33, 63), (9, 65, 256)])
def test_conv_c2in_capped_grid_second_trip(lib, taps, H, W):
    """Cout = 512 (2 pixels per block trip).  33 x 63 x 2 = 4158 pixels > 2048 x 2: the 2048-block grid of conv_c2in_reg_kernel<1> / <9> (W % 4 != 0)
    makes a second trip; 65 x 64 x 2 = 8320 groups of 4 > 4096 x 2: the 4096-block grid of conv_c2in_reg4_kernel does."""
    r, e = run_c2in(lib, 2, H, W, 512, taps, 1, 1, 1, 0, seed=200 + taps + W)
    report(f"conv_c2in capped grid taps={taps} H={H} W={W}: {r:.3f} of the sum bound, rel {e:.2e}")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------ conv_c2out
def ref_c2out(x, w, bias, up, pre, taps):
    """float64: x (B,H,W,Cin), w [taps][Cin][2] -> (B,H,W,2); up (B,H/2,W/2,2) is added nearest-upsampled"""
    Cin, k = x.shape[-1], 3 if taps == 9 else 1
    wt = w.reshape(k, k, Cin, 2).permute(3, 2, 0, 1)
    y = F.conv2d(x.permute(0, 3, 1, 2), wt, bias, padding=k // 2).permute(0, 2, 3, 1)
    if up is not None:
        y = y + up.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    if pre is not None:
        y = y + pre
    return y


class C2OutCase:
    """inputs and the float64 results (with and without prefill) of one Cin -> 2 case, computed once"""

    def __init__(self, B, H, W, Cin, taps, bias_on, up_on, ldpad, seed):
        self.B, self.H, self.W, self.Cin, self.taps = B, H, W, Cin, taps
        g = gen(seed)
        self.x = torch.randn(B, H, W, Cin, generator=g)
        self.w = torch.randn(taps, Cin, 2, generator=g) / math.sqrt(Cin)
        self.bias = torch.randn(2, generator=g) if bias_on else None
        self.up = torch.randn(B, H // 2, W // 2, 2, generator=g) if up_on else None
        self.ldX = Cin + (12 if ldpad else 0)
        self.pre = prefill((B, H, W, 2), seed + 1)
        d = lambda t: None if t is None else t.double()
        a = lambda t: None if t is None else t.double().abs()
        self.ref = {acc: ref_c2out(d(self.x), d(self.w), d(self.bias), d(self.up), d(self.pre) if acc else None, taps) for acc in (0, 1)}
        self.A = {acc: ref_c2out(a(self.x), a(self.w), a(self.bias), a(self.up), a(self.pre) if acc else None, taps) for acc in (0, 1)}
        self.dev = (padded(self.x, self.ldX), self.w.cuda(), None if self.bias is None else self.bias.cuda(), None if self.up is None else self.up.cuda())

    def run(self, lib, form, acc):
        buf, y = guarded(self.pre)
        xc, wc, bc, uc = self.dev
        check(lib.buddy_conv_c2out(P(xc), self.ldX, P(wc), P(bc), P(uc), P(y), self.B, self.H, self.W, self.Cin, self.taps, acc, form, S()))
        torch.cuda.synchronize()
        assert guard_intact(buf), "wrote behind the output"
        return y.clone()

    def judge(self, out, acc):
        """the gate's figure (<= 1 passes), the relative error, and which gate applied"""
        ref, n = self.ref[acc], self.taps * self.Cin
        rel = float((out.cpu().double() - ref).abs().max() / ref.abs().max())
        if n <= 512:
            return sum_bound_ratio(out, ref, self.A[acc], n), rel, "sum bound"
        return rel / CONTRACTION, rel, "2e-5 of abs-max"


@pytest.mark.parametrize("Cin", [12, 16, 32, 48, 64, 128, 256, 384, 512])
@pytest.mark.parametrize("taps", [1, 9])
def test_conv_c2out_lane_group(lib, taps, Cin):
    """form 0.  Cin = 16 ... 256 (4 ... 64 lanes per pixel) run conv_c2out_kernel<taps>; Cin = 384 and 512 (96 and 128 lanes: no aligned power-of-two
    group of one wave) run conv_c2out_wide_kernel<taps> with 32 and 64 lanes and 3 and 2 quads per lane, Cin = 12 and 48 (3 and 12 quads) with 1 and
    4 lanes and 3 quads each.  B = 2, 5 x 7 = 35 pixels per utterance: 70 is
    no multiple of the 64 ... 4 pixels of a block trip (nor of the wide kernel's 8 and 4).  One run with ldX > Cin (NaN padding), bias and
    accumulate; one plain; and on an even grid (6 x 10) one with up_add."""
    for (H, W, b, up, ldp, acc) in ((5, 7, 1, 0, 1, 1), (5, 7, 0, 0, 0, 0), (6, 10, 1, 1, 1, 0)):
        c = C2OutCase(2, H, W, Cin, taps, b, up, ldp, seed=300 + Cin + taps + H)
        r, rel, gate = c.judge(c.run(lib, 0, acc), acc)
        report(f"conv_c2out form 0 taps={taps} Cin={Cin} H={H} W={W} bias={b} up_add={up} acc={acc}: {r:.3f} of the gate ({gate}), rel {rel:.2e}")
        assert r <= 1.0


@pytest.mark.parametrize("Cin", [256, 384])
def test_conv_c2out_lane_group_capped_grid(lib, Cin):
    """more than 2048 groups: 2 x 65 x 127 = 16510 pixels in groups of 4 (Cin = 256, conv_c2out_kernel<1>) and of 8 (Cin = 384,
    conv_c2out_wide_kernel<1>): 4128 and 2064 groups on the 2048-block grid, a ragged last group at 256"""
    c = C2OutCase(2, 65, 127, Cin, 1, 1, 0, 0, seed=400 + Cin)
    r, rel, gate = c.judge(c.run(lib, 0, 1), 1)
    report(f"conv_c2out form 0 capped grid Cin={Cin}: {r:.3f} of the gate ({gate}), rel {rel:.2e}")
    assert r <= 1.0


@pytest.mark.parametrize("HW", [(7, 31), (8, 32), (9, 33)])
@pytest.mark.parametrize("Cin", [32, 96, 256, 512])
def test_conv_c2out_tiled_and_strip(lib, Cin, HW):
    """forms 1 (conv_c2out_tiled_kernel) and 2 (conv_c2out_strip_kernel), 9 taps, B = 2: less than one 8 x 32 tile, an exact tile, a tile plus a ragged
    edge in both directions (four blocks per utterance); 1, 3, 8 and 16 channel chunks.  Each against float64, and against form 0 on the same input
    (two fp32 sums of the same terms: within twice the gate).  up_add on the even grid, bias and ldX > Cin throughout."""
    H, W = HW
    c = C2OutCase(2, H, W, Cin, 9, 1, int(H % 2 == 0), 1, seed=500 + Cin + H)
    out0 = c.run(lib, 0, 1)
    outs = {1: c.run(lib, 1, 1), 2: c.run(lib, 2, 1)}
    for form, out in outs.items():
        r, rel, gate = c.judge(out, 1)
        d0 = float((out.double() - out0.double()).abs().max() / c.ref[1].abs().max())
        report(f"conv_c2out form {form} Cin={Cin} H={H} W={W}: {r:.3f} of the gate ({gate}), rel {rel:.2e}, against form 0 {d0:.2e}")
        assert r <= 1.0
        assert d0 <= 2 * CONTRACTION


# ------------------------------------------------------------------------------------------------ STFT glue
GEOS = [(16, 4), (126, 32)]


def lengths(n_fft, hop):
    """L = n_fft (a sample receives both reflections), n_fft + 1, a hop multiple and its neighbours, and one L with T = 1 + L / hop a multiple of 16"""
    return [n_fft, n_fft + 1, 8 * hop - 1, 8 * hop, 8 * hop + 1, 15 * hop + 1]


def frame_geo(n_fft, hop, L):
    T = 1 + L // hop
    Tp = (T + 15) // 16 * 16
    Lp = (L + n_fft + 8 + 3) // 4 * 4
    return T, Tp, Lp, n_fft // 2


def inv_envelope(n_fft, hop, Tp):
    """as the network computes it: the squared periodic Hann window overlap-added in float64, rounded to float, reciprocal, 0 below 1e-11"""
    env = np.zeros(n_fft + hop * (Tp - 1))
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    for t in range(Tp):
        env[t * hop:t * hop + n_fft] += w * w
    inv = np.zeros(env.size, dtype=np.float32)
    ok = env > 1e-11
    inv[ok] = (1.0 / env[ok].astype(np.float32).astype(np.float64)).astype(np.float32)
    return torch.from_numpy(inv)


def ref_reflect_pad(x, pad, Lp, scale, scale_b):
    """float64 (B, L) -> (B, Lp)"""
    xp = F.pad(x[:, None], (pad, pad), mode="reflect")[:, 0] * scale
    if scale_b is not None:
        xp = xp * scale_b[:, None]
    return F.pad(xp, (0, Lp - xp.shape[1]))


def ref_frames(xp, T, n_fft, hop):
    """frames[b][t][n] = xp[b][t hop + n], t < T: the framing the forward STFT GEMM reads"""
    return xp.unfold(1, n_fft, hop)[:, :T]


def ref_ola(frames, inv_env, L, pad, hop, xin, cskip, cout):
    """float64: frames (B, Tp, n_fft) -> (B, L)"""
    B, Tp, n_fft = frames.shape
    acc = torch.zeros(B, n_fft + hop * (Tp - 1), dtype=frames.dtype)
    for t in range(Tp):
        acc[:, t * hop:t * hop + n_fft] = acc[:, t * hop:t * hop + n_fft] + frames[:, t]
    y = (acc * inv_env)[:, pad:pad + L]
    if xin is not None:
        y = cskip[:, None] * xin + cout[:, None] * y
    return y


@pytest.mark.parametrize("scaled", [0, 1])
@pytest.mark.parametrize("n_fft,hop", GEOS)
def test_reflect_pad(lib, n_fft, hop, scaled):
    """reflect_pad_kernel, B = 2: bit equality with F.pad(mode="reflect") at scale 1 without per-row scales, the sum bound (n = 1) with scale 0.7 and
    per-row scales; the tail [L + 2 pad, Lp) must be zero"""
    for L in lengths(n_fft, hop):
        T, Tp, Lp, pad = frame_geo(n_fft, hop, L)
        g = gen(600 + L)
        x = torch.randn(2, L, generator=g)
        sb = torch.tensor([1.7, -0.6]) if scaled else None
        scale = 0.7 if scaled else 1.0
        ref = ref_reflect_pad(x.double(), pad, Lp, float(np.float32(scale)), None if sb is None else sb.double())
        buf, xp = guarded(prefill((2, Lp)))
        xc, sc = x.cuda(), None if sb is None else sb.cuda()
        check(lib.buddy_reflect_pad(P(xc), P(xp), 2, L, pad, Lp, scale, P(sc), S()))
        torch.cuda.synchronize()
        assert guard_intact(buf)
        assert bool((xp[:, L + 2 * pad:] == 0).all()), "tail of xp not zero"
        if scaled:
            assert sum_bound_ratio(xp, ref, ref.abs(), 1) <= 1.0, f"L={L}"
        else:
            assert torch.equal(xp.cpu().double(), ref), f"L={L}"


@pytest.mark.parametrize("edm", [0, 1])
@pytest.mark.parametrize("n_fft,hop", GEOS)
def test_ola_and_adjoint(lib, n_fft, hop, edm):
    """ola_kernel and ola_adj_kernel over all Tp frames of the 16-padded spectrogram (frames T .. Tp - 1 included), frames at ldF > n_fft with NaN
    padding, with and without xin / cskip / cout, B = 2.  ola against the float64 overlap-add (sum bound, n = ceil(n_fft / hop) terms); ola_adj
    against float64 autograd of that restatement (n = 1) with its row padding written as 0; and <ola(F), g> = <F, ola_adj(g)> between the two
    kernels, inner products in float64 on the host, to (n + 4) u of sum |terms|."""
    B, ldF, n = 2, n_fft + 6, -(-n_fft // hop)
    for L in lengths(n_fft, hop):
        T, Tp, Lp, pad = frame_geo(n_fft, hop, L)
        g = gen(700 + L + edm)
        fr = torch.randn(B, Tp, n_fft, generator=g)
        cot = torch.randn(B, L, generator=g)
        xin = torch.randn(B, L, generator=g) if edm else None
        cskip, cout = (torch.tensor([0.8, -0.3]), torch.tensor([0.45, 1.6])) if edm else (None, None)
        inv = inv_envelope(n_fft, hop, Tp)
        d = lambda t: None if t is None else t.double()
        a = lambda t: None if t is None else t.double().abs()
        frd = fr.double().requires_grad_(True)
        ref = ref_ola(frd, inv.double(), L, pad, hop, d(xin), d(cskip), d(cout))
        gfr, = torch.autograd.grad(ref, frd, cot.double())
        A = ref_ola(a(fr), inv.double(), L, pad, hop, a(xin), a(cskip), a(cout))
        frc, invc, cotc = padded(fr, ldF), inv.cuda(), cot.cuda()
        xc, ck, co = (None if t is None else t.cuda() for t in (xin, cskip, cout))
        buf, y = guarded(prefill((B, L)))
        check(lib.buddy_ola(P(frc), ldF, Tp, n_fft, hop, P(invc), P(y), B, L, pad, P(xc), P(ck), P(co), S()))
        bufa, fa = guarded(prefill((B, Tp, ldF)))
        check(lib.buddy_ola_adj(P(cotc), B, L, pad, Tp, n_fft, hop, P(invc), P(co), P(fa), ldF, S()))
        torch.cuda.synchronize()
        assert guard_intact(buf) and guard_intact(bufa)
        r = sum_bound_ratio(y, ref.detach(), A, n)
        assert r <= 1.0, f"ola L={L}: {r:.2f} of the sum bound"
        assert bool((fa[:, :, n_fft:] == 0).all()), "ola_adj: row padding not zero"
        ra = sum_bound_ratio(fa[:, :, :n_fft], gfr, gfr.abs(), 1)
        assert ra <= 1.0, f"ola_adj L={L}: {ra:.2f} of the sum bound"
        # <A F, g> = <F, A^T g> for the linear part (without the xin term): kernel outputs, float64 inner products
        lin = y.cpu().double() - (cskip.double()[:, None] * xin.double() if edm else 0.0)
        lhs, rhs = (lin * cot.double()).sum(), (fr.double() * fa[:, :, :n_fft].cpu().double()).sum()
        scale = (A * cot.double().abs()).sum() + (fr.double().abs() * fa[:, :, :n_fft].cpu().double().abs()).sum()
        assert abs(float(lhs - rhs)) <= (n + 4) * U * float(scale), f"adjoint identity L={L}"


@pytest.mark.parametrize("edm", [0, 1])
@pytest.mark.parametrize("n_fft,hop", GEOS)
def test_unpad_adj(lib, n_fft, hop, edm):
    """unpad_adj_kernel: the adjoint in x of frames(reflect_pad(x)) (T frames, rows at ldF > n_fft with NaN padding), scale and per-row scales, plus
    cskip * g_out; B = 2.  At L = n_fft sample n_fft / 2 is in both reflection ranges.  Against float64 autograd of the forward restatement (sum
    bound over the 3 ceil(n_fft / hop) terms a sample can receive), and <frames(reflect_pad(x)), G> = <x, unpad_adj(G)> with the reflect_pad KERNEL's
    output framed on the host."""
    B, ldF, n = 2, n_fft + 2, 3 * -(-n_fft // hop)
    for L in lengths(n_fft, hop):
        T, Tp, Lp, pad = frame_geo(n_fft, hop, L)
        g = gen(800 + L + edm)
        x = torch.randn(B, L, generator=g)
        G = torch.randn(B, T, n_fft, generator=g)
        sb = torch.tensor([1.7, -0.6]) if edm else None
        gout, cskip = (torch.randn(B, L, generator=g), torch.tensor([0.8, -0.3])) if edm else (None, None)
        scale = 0.7 if edm else 1.0
        s64 = float(np.float32(scale))

        def fwd(xx, GG, sbb):
            return (ref_frames(ref_reflect_pad(xx, pad, Lp, s64, sbb), T, n_fft, hop) * GG).sum()
        xd = x.double().requires_grad_(True)
        ref, = torch.autograd.grad(fwd(xd, G.double(), None if sb is None else sb.double()), xd)
        xa = torch.ones(B, L, dtype=torch.float64, requires_grad=True)
        A, = torch.autograd.grad(fwd(xa, G.double().abs(), None if sb is None else sb.double().abs()), xa)
        if edm:
            ref = ref + cskip.double()[:, None] * gout.double()
            A = A + cskip.double().abs()[:, None] * gout.double().abs()
        Gc, xc = padded(G, ldF), x.cuda()
        sc, gc, ck = (None if t is None else t.cuda() for t in (sb, gout, cskip))
        buf, dx = guarded(prefill((B, L)))
        check(lib.buddy_unpad_adj(P(Gc), ldF, T, n_fft, hop, B, L, pad, scale, P(sc), P(gc), P(ck), P(dx), S()))
        bufp, xp = guarded(prefill((B, Lp)))
        check(lib.buddy_reflect_pad(P(xc), P(xp), B, L, pad, Lp, scale, P(sc), S()))
        torch.cuda.synchronize()
        assert guard_intact(buf) and guard_intact(bufp)
        r = sum_bound_ratio(dx, ref, A, n)
        assert r <= 1.0, f"unpad_adj L={L}: {r:.2f} of the sum bound"
        lin = dx.cpu().double() - (cskip.double()[:, None] * gout.double() if edm else 0.0)
        fk = ref_frames(xp.cpu().double(), T, n_fft, hop)
        lhs, rhs = (fk * G.double()).sum(), (x.double() * lin).sum()
        scl = (fk.abs() * G.double().abs()).sum() + (x.double().abs() * A).sum()
        assert abs(float(lhs - rhs)) <= (n + 4) * U * float(scl), f"adjoint identity L={L}"


# ------------------------------------------------------------------------------------------------ pool2, up2_acc
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("HW", [(2, 2), (6, 10)])
@pytest.mark.parametrize("C", [2, 4, 12, 32])
def test_pool2_and_up2(lib, C, HW, acc):
    """pool2_c2_kernel (C = 2) and pool2_kernel (C = 4, 12, 32), up2_acc_kernel at every C; B = 2 (a box or a source pixel of the wrong utterance
    changes the result), scale != 1.  pool2: F.avg_pool2d x 4 x scale, sum bound with n = 4.  up2_acc: repeat_interleave; bit equality with the
    power-of-two scale 0.25 when it overwrites, the sum bound (n = 1) with scale 0.3 and when it accumulates."""
    B, (H, W) = 2, HW
    g = gen(900 + C + H)
    x = torch.randn(B, H, W, C, generator=g)
    pre = prefill((B, H // 2, W // 2, C))
    scale = 0.3
    s64 = float(np.float32(scale))

    def pool(t, p):
        y = F.avg_pool2d(t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * 4.0 * s64
        return y + p if acc else y
    ref, A = pool(x.double(), pre.double()), pool(x.double().abs(), pre.double().abs())
    buf, y = guarded(pre)
    xc = x.cuda()
    check(lib.buddy_pool2(P(xc), P(y), B, H, W, C, scale, acc, S()))
    torch.cuda.synchronize()
    assert guard_intact(buf)
    assert sum_bound_ratio(y, ref, A, 4) <= 1.0

    src = torch.randn(B, H // 2, W // 2, C, generator=g)
    preu = prefill((B, H, W, C), 6)
    sc = src.cuda()
    for scale in (0.25, 0.3):
        s64 = float(np.float32(scale))
        up = src.double().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) * s64
        ref = up + preu.double() if acc else up
        buf, y = guarded(preu)
        check(lib.buddy_up2_acc(P(sc), P(y), B, H // 2, W // 2, C, scale, acc, S()))
        torch.cuda.synchronize()
        assert guard_intact(buf)
        if scale == 0.25 and not acc:
            assert torch.equal(y.cpu().double(), ref)
        else:
            assert sum_bound_ratio(y, ref, up.abs() + (preu.double().abs() if acc else 0.0), 1) <= 1.0


# ------------------------------------------------------------------------------------------------ fourier, linear
@pytest.mark.parametrize("nf", [32, 128])
def test_fourier(lib, nf):
    """fourier_kernel, B = 3: the phase in float32 with the kernel's product order (numpy float32), sin and cos of it in float64; Wf at the
    reference's scale 16, so phases reach hundreds of radians.  max(sum bound with n = 1, 4 x e32), e32 from torch.sin / torch.cos in fp32 on
    the device on the same float32 phases."""
    B = 3
    g = gen(1000 + nf)
    cn = torch.tensor([-1.9, 0.37, 1.1])
    Wf = torch.randn(nf, generator=g) * 16.0
    ph = ((cn.numpy()[:, None] * Wf.numpy()[None, :]) * np.float32(2.0)) * np.float32(3.14159265358979323846)
    assert ph.dtype == np.float32
    ph64 = torch.from_numpy(ph.astype(np.float64))
    ref = torch.cat([torch.sin(ph64), torch.cos(ph64)], dim=1)
    phc = torch.from_numpy(ph).cuda()
    t32 = torch.cat([torch.sin(phc), torch.cos(phc)], dim=1).cpu().double()
    e32 = float((t32 - ref).abs().max())
    buf, out = guarded(prefill((B, 2 * nf)))
    cc, wc = cn.cuda(), Wf.cuda()
    check(lib.buddy_fourier(P(cc), P(wc), P(out), B, nf, S()))
    torch.cuda.synchronize()
    assert guard_intact(buf)
    err = (out.cpu().double() - ref).abs()
    gate = torch.maximum(sum_bound(ref.abs(), 1), torch.full_like(ref, 4 * e32))
    report(f"fourier nf={nf}: kernel {float(err.max()):.2e}, torch fp32 (e32) {e32:.2e}, max |phase| {float(np.abs(ph).max()):.0f}")
    assert bool((err <= gate).all())


@pytest.mark.parametrize("silu_in", [0, 1])
@pytest.mark.parametrize("N", [1, 5, 512])
@pytest.mark.parametrize("K", [64, 100, 512])
def test_linear(lib, K, N, silu_in):
    """linear_kernel, B = 3 (B N % 4 != 0 at N = 1, 5: a last block of one or three live waves); K = 64 one trip per lane, 100 a ragged second, 512
    eight; with a bias and without.  Sum bound with n = K; with SiLU on the input max(that, 4 x e32), e32 from F.linear(F.silu(x)) in fp32 on the
    device."""
    B = 3
    g = gen(1100 + K + N)
    x, Wm, bias = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
    xc, wc, bc = x.cuda(), Wm.cuda(), bias.cuda()
    for b64, bdev in ((bias.double(), bc), (None, None)):
        act = F.silu(x.double()) if silu_in else x.double()
        ref = F.linear(act, Wm.double(), b64)
        A = F.linear(act.abs(), Wm.double().abs(), None if b64 is None else b64.abs())
        e32 = 0.0
        if silu_in:
            e32 = float((F.linear(F.silu(xc), wc, bdev).cpu().double() - ref).abs().max())
        buf, y = guarded(prefill((B, N)))
        check(lib.buddy_linear(P(xc), P(wc), P(bdev), P(y), B, K, N, silu_in, S()))
        torch.cuda.synchronize()
        assert guard_intact(buf)
        err = (y.cpu().double() - ref).abs()
        gate = torch.maximum(sum_bound(A, K), torch.full_like(ref, 4 * e32))
        if silu_in:
            report(f"linear K={K} N={N} silu_in=1 bias={int(b64 is not None)}: kernel {float(err.max()):.2e}, torch fp32 (e32) {e32:.2e}")
        assert bool((err <= gate).all())


# ------------------------------------------------------------------------------------------------ softmax, transpose
@pytest.mark.parametrize("rows", [1, 5, 8])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 1000])
def test_softmax_rows_and_backward(lib, cols, rows):
    """softmax_rows_kernel and softmax_bwd_rows_kernel: one wave per row, four rows per block (rows = 1, 5: a block with idle waves; 8: two full
    blocks); cols = 1, 63 (idle lanes), 64, 65 (a second trip of one lane), 1000.  Two inputs: unit normal, and entries spread over +-80 with one of 95
    in every row (expf(95) overflows fp32: without the max subtraction that entry is inf / inf).  Forward: max(sum bound with n = cols, 4 x e32), e32 from torch.softmax in fp32 on the device.  Backward
    dS = P (dP - sum P dP): the sum bound with n = cols against float64 on the same float32 P."""
    g = gen(1200 + cols + rows)
    for spread in (1.0, 80.0):
        s = torch.randn(rows, cols, generator=g)
        if spread > 1:
            s = (torch.rand(rows, cols, generator=g) * 2 - 1) * spread
            s[torch.arange(rows), torch.arange(rows) % cols] = 95.0
        ref = torch.softmax(s.double(), dim=1)
        sc = s.cuda()
        e32 = float((torch.softmax(sc, dim=1).cpu().double() - ref).abs().max())
        buf, out = guarded(s)
        check(lib.buddy_softmax_rows(P(out), rows, cols, S()))
        torch.cuda.synchronize()
        assert guard_intact(buf)
        err = (out.cpu().double() - ref).abs()
        gate = torch.maximum(sum_bound(ref, cols), torch.full_like(ref, 4 * e32))
        report(f"softmax rows={rows} cols={cols} spread={spread:g}: kernel {float(err.max()):.2e}, torch fp32 (e32) {e32:.2e}")
        assert bool(torch.isfinite(out).all())
        assert bool((err <= gate).all())
        p = out.cpu()
        dP = torch.randn(rows, cols, generator=g)
        dot = (p.double() * dP.double()).sum(dim=1, keepdim=True)
        refb = p.double() * (dP.double() - dot)
        Ab = p.double() * (dP.double().abs() + (p.double() * dP.double().abs()).sum(dim=1, keepdim=True))
        pc = p.cuda()
        bufb, d = guarded(dP)
        check(lib.buddy_softmax_bwd_rows(P(pc), P(d), rows, cols, S()))
        torch.cuda.synchronize()
        assert guard_intact(bufb)
        assert sum_bound_ratio(d, refb, Ab, cols) <= 1.0


@pytest.mark.parametrize("n", [32, 96])
def test_transpose_sq(lib, n):
    """transpose_sq_kernel: one 32 x 32 tile and 3 x 3 tiles, batch 3, bit for bit"""
    x = torch.randn(3, n, n, generator=gen(1300 + n))
    buf, out = guarded(prefill((3, n, n)))
    xc = x.cuda()
    check(lib.buddy_transpose_sq(P(xc), P(out), 3, n, S()))
    torch.cuda.synchronize()
    assert guard_intact(buf)
    assert torch.equal(out.cpu(), x.transpose(1, 2).contiguous())


# ------------------------------------------------------------------------------------------------ mix2, axpy
def mix2_ref(x, w, b, pre, transpose):
    y = x @ (w if transpose else w.t())
    if b is not None and not transpose:
        y = y + b
    return y + pre if pre is not None else y


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("npix", [1, 257, 65536 * 256 + 3])
def test_mix2(lib, npix, transpose, acc):
    """mix2_kernel: y = x W^T + b (the output layer) and y = x W (its input-VJP, which ignores the bias); npix = 1, 257 (a second block of one
    pixel) and three pixels more than the 65536-block grid covers in one trip.  Sum bound with n = 2.  The float64 restatement of the big case
    runs on the device."""
    big = npix > 1 << 20
    g = gen(1400 + (npix % 1000) + transpose)
    w, b = torch.randn(2, 2, generator=g), torch.randn(2, generator=g)
    wc, bc = w.cuda(), b.cuda()
    if big:
        dg = torch.Generator(device="cuda").manual_seed(7)
        xc = torch.randn(npix, 2, device="cuda", generator=dg)
        pre = torch.randn(npix, 2, device="cuda", generator=dg) + 3.0
        buf = torch.cat([pre.reshape(-1), torch.full((GUARD,), NAN, device="cuda")])
        y = buf[:2 * npix].view(npix, 2)
        dev = "cuda"
    else:
        x, prec = torch.randn(npix, 2, generator=g), prefill((npix, 2))
        xc, pre = x.cuda(), prec
        buf, y = guarded(prec)
        dev = "cpu"
    for bias in ((bc, None) if not big else (bc,)):
        if bias is None:
            y.copy_(pre)
        check(lib.buddy_mix2(P(xc), P(wc), P(bias), P(y), npix, transpose, acc, S()))
        torch.cuda.synchronize()
        assert guard_intact(buf)
        xd, wd = xc.to(dev).double(), w.to(dev).double()
        bd = None if bias is None else b.to(dev).double()
        pd = pre.to(dev).double() if acc else None
        ref = mix2_ref(xd, wd, bd, pd, transpose)
        A = mix2_ref(xd.abs(), wd.abs(), None if bd is None else bd.abs(), None if pd is None else pd.abs(), transpose)
        err = (y.to(dev).double() - ref).abs()
        assert bool((err <= sum_bound(A, 2)).all())


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", [4, 1028])
def test_axpy(lib, n, acc):
    """axpy_kernel: one float4, and 257 of them (a second block of one thread); dst = alpha src [+ dst], sum bound with n = 1"""
    g = gen(1500 + n)
    src, pre, alpha = torch.randn(n, generator=g), prefill((n,)), -0.37
    a64 = float(np.float32(alpha))
    ref = a64 * src.double() + (pre.double() if acc else 0.0)
    A = abs(a64) * src.double().abs() + (pre.double().abs() if acc else 0.0)
    buf, dst = guarded(pre)
    sc = src.cuda()
    check(lib.buddy_axpy(P(dst), P(sc), alpha, n, acc, S()))
    torch.cuda.synchronize()
    assert guard_intact(buf)
    assert sum_bound_ratio(dst, ref, A, 1) <= 1.0
