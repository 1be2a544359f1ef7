"""gemm = "f16": the opt-in fast mode of the batched Winograd-domain GEMMs (csrc/wgemm16.hip, w6_input_f16_kernel in csrc/wino6.hip).  V is stored as
ONE f16 term with a power of two per tile, U as one f16 term with a power of two per position, one f16 MFMA per 16 k (format: include/buddy_hip.h,
buddy_gemm_winograd_domain_f16).  Against float64: the GEMM on its own, one whole convolution, one denoiser evaluation + VJP at full size; and the
properties the project asks of every arithmetic (bit-for-bit reproducible, batch-independent, per-handle)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from buddy_amd import _lib
    return _lib.require_gpu()


def P(t):
    return None if t is None else t.data_ptr()


def S():
    return torch.cuda.current_stream().cuda_stream


def _pow2_exponent(m):
    """141 - clamp(exponent field of m, 15, 253): m * 2^e in [2^14, 2^15) (the documented rule for vexp and the weights' per-position scale)"""
    f = (np.asarray(m, dtype=np.float32).view(np.uint32) >> 23) & 0xFF
    return 141 - np.clip(f.astype(np.int64), 15, 253)


@pytest.mark.parametrize("Cout,Cin,Pn", [(128, 128, 16), (256, 256, 16), (128, 384, 16), (256, 512, 16), (256, 96, 12)])
def test_gemm_f16_vs_float64(lib, Cout, Cin, Pn):
    """M[p] = 2^-e . V16[p] . U1[p]^T . u_inv[p] with operands built in numpy in the documented format; per-tile magnitudes 2^-20 .. 2^10, some all-zero
    tiles, an asymmetric U (a row / column swap cannot pass).  Same f16 operands in float64: only fp32 accumulation is left (<= 2e-6 of each row's
    abs-max); unrounded operands in float64: the price of the format (<= 4e-3).  12 positions: the grid with one position per blockIdx.z."""
    from buddy_amd import _lib
    rs = np.random.RandomState(Cout + 7 * Cin)
    tiles = 300                 # not a multiple of the 256-row workgroup; Pn = 12: the grid is not folded over positions (P % 8 != 0), 96 = 3 K-stages
    mag = 2.0 ** rs.uniform(-20, 10, size=tiles)
    mag[[0, 17, 299]] = 0.0
    V = (rs.standard_normal((Pn, tiles, Cin)) * mag[None, :, None]).astype(np.float32)
    U = (rs.standard_normal((Pn, Cout, Cin)) * np.linspace(0.5, 2.0, Cin)[None, None, :] + 0.1 * np.arange(Cout)[None, :, None] / Cout)
    U = (U * 2.0 ** rs.uniform(-6, 3, size=(Pn, 1, 1))).astype(np.float32)
    e = _pow2_exponent(np.abs(V).max(axis=(0, 2)))
    assert np.all(e[mag == 0] == 126)
    V16 = (V.astype(np.float64) * 2.0 ** e[None, :, None]).astype(np.float16)
    eu = _pow2_exponent(np.abs(U).max(axis=(1, 2)))
    U1 = (U.astype(np.float64) * 2.0 ** eu[:, None, None]).astype(np.float16)
    nbytes = lib.buddy_wgemm_f16_packed_bytes(Pn, Cout, Cin)
    assert nbytes > 0
    Ud = torch.from_numpy(U).cuda()
    img = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.buddy_wgemm_f16_pack_weights(P(Ud), P(img), Pn, Cout, Cin, S()))
    Vd = torch.from_numpy(V16).cuda()
    ed = torch.from_numpy(e.astype(np.int8)).cuda()
    M = torch.full((Pn, tiles, Cout), float("nan"), device="cuda")
    _lib.check(lib.buddy_gemm_winograd_domain_f16(P(Vd), P(ed), P(img), P(M), tiles, Cout, Cin, Pn, S()))
    torch.cuda.synchronize()
    inv = img[Pn * Cout * Cin * 2:Pn * Cout * Cin * 2 + 4 * Pn].view(torch.float32).cpu().numpy()
    assert np.array_equal(inv, (2.0 ** -eu).astype(np.float32)), "per-position inverse scales"
    Mh = M.cpu().numpy().astype(np.float64)
    ref_q = np.einsum("ptc,pnc->ptn", V16.astype(np.float64) * 2.0 ** -e[None, :, None], U1.astype(np.float64) * 2.0 ** -eu[:, None, None])
    ref = np.einsum("ptc,pnc->ptn", V.astype(np.float64), U.astype(np.float64))
    amax_q = np.abs(ref_q).max(axis=2, keepdims=True)
    amax = np.abs(ref).max(axis=2, keepdims=True)
    assert np.all(np.isfinite(Mh))
    assert np.all(Mh[:, mag == 0, :] == 0.0)
    live = (mag > 0)
    eq = float((np.abs(Mh - ref_q)[:, live] / amax_q[:, live]).max())
    er = float((np.abs(Mh - ref)[:, live] / amax[:, live]).max())
    print(f"f16 GEMM {tiles} x {Cout} x {Cin} x {Pn}: vs float64 of the f16 operands {eq:.2e}, vs float64 of the unrounded operands {er:.2e} (of each row's abs-max)")
    assert eq <= 2e-6
    assert er <= 4e-3


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 66, 40, 128, 128), (1, 33, 20, 256, 256)])
def test_conv3x3_winograd6_f16_vs_float64_and_v_format(lib, B, H, W, Cin, Cout):
    """One whole F(6x6,3x3) convolution with the f16 GEMM (level-0 and 256-channel shapes; H, W not multiples of 6: overhanging, zero-padded tiles)
    against a float64 direct convolution; and V16 with its exponents equals the fp32 V of the same transform (the fp32 path's scratch) times 2^e,
    rounded to nearest f16, bit for bit -- the f16 form runs the same fp32 transform arithmetic (shared column phase, same row phase) before one rounding."""
    from buddy_amd import _lib
    g = torch.Generator(device="cpu").manual_seed(B * 100 + Cin + Cout)
    x = (torch.randn(B, Cin, H, W, generator=g) * 0.7 + 0.1)
    x[:, :, :6, :6] = 0.0                                       # the first tile of every utterance is all zero
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g).cuda()
    ref = F.conv2d(x.double(), w.double(), b.cpu().double(), padding=1)
    wt = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().numpy()
    U = np.empty(64 * Cin * Cout, dtype=np.float32)
    _lib.check(lib.buddy_winograd6_transform_weights(wt.ctypes.data, Cout, Cin, U.ctypes.data))
    Ud = torch.from_numpy(U).cuda()
    img = torch.empty(lib.buddy_wgemm_f16_packed_bytes(64, Cout, Cin), dtype=torch.uint8, device="cuda")
    _lib.check(lib.buddy_wgemm_f16_pack_weights(P(Ud), P(img), 64, Cout, Cin, S()))
    xn = x.permute(0, 2, 3, 1).contiguous().cuda()
    tiles = B * ((H + 5) // 6) * ((W + 5) // 6)
    y16 = torch.full((B, H, W, Cout), float("nan"), device="cuda")
    s16 = torch.empty(64 * tiles * (Cin + Cout), device="cuda")
    _lib.check(lib.buddy_conv3x3_winograd6_f16(P(xn), P(img), P(b), P(y16), P(s16), B, H, W, Cin, Cout, S()))
    y32 = torch.empty(B, H, W, Cout, device="cuda")
    s32 = torch.empty(64 * tiles * (Cin + Cout), device="cuda")
    _lib.check(lib.buddy_conv3x3_winograd6(P(xn), P(Ud), P(b), P(y32), P(s32), B, H, W, Cin, Cout, S()))
    torch.cuda.synchronize()
    y = y16.permute(0, 3, 1, 2).double().cpu()
    assert torch.isfinite(y).all()
    e16 = float((y - ref).abs().max() / ref.abs().max())
    e32 = float((y32.permute(0, 3, 1, 2).double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"F(6x6,3x3) {B}x{H}x{W} {Cin}->{Cout}: f16 GEMM {e16:.2e}, fp32 path {e32:.2e} of the abs-max vs float64")
    assert e16 < 1.5e-2                                         # measured 7.2e-3 (2 x 66 x 40, 128 -> 128): F(6x6,3x3) amplifies the 2^-12 operand rounding
    n = 64 * tiles * Cin
    V16 = s16.view(torch.int16)[:n].view(torch.float16).cpu().numpy().reshape(64, tiles, Cin)
    vexp = s16.view(torch.int8)[2 * n:2 * n + tiles].cpu().numpy().astype(np.int64)
    V32 = s32[:n].cpu().numpy().reshape(64, tiles, Cin).astype(np.float64)
    assert np.array_equal(vexp, _pow2_exponent(np.abs(V32).max(axis=(0, 2)).astype(np.float32)))
    want = (V32 * 2.0 ** vexp[None, :, None]).astype(np.float16)
    assert np.array_equal(V16.view(np.uint16), want.view(np.uint16))


def _tiles(B, H, W, up):
    ax = (lambda n: n // 7 + 1) if up == 1 else (lambda n: (n + 6) // 7) if up == 2 else (lambda n: (n + 5) // 6)
    return B * ax(H) * ax(W)


def _pack16(lib, U, Co, Ci):
    from buddy_amd import _lib
    img = torch.empty(lib.buddy_wgemm_f16_packed_bytes(64, Co, Ci), dtype=torch.uint8, device="cuda")
    assert img.numel() > 0
    _lib.check(lib.buddy_wgemm_f16_pack_weights(P(U), P(img), 64, Co, Ci, S()))
    return img


def _check_v(s16, s32, tiles, K):
    """V16 . 2^-vexp of the f16 form == the fp32 form's V (same launch, fp32 arithmetic) rounded to nearest f16 after the scale, bit for bit; vexp by the
    documented rule from that V"""
    n = 64 * tiles * K
    V16 = s16.view(torch.int16)[:n].cpu().numpy().view(np.uint16).reshape(64, tiles, K)
    vexp = s16.view(torch.int8)[2 * n:2 * n + tiles].cpu().numpy().astype(np.int64)
    V32 = s32[:n].cpu().numpy().reshape(64, tiles, K).astype(np.float64)
    assert np.array_equal(vexp, _pow2_exponent(np.abs(V32).max(axis=(0, 2)).astype(np.float32))), "per-tile exponents"
    assert np.array_equal(V16, (V32 * 2.0 ** vexp[None, :, None]).astype(np.float16).view(np.uint16)), "V16 != f16_rn(V . 2^e)"


def _gn_stats(x, G):
    """(mean, rstd) per (utterance, group) of an NHWC tensor, float64 -> float32 [B][G][2]"""
    B, C = x.shape[0], x.shape[-1]
    xg = x.double().reshape(B, -1, G, C // G)
    mean = xg.mean(dim=(1, 3)); rstd = 1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False) + 1e-6)
    return torch.stack([mean, rstd], dim=-1).float().contiguous()


# The four launch forms of the network's F(6x6,3x3) convolutions with the f16 GEMM (buddy_*_winograd6_f16) against float64, each beside its fp32 form on the
# same inputs for the V format (all-zero tiles: test_conv3x3_winograd6_f16_vs_float64_and_v_format -- the GroupNorm forms have none).  K = 512 / 1024 cases
# run the input transform's second walk over channel blocks beyond those it keeps in registers (2; 1 for the GroupNorm-backward forms), and the concatenated view.
@pytest.mark.parametrize("B,H,W,C0,C1,Cout", [(2, 40, 30, 128, 0, 128), (1, 20, 14, 256, 256, 256)])
def test_gn_conv3x3_winograd6_f16(lib, B, H, W, C0, C1, Cout):
    from buddy_amd import _lib
    Cin, silu = C0 + C1, 1
    G = min(Cin // 4, 32)
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + Cin + Cout + 301)
    x = (torch.randn(B, H, W, Cin, generator=g) * 1.5 + 0.3).cuda()
    gamma = (1 + 0.2 * torch.randn(Cin, generator=g)).cuda(); beta = (0.2 * torch.randn(Cin, generator=g)).cuda()
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g).cuda()
    z = F.silu(F.group_norm(x.permute(0, 3, 1, 2).double(), G, gamma.double(), beta.double(), eps=1e-6))
    ref = F.conv2d(z, w.cuda().double(), b.double(), padding=1).permute(0, 2, 3, 1)
    wt = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().numpy()
    U = np.empty(64 * Cin * Cout, dtype=np.float32)
    _lib.check(lib.buddy_winograd6_transform_weights(wt.ctypes.data, Cout, Cin, U.ctypes.data))
    Ud = torch.from_numpy(U).cuda()
    img = _pack16(lib, Ud, Cout, Cin)
    x0 = x[..., :C0].contiguous(); x1 = x[..., C0:].contiguous() if C1 else None
    tiles = _tiles(B, H, W, 0)
    out = {}
    for f16 in (0, 1):
        y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
        scratch = torch.empty(64 * tiles * (Cin + Cout), device="cuda")
        stats = torch.empty(B, G, 2, device="cuda")
        stat_scratch = torch.empty(B * 256 * 1024 * 2, dtype=torch.float64, device="cuda")
        fn = lib.buddy_gn_conv3x3_winograd6_f16 if f16 else lib.buddy_gn_conv3x3_winograd6
        _lib.check(fn(P(x0), P(x1), C0, P(gamma), P(beta), G, silu, P(img) if f16 else P(Ud), P(b), P(y), P(scratch), P(stats), stat_scratch.data_ptr(),
                      None, B, H, W, Cin, Cout, S()))
        torch.cuda.synchronize()
        out[f16] = (y, scratch)
    y = out[1][0]
    assert torch.isfinite(y).all()
    e = float((y.double() - ref).abs().max() / ref.abs().max())
    print(f"f16 GN + F(6x6,3x3) {B}x{H}x{W} {Cin}->{Cout}: {e:.2e} of the abs-max vs float64 (fp32 form {float((out[0][0].double() - ref).abs().max() / ref.abs().max()):.2e})")
    assert e < 2e-2
    _check_v(out[1][1], out[0][1], tiles, Cin)


@pytest.mark.parametrize("B,H,W,C,Cout", [(2, 40, 30, 128, 128), (1, 20, 14, 256, 256)])
def test_gnbwd_conv3x3_winograd6_f16(lib, B, H, W, C, Cout):
    from buddy_amd import _lib
    G, silu = min(C // 4, 32), 1
    gen = torch.Generator(device="cpu").manual_seed(B * 1000 + C + Cout + 302)
    x = (torch.randn(B, H, W, C, generator=gen) * 1.5 + 0.3).cuda()
    da = torch.randn(B, H, W, C, generator=gen).cuda()
    gamma = (1 + 0.2 * torch.randn(C, generator=gen)).cuda(); beta = (0.2 * torch.randn(C, generator=gen)).cuda()
    w = torch.randn(Cout, C, 3, 3, generator=gen) / np.sqrt(9 * C)
    xd = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    a = F.silu(F.group_norm(xd, G, gamma.double(), beta.double(), eps=1e-6))
    dx, = torch.autograd.grad(a, xd, da.permute(0, 3, 1, 2).double())
    ref = F.conv2d(dx, w.cuda().double(), None, padding=1).permute(0, 2, 3, 1)
    stats = _gn_stats(x, G)
    wt = w.permute(0, 2, 3, 1).reshape(Cout, 9 * C).contiguous().numpy()
    U = np.empty(64 * C * Cout, dtype=np.float32)
    _lib.check(lib.buddy_winograd6_transform_weights(wt.ctypes.data, Cout, C, U.ctypes.data))
    Ud = torch.from_numpy(U).cuda()
    img = _pack16(lib, Ud, Cout, C)
    tiles = _tiles(B, H, W, 0)
    out = {}
    for f16 in (0, 1):
        y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
        scratch = torch.empty(64 * tiles * (C + Cout), device="cuda")
        stat_scratch = torch.empty(B * 256 * C * 2, dtype=torch.float64, device="cuda")
        red = torch.empty(B, G, 2, device="cuda")
        fn = lib.buddy_gnbwd_conv3x3_winograd6_f16 if f16 else lib.buddy_gnbwd_conv3x3_winograd6
        _lib.check(fn(P(x), P(gamma), P(beta), P(stats), P(da), G, silu, P(img) if f16 else P(Ud), P(y), P(scratch), stat_scratch.data_ptr(), P(red),
                      B, H, W, C, Cout, S()))
        torch.cuda.synchronize()
        out[f16] = (y, scratch)
    y = out[1][0]
    assert torch.isfinite(y).all()
    e = float((y.double() - ref).abs().max() / ref.abs().max())
    print(f"f16 GN-backward + F(6x6,3x3) {B}x{H}x{W} {C}->{Cout}: {e:.2e} of the abs-max vs float64 (fp32 form {float((out[0][0].double() - ref).abs().max() / ref.abs().max()):.2e})")
    assert e < 3e-2
    _check_v(out[1][1], out[0][1], tiles, C)


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 16, 16, 128, 128), (1, 24, 36, 512, 128)])
def test_gn_upconv3x3_winograd6_f16(lib, B, H, W, Cin, Cout):
    from buddy_amd import _lib
    G, silu = min(Cin // 4, 32), 1
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + Cin + Cout + 303)
    x = (torch.randn(B, H, W, Cin, generator=g) * 1.5 + 0.3).cuda()
    gamma = (1 + 0.2 * torch.randn(Cin, generator=g)).cuda(); beta = (0.2 * torch.randn(Cin, generator=g)).cuda()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / np.sqrt(9 * Cin)).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    z = F.silu(F.group_norm(x.permute(0, 3, 2, 1).double(), G, gamma.double(), beta.double(), eps=1e-6))
    ref = F.conv2d(F.interpolate(z, scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1).permute(0, 3, 2, 1)
    U = torch.full((256 * Cin * Cout,), float("nan"), device="cuda")
    _lib.check(lib.buddy_conv3_weight_prep(P(w.contiguous()), Cout, Cin, 0, 61, P(U), S()))
    img = _pack16(lib, U, 4 * Cout, Cin)
    tiles = _tiles(B, H, W, 1)
    out = {}
    for f16 in (0, 1):
        y = torch.full((B, 2 * H, 2 * W, Cout), float("nan"), device="cuda")
        scratch = torch.empty(64 * tiles * (Cin + 4 * Cout), device="cuda")
        stats = torch.empty(B, G, 2, device="cuda")
        stat_scratch = torch.empty(B * 256 * 1024 * 2, dtype=torch.float64, device="cuda")
        fn = lib.buddy_gn_upconv3x3_winograd6_f16 if f16 else lib.buddy_gn_upconv3x3_winograd6
        _lib.check(fn(P(x), P(gamma), P(beta), G, silu, P(img) if f16 else P(U), P(b), P(y), P(scratch), P(stats), stat_scratch.data_ptr(), None,
                      B, H, W, Cin, Cout, S()))
        torch.cuda.synchronize()
        out[f16] = (y, scratch)
    y = out[1][0]
    assert torch.isfinite(y).all()
    e = float((y.double() - ref).abs().max() / ref.abs().max())
    print(f"f16 sub-pixel up conv {B}x{H}x{W} {Cin}->{Cout}: {e:.2e} of the abs-max vs float64 (fp32 form {float((out[0][0].double() - ref).abs().max() / ref.abs().max()):.2e})")
    assert e < 2e-2
    _check_v(out[1][1], out[0][1], tiles, Cin)


@pytest.mark.parametrize("B,H,W,C,Cout", [(2, 16, 16, 128, 128), (1, 24, 36, 256, 256)])
def test_gnbwd_upconv3x3_winograd6_f16(lib, B, H, W, C, Cout):
    from buddy_amd import _lib
    G, silu = min(C // 4, 32), 1
    gen = torch.Generator(device="cpu").manual_seed(B * 1000 + C + Cout + 304)
    h = (torch.randn(B, 2 * H, 2 * W, C, generator=gen) * 1.5 + 0.3).cuda()
    da = torch.randn(B, 2 * H, 2 * W, C, generator=gen).cuda()
    gamma = (1 + 0.2 * torch.randn(C, generator=gen)).cuda(); beta = (0.2 * torch.randn(C, generator=gen)).cuda()
    w = (torch.randn(C, Cout, 3, 3, generator=gen) / np.sqrt(9 * Cout)).cuda()
    hd = h.permute(0, 3, 2, 1).double().requires_grad_(True)
    a = F.silu(F.group_norm(hd, G, gamma.double(), beta.double(), eps=1e-6))
    dx, = torch.autograd.grad(a, hd, da.permute(0, 3, 2, 1).double())
    u = torch.zeros(B, Cout, W, H, dtype=torch.float64, device="cuda", requires_grad=True)
    hh = F.conv2d(F.interpolate(u, scale_factor=2, mode="nearest"), w.double(), None, padding=1)
    ref, = torch.autograd.grad(hh, u, dx)
    ref = ref.permute(0, 3, 2, 1)
    stats = _gn_stats(h, G)
    U = torch.full((256 * C * Cout,), float("nan"), device="cuda")
    _lib.check(lib.buddy_conv3_weight_prep(P(w.contiguous()), C, Cout, 1, 61, P(U), S()))
    img = _pack16(lib, U, Cout, 4 * C)
    tiles = _tiles(B, H, W, 2)
    out = {}
    for f16 in (0, 1):
        y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
        scratch = torch.empty(64 * tiles * (4 * C + Cout), device="cuda")
        stat_scratch = torch.empty(B * 256 * C * 2, dtype=torch.float64, device="cuda")
        red = torch.empty(B, G, 2, device="cuda")
        fn = lib.buddy_gnbwd_upconv3x3_winograd6_f16 if f16 else lib.buddy_gnbwd_upconv3x3_winograd6
        _lib.check(fn(P(h), P(gamma), P(beta), P(stats), P(da), G, silu, P(img) if f16 else P(U), P(y), P(scratch), stat_scratch.data_ptr(), P(red),
                      B, H, W, C, Cout, S()))
        torch.cuda.synchronize()
        out[f16] = (y, scratch)
    y = out[1][0]
    assert torch.isfinite(y).all()
    e = float((y.double() - ref).abs().max() / ref.abs().max())
    print(f"f16 GN-backward + sub-pixel up data-gradient {B}x{H}x{W} {C}->{Cout}: {e:.2e} of the abs-max vs float64 (fp32 form {float((out[0][0].double() - ref).abs().max() / ref.abs().max()):.2e})")
    assert e < 3e-2
    _check_v(out[1][1], out[0][1], tiles, 4 * C)


def _sd(a, b):
    from buddy_amd.utils.metrics import si_sdr
    return float(si_sdr(torch.as_tensor(a).double().reshape(1, -1), torch.as_tensor(b).double().reshape(1, -1)))


def test_denoiser_evaluation_vs_float64_full_size():
    """ONE denoiser evaluation + input-VJP at full width / length (nf 128, L 64000) with gemm = f16 against the algorithm in float64 (as
    test_precision_budget_one_denoiser_evaluation_vs_fp64 does for the default).  Measured: sigma 0.5 D 55.3 dB, VJP 51.6 dB; sigma 0.02 67.5 / 63.3 dB
    (f16x2: 117 / 113 dB).  Floors: the measured values minus 4 dB."""
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from oracle.arbiter_runs import denoiser_eval
    from tests.test_hip_network import build
    net = build(128, 510, 128, 0, gemm="f16")
    edm = instantiate(compose().diff_params)
    for sigma, floor_d, floor_g in ((0.5, 51.3, 47.6), (0.02, 63.5, 59.3)):
        d64, g64, x, w = denoiser_eval(0, 64000, 128, sigma, fp64=True, device="cuda")
        xg = x.cuda().requires_grad_(True)
        d = edm.denoiser(xg, net, sigma)
        g, = torch.autograd.grad(d, xg, w.cuda())
        sd_d, sd_g = _sd(d.detach().cpu(), d64), _sd(g.cpu(), g64)
        print(f"gemm=f16, sigma {sigma}: one denoiser evaluation vs float64: D {sd_d:.1f} dB, VJP {sd_g:.1f} dB")
        assert sd_d > floor_d and sd_g > floor_g, (sigma, sd_d, sd_g)


def test_reproducible_batch_independent_and_per_handle():
    """Two f16 runs are bit-identical; row 0 of B = 2 equals B = 1 (the scale of V depends on the tile's data only); a handle switched
    f16x2 -> f16 -> f16x2 reproduces its first f16x2 result; a replica with gemm = 3 next to a default parent gives each its own arithmetic."""
    from tests.test_hip_network import build
    L = 32000
    net = build(128, 510, 128, 0)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = (0.3 * torch.randn(2, 1, L, generator=g)).cuda()
    cn = torch.tensor([-0.8, 0.3]).cuda()

    def fwd(m, xx, cc):
        with torch.no_grad():
            return m(xx, cc).cpu()
    y2 = fwd(net, x, cn)
    net.set_option("gemm", 3)
    a = fwd(net, x, cn)
    b = fwd(net, x, cn)
    a1 = fwd(net, x[:1], cn[:1])
    net.set_option("gemm", 2)
    y2b = fwd(net, x, cn)
    assert torch.equal(a, b), "two f16 runs differ"
    assert torch.equal(a[:1], a1), "B = 2 row 0 != B = 1"
    assert torch.equal(y2, y2b), "f16x2 -> f16 -> f16x2 does not reproduce"
    assert not torch.equal(a, y2), "gemm = 3 ran the f16x2 arithmetic"
    rel = float((a.double() - y2.double()).abs().max() / y2.double().abs().max())
    print(f"f16 vs f16x2 forward at B = 2, L = {L}: {rel:.2e} of the abs-max")
    assert rel < 2e-2
    r = net.replica()
    r.set_option("gemm", 3)
    assert torch.equal(fwd(r, x, cn), a)
    assert torch.equal(fwd(net, x, cn), y2)


def _chain(net, blind, seeds, L=64000, T=50):
    """The whole schedule for `seeds` as ONE batch on `net` with the seeded noise streams of the float64 gates: the final estimates and the clean signals.
    Two calls on the same seeds differ in nothing but what the network computes."""
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.synth import synth_clean, synth_rir
    from buddy_amd.testing.tester import Tester
    from oracle.arbiter_runs import overrides
    from oracle.sampler_ref import NoiseStream
    args = compose(overrides=overrides(T, 10, 128)) if blind else compose(tester="informed_dereverberation_DPS", overrides=[f"tester.sampling_params.T={T}"])
    t = Tester(args, net, instantiate(args.diff_params), test_set=None, device="cuda", in_training=True)
    ns = [NoiseStream(9000 + s) for s in seeds]
    t.sampler.noise = ns
    seg, y, op, _ = t.prepare_batch([(synth_clean(s, L), synth_rir(s, 8000), f"u{s}.wav") for s in seeds], blind=blind, noise=ns)
    smp = t.sampler
    smp.bind(y, op, blind)
    sched = smp.create_schedule()
    tl, gl = sched.tolist(), smp.get_gamma(sched).tolist()
    x = smp.initialize_x(tuple(y.shape), "cuda", sched)
    for i in range(T):
        x, xd = smp.step(x, tl[i], tl[i + 1], gl[i], blind=blind)
    torch.cuda.synchronize()
    assert torch.isfinite(xd).all()
    return xd.reshape(len(seeds), -1).cpu(), seg.reshape(len(seeds), -1).cpu(), [n.k for n in ns]


def _chain_pair(blind, seeds):
    from tests.test_hip_network import build
    net = build(128, 510, 128, 0)
    a, clean, ka = _chain(net, blind, seeds)
    net.set_option("gemm", 3)
    b, _, kb = _chain(net, blind, seeds)
    assert ka == kb, "noise streams out of step"
    d = [_sd(b[i], clean[i]) - _sd(a[i], clean[i]) for i in range(len(seeds))]
    x = [_sd(b[i], a[i]) for i in range(len(seeds))]
    return d, x


def test_informed_chain_f16_vs_default():
    """Informed DPS (known RIR), order 2, T = 50, full size, seeds 0-3 as one batch, the same noise streams: f16 against the default f16x2 build in the
    same process.  Every |delta SI-SDR to clean| <= 0.1 dB (the north-star tolerance)."""
    d, x = _chain_pair(False, [0, 1, 2, 3])
    print("informed T=50, gemm=f16 vs f16x2: delta SI-SDR to clean " + ", ".join(f"{v:+.4f}" for v in d) + " dB; SI-SDR(f16; f16x2) "
          + ", ".join(f"{v:.1f}" for v in x) + " dB")
    assert max(abs(v) for v in d) <= 0.1, d


def test_blind_chain_f16_vs_default_headline_shape():
    """Blind DPS at the headline shape: B = 8 x 64000, T = 50, 10 operator updates per step, seeds 0-7 as one batch, the same noise streams: f16 against the
    default f16x2 build.  Median over the 8 utterances of |delta SI-SDR to clean| <= 1.0 dB (two float64 executions of this chaotic chain differ by a
    median of 0.74 dB, tests/test_hip_fullsize.py)."""
    d, x = _chain_pair(True, list(range(8)))
    print("blind T=50 B=8, gemm=f16 vs f16x2: delta SI-SDR to clean " + ", ".join(f"{v:+.3f}" for v in d) + f" dB (median |delta| "
          f"{float(np.median(np.abs(d))):.3f} dB); SI-SDR(f16; f16x2) " + ", ".join(f"{v:.1f}" for v in x) + " dB")
    assert float(np.median(np.abs(d))) <= 1.0, d
