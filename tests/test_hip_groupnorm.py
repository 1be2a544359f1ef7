"""GPU unit tests of the stand-alone GroupNorm kernel family (csrc/ops.hip) behind buddy_groupnorm_view_fwd / _bwd, which reach the launchers
with everything the network hands them: concatenated and strided source views, both statistics routes, pooled_raw, the extra gradient and
two-destination gradient views.

  chan_reduce_kernel<0>, group_finalize_kernel<0>      route 0 statistics             every test
  chan_reduce_kernel<0>, csum_collapse_kernel,
  group_finalize_csum_kernel                           route 1 (the network's)        test_concat_views, test_families, test_batch_independence
  gn_apply_m0_kernel, gn_bwd_apply_m0_kernel<EX,ACC>   mode 0                         test_widths, test_pixel_counts, test_m0_tails, test_large,
                                                                                      test_backward_options (all four instantiations)
  gn_apply_kernel, gn_bwd_apply_kernel                 modes 1, 2; extra_mode 2       test_modes_1_2, test_backward_options
  chan_reduce_kernel<1>, group_finalize_kernel<1>      red of every backward

Every case compares with the float64 restatement of tests/_groupnorm_ref.py on the same fp32 inputs, evaluated on the device, and is held per
element to the bound that module returns (a count of fp32 roundings, never relative to an abs-max); behind SiLU to max(bound, 4 e32), e32 the
largest error, within the element's (utterance, group), against float64 of the same expression in torch's own fp32 ops on the device.  Outputs are prefilled and followed by a NaN guard;
source row padding and a non-accumulating destination hold NaN; accumulation is checked as prefill + result; destination row padding must keep
its prefill.  The worst measured / bound ratio per case is printed (pytest -s) as lines starting with "groupnorm"
(profiles/groupnorm_accuracy.txt)."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _groupnorm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 256
PADFILL = 7.0


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


def guarded(t):
    """device copy of t followed by a NaN guard; (flat buffer, view of t's shape)"""
    buf = torch.cat([t.reshape(-1), torch.full((GUARD,), NAN, dtype=t.dtype)]).cuda()
    return buf, buf[:t.numel()].view(t.shape)


def guard_intact(buf):
    return bool(torch.isnan(buf[-GUARD:]).all())


def padded(x, ld, fill=NAN):
    """rows of x (..., C) at a row stride of ld >= C floats on the device; the padding columns hold `fill`"""
    C = x.shape[-1]
    buf = torch.full((x.numel() // C, ld), fill, dtype=x.dtype, device=x.device)
    buf[:, :C] = x.reshape(-1, C)
    return buf.cuda()


def ratio(out, ref, bound, floor=None):
    """max over the elements of |out - ref| / max(bound, floor); NaN (a NaN in out) fails every comparison"""
    err = (out.double() - ref).abs()
    gate = bound if floor is None else torch.maximum(bound, floor)
    r = torch.where((gate == 0) & (err == 0), torch.zeros_like(err), err / gate)
    return float(r.max())


def report(line):
    print("groupnorm " + line)


def e32_floor(t32, ref, G):
    """4 e32 per element: e32 = the largest error of torch's fp32 evaluation within the element's (utterance, group), which shares one mean and
    rstd -- narrower than one figure for the tensor, under which a group at rstd = 1000 or an utterance 3000 times larger would set the gate of all"""
    B, H, W, C = ref.shape
    e = (t32.double() - ref).abs().reshape(B, H * W, G, C // G).amax(dim=(1, 3))
    return 4 * R.per_channel(e, C)


def groups(C):
    return min(C // 4, 32)


def run(lib, x, gamma, beta, G, C0=None, pad=False, route=0, mode=0, silu=1, pooled=False, extra_mode=0, extra_scale=1.0, Cd0=None,
        acc=(0, 0), dpad=False, seed=1, keep=None):
    """one forward and one backward launch on the CPU tensors x (B, H, W, C), gamma, beta; returns the worst ratios by output.  C0: split of the
    source view (None: one source); pad: source row strides of C0 + 8 / C1 + 4; Cd0: split of the destination view; dpad: destination strides of
    width + 4 / + 8.  keep: a dict that receives the raw device outputs."""
    B, H, W, C = x.shape
    g = gen(seed)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    if C0 is None:
        ld0, ld1, C1 = C + (8 if pad else 0), 0, 0
        x0, x1 = padded(xd, ld0), None
    else:
        C1 = C - C0
        ld0, ld1 = C0 + (8 if pad else 0), C1 + (4 if pad else 0)
        x0, x1 = padded(xd[..., :C0], ld0), padded(xd[..., C0:], ld1)
    Ho, Wo = (H // 2, W // 2) if mode == 1 else (2 * H, 2 * W) if mode == 2 else (H, W)
    ybuf, y = guarded(torch.randn(B, Ho, Wo, C, generator=g) + 3.0)
    pbuf, praw = guarded(torch.randn(B, Ho, Wo, C, generator=g) + 3.0) if pooled else (None, None)
    sbuf, stats = guarded(torch.full((B, G, 2), 5.0))
    c0buf, cs0 = guarded(torch.full((B, C0 or C, 2), 5.0, dtype=torch.float64))
    c1buf, cs1 = guarded(torch.full((B, max(C1, 1), 2), 5.0, dtype=torch.float64))
    scratch = torch.empty(B * 256 * C * 2, dtype=torch.float64, device="cuda")
    check(lib.buddy_groupnorm_view_fwd(P(x0), ld0, C if C0 is None else C0, P(x1), ld1, C1, P(gd), P(bd), G, mode, silu,
                                       P(y), P(praw), P(stats), route, P(cs0) if route else None, P(cs1) if route and x1 is not None else None,
                                       P(scratch), B, H, W, S()))
    torch.cuda.synchronize()
    assert guard_intact(ybuf) and guard_intact(sbuf) and guard_intact(c0buf) and guard_intact(c1buf), "wrote behind an output"
    f = R.forward(xd, gd, bd, G, mode, silu)
    floor = e32_floor(R.fp32_forward(xd, gd, bd, G, f.stats, mode), f.y, G) if silu else None
    out = {"y": ratio(y, f.y, f.bound, floor), "mean": ratio(stats[:, :, 0], f.stats.mean, f.stats.mean_bound),
           "rstd": ratio(stats[:, :, 1], f.stats.rstd, f.stats.rstd_bound)}
    assert bool(torch.isfinite(y).all())
    if pooled:
        assert guard_intact(pbuf)
        out["pooled"] = ratio(praw, f.pooled_raw, f.pooled_bound)
    if route:
        cr, cb = R.chan_sums(xd)
        out["csum"] = ratio(cs0, cr[:, :C0 or C], cb[:, :C0 or C])
        if x1 is not None:
            out["csum"] = max(out["csum"], ratio(cs1, cr[:, C0:], cb[:, C0:]))

    # backward
    dy = torch.randn(B, Ho, Wo, C, generator=g).cuda()
    extra = None
    if extra_mode:
        extra = torch.randn((B, H, W, C) if extra_mode == 1 else (B, H // 2, W // 2, C), generator=g).cuda()
    cd0 = C if Cd0 is None else Cd0
    accm = torch.cat([torch.full((cd0,), float(acc[0])), torch.full((C - cd0,), float(acc[1]))]).cuda()
    pre = (torch.randn(B, H, W, C, generator=g) + 3.0).cuda()
    pre_in = torch.where(accm.bool(), pre, torch.full_like(pre, NAN))          # a half that does not accumulate must ignore what it holds
    ldd0, ldd1 = cd0 + (4 if dpad else 0), (C - cd0) + (8 if dpad else 0)
    d0 = padded(pre_in[..., :cd0], ldd0, PADFILL)
    d0buf, d0 = guarded(d0.cpu())
    d1buf = d1 = None
    if Cd0 is not None:
        d1buf, d1 = guarded(padded(pre_in[..., cd0:], ldd1, PADFILL).cpu())
    rbuf, red = guarded(torch.full((B, G, 2), 5.0))
    check(lib.buddy_groupnorm_view_bwd(P(x0), ld0, C if C0 is None else C0, P(x1), ld1, C1, P(gd), P(bd), P(stats), P(dy), G, mode, silu, P(extra),
                                       extra_mode, extra_scale, P(d0), ldd0, int(acc[0]), P(d1), ldd1, int(acc[1]), cd0, P(scratch), P(red), B, H, W,
                                       S()))
    torch.cuda.synchronize()
    assert guard_intact(d0buf) and guard_intact(rbuf) and (d1buf is None or guard_intact(d1buf)), "wrote behind an output"
    assert bool((d0[:, cd0:] == PADFILL).all()) and (d1 is None or bool((d1[:, C - cd0:] == PADFILL).all())), "wrote into the row padding of dx"
    dx = d0[:, :cd0] if d1 is None else torch.cat([d0[:, :cd0], d1[:, :C - cd0]], dim=1)
    dx = dx.reshape(B, H, W, C)
    assert bool(torch.isfinite(dx).all())
    b = R.backward(xd, gd, bd, G, dy, mode, silu, extra, extra_mode, extra_scale, pre, accm if any(acc) else None)
    floor = None
    if silu:
        core = b if not (extra_mode or any(acc)) else R.backward(xd, gd, bd, G, dy, mode, silu)
        floor = e32_floor(R.fp32_backward(xd, gd, bd, G, dy, f.stats, b.red, mode), core.dx, G)
    out["dx"] = ratio(dx, b.dx, b.bound, floor)
    out["red"] = ratio(red, b.red, b.red_bound)
    if keep is not None:
        keep.update(y=y.clone(), stats=stats.clone(), dx=dx.clone(), red=red.clone(), cs0=cs0.clone(), cs1=cs1.clone(), dy=dy, extra=extra, pre=pre)
    return out


def fmt(r):
    return " ".join(f"{k} {v:.2f}" for k, v in r.items())


def merge(worst, r):
    for k, v in r.items():
        w = worst.get(k, 0.0)
        worst[k] = w if (w != w or v <= w) else v                              # a NaN ratio sticks


def passes(r):
    return all(v <= 1.0 for v in r.values())


# ------------------------------------------------------------------------------------------------ widths and thread geometry
@pytest.mark.parametrize("C", [4, 8, 32, 96, 128, 256, 384, 512, 768, 1024])
def test_widths(lib, C):
    """mode 0, forward + backward, one source, B = 2, HW = 130, G = min(C / 4, 32): q = C / 4 channel quads and pl = 256 / q pixels per block from
    (1, 256) at C = 4 to (256, 1) at C = 1024; C = 96 a 240-thread apply block and 16 idle reduction threads, C = 768 pl = 1 with 64 idle."""
    B, H, W, G = 2, 10, 13, groups(C)
    x, gamma, beta = R.family("base", B, H, W, C, G, seed=100 + C)
    for silu in (1, 0):
        r = run(lib, x, gamma, beta, G, silu=silu, seed=200 + C)
        report(f"widths C={C} G={G} silu={silu}: {fmt(r)}")
        assert passes(r), r


# ------------------------------------------------------------------------------------------------ concatenated views
@pytest.mark.parametrize("C0,C1", [(128, 256), (256, 128), (512, 512), (16, 16), (4, 4)])
def test_concat_views(lib, C0, C1):
    """two sources, dense and with padded rows (ld0 = C0 + 8, ld1 = C1 + 4, NaN in the padding), both statistics routes, each held to the float64
    bound (csum0 / csum1 too on route 1); (128, 256) and (256, 128) have 12 channels per group, so one group straddles the sources.  The gradient
    goes to a destination split like the source, the second half accumulating."""
    C = C0 + C1
    B, H, W, G = 2, 10, 13, groups(C)
    x, gamma, beta = R.family("base", B, H, W, C, G, seed=300 + C0)
    for pad in (0, 1):
        for route in (0, 1):
            r = run(lib, x, gamma, beta, G, C0=C0, pad=pad, route=route, Cd0=C0, acc=(0, 1), dpad=pad, seed=400 + C0 + pad)
            report(f"concat ({C0}, {C1}) padded={pad} route={route}: {fmt(r)}")
            assert passes(r), r


# ------------------------------------------------------------------------------------------------ pixel counts
@pytest.mark.parametrize("H,W", [(1, 1), (1, 63), (8, 8), (5, 13), (2, 65), (257, 65)])
@pytest.mark.parametrize("C", [32, 4])
def test_pixel_counts(lib, C, H, W):
    """mode 0, B = 2.  HW = 1 (one thread of a block has a pixel), 63 / 64 / 65 / 130 around the 64-pixel reduction chunk, 16 705 = 257 x 65: the
    256-chunk cap of gn_num_chunks with ppc = 66, so the last two chunks are empty."""
    G = groups(C)
    x, gamma, beta = R.family("base", 2, H, W, C, G, seed=500 + H * W + C)
    r = run(lib, x, gamma, beta, G, seed=600 + H * W)
    report(f"pixels C={C} {H}x{W}: {fmt(r)}")
    assert passes(r), r


@pytest.mark.parametrize("C,HWs", [(128, (40, 48, 56, 43, 129)), (512, (10, 12, 14, 13, 33))])
def test_m0_tails(lib, C, HWs):
    """C = 128 (pl = 8) and 512 (pl = 2) with one chunk of 5, 6 and 7 trips per thread: the 4-pixel forward loop leaves tails of 1, 2 and 3 trips, the
    2-pixel backward loop of 1 and 0; the odd counts give the threads of a block different trip counts; the last is more than one chunk."""
    G = groups(C)
    for HW in HWs:
        x, gamma, beta = R.family("base", 2, 1, HW, C, G, seed=700 + HW)
        r = run(lib, x, gamma, beta, G, extra_mode=1, extra_scale=0.5, acc=(1, 0), seed=800 + HW)
        report(f"tails C={C} HW={HW}: {fmt(r)}")
        assert passes(r), r


def test_large(lib):
    """B = 1, C = 1024, HW = 131 072 + 1 027 = 33 x 4003: gn_m0_geo asks for HW / 4 = 33 024 chunks and is capped at 32 768, so ppc = 5 (one tail
    trip) over 26 420 blocks; pixel offsets pass 2^27 floats.  Inputs drawn on the device; the float64 restatement runs in slabs of 8192 pixels."""
    B, H, W, C, G, SL = 1, 33, 4003, 1024, 32, 8192
    HW = H * W
    gd = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(B, 1, HW, C, device="cuda", generator=gd) * 1.5 + 0.3
    dy = torch.randn(B, 1, HW, C, device="cuda", generator=gd)
    gamma = 1 + 0.2 * torch.randn(C, device="cuda", generator=gd)
    beta = 0.2 * torch.randn(C, device="cuda", generator=gd)
    ybuf = torch.full((x.numel() + GUARD,), NAN, device="cuda")
    dbuf = torch.full((x.numel() + GUARD,), NAN, device="cuda")
    sbuf, stats = guarded(torch.full((B, G, 2), 5.0))
    rbuf, red = guarded(torch.full((B, G, 2), 5.0))
    scratch = torch.empty(B * 256 * C * 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    check(lib.buddy_groupnorm_view_fwd(P(x), C, C, None, 0, 0, P(gamma), P(beta), G, 0, 1, P(ybuf), None, P(stats), 0, None, None, P(scratch), B, H,
                                       W, S()))
    check(lib.buddy_groupnorm_view_bwd(P(x), C, C, None, 0, 0, P(gamma), P(beta), P(stats), P(dy), G, 0, 1, None, 0, 0.0, P(dbuf), C, 0, None, 0, 0,
                                       C, P(scratch), P(red), B, H, W, S()))
    torch.cuda.synchronize()
    t_kernels = time.perf_counter() - t0
    assert guard_intact(ybuf) and guard_intact(dbuf) and guard_intact(sbuf) and guard_intact(rbuf)
    y, dx = ybuf[:-GUARD].view(x.shape), dbuf[:-GUARD].view(x.shape)
    slabs = [slice(p, min(HW, p + SL)) for p in range(0, HW, SL)]
    n = float(HW * (C // G))
    s1 = sum(R.group_sum(x[:, :, s].double(), G) for s in slabs)
    sa = sum(R.group_sum(x[:, :, s].double().abs(), G) for s in slabs)
    s2 = sum(R.group_sum(x[:, :, s].double() ** 2, G) for s in slabs)
    mean = s1 / n
    var = sum(R.group_sum((x[:, :, s].double() - R.per_channel(mean, C)) ** 2, G) for s in slabs) / n
    rstd = 1.0 / torch.sqrt(var + R.EPS)
    st = R.Stats(mean, rstd, R.U * mean.abs() + R.FP64_SUM * sa / n, rstd * (2 * R.U + R.FP64_SUM * (s2 / n) / (var + R.EPS)))
    sums = None
    for s in slabs:
        t = R.backward_sums(x[:, :, s], gamma, beta, G, dy[:, :, s], st, 0, True)
        sums = t if sums is None else R.RedSums(*[a + b for a, b in zip(sums, t)])
    rd = R.red_of(sums, 0)
    r = {"mean": ratio(stats[:, :, 0], st.mean, st.mean_bound), "rstd": ratio(stats[:, :, 1], st.rstd, st.rstd_bound),
         "red": ratio(red, rd[0], rd[1]), "y": 0.0, "dx": 0.0}
    for s in slabs:
        f = R.forward(x[:, :, s], gamma, beta, G, 0, True, st=st)
        b = R.backward(x[:, :, s], gamma, beta, G, dy[:, :, s], 0, True, st=st, red=rd)
        ef = e32_floor(R.fp32_forward(x[:, :, s], gamma, beta, G, st), f.y, G)
        eb = e32_floor(R.fp32_backward(x[:, :, s], gamma, beta, G, dy[:, :, s], st, rd[0]), b.dx, G)
        merge(r, {"y": ratio(y[:, :, s], f.y, f.bound, ef), "dx": ratio(dx[:, :, s], b.dx, b.bound, eb)})
    torch.cuda.synchronize()
    report(f"large C={C} HW={HW}: {fmt(r)}; kernels (4 launches + first-use) {1e3 * t_kernels:.1f} ms, test {time.perf_counter() - t0:.2f} s")
    assert passes(r), r


# ------------------------------------------------------------------------------------------------ modes 1 and 2
@pytest.mark.parametrize("H,W", [(2, 2), (6, 10), (16, 24)])
@pytest.mark.parametrize("C,C0", [(4, 4), (96, 48), (384, 128)])
def test_modes_1_2(lib, C, C0, H, W):
    """gn_apply_kernel / gn_bwd_apply_kernel: mode 1 (2x2 mean; with and without pooled_raw, held to 4u of the mean of absolute values) and mode 2
    (nearest x2; the gradient is the fp32 sum of four), one source of C channels and two (C0, C0) resp. (128, 256) -- 4 channels cannot be split,
    so the smallest pair is (4, 4) with C = 8."""
    for concat in (0, 1):
        Cc = (2 * C0 if C != 384 else C) if concat else C
        G = groups(Cc)
        x, gamma, beta = R.family("base", 2, H, W, Cc, G, seed=900 + Cc + H)
        worst = {}
        for mode, pooled in ((1, 0), (1, 1), (2, 0)):
            for silu in (1, 0):
                r = run(lib, x, gamma, beta, G, C0=C0 if concat else None, pad=concat, route=concat, mode=mode, silu=silu, pooled=pooled,
                        seed=1000 + mode + H)
                assert passes(r), (concat, mode, pooled, silu, r)
                merge(worst, r)
        report(f"modes C={Cc} concat={concat} {H}x{W}: {fmt(worst)}")


# ------------------------------------------------------------------------------------------------ backward options
@pytest.mark.parametrize("C,C0,Cd0", [(32, 16, 12), (384, 128, 256)])
def test_backward_options(lib, C, C0, Cd0):
    """a destination split unlike the source's, at strides wider than the parts.  extra_mode 0 / 1 x (acc0, acc1) in all four combinations: the four
    gn_bwd_apply_m0_kernel<EX, ACC> instantiations; the half that does not accumulate is prefilled with NaN, which <*, true> reads and must discard.
    extra_mode 2 (a quarter-resolution extra, factor 0.25 extra_scale) with extra_scale 1 and 2^-0.5: the general kernel."""
    B, H, W, G = 2, 6, 10, groups(C)
    x, gamma, beta = R.family("base", B, H, W, C, G, seed=1100 + C)
    for em, scale in ((0, 1.0), (1, 0.75), (2, 1.0), (2, 2.0 ** -0.5)):
        for acc in ((0, 0), (1, 0), (0, 1), (1, 1)):
            r = run(lib, x, gamma, beta, G, C0=C0, extra_mode=em, extra_scale=scale, Cd0=Cd0, acc=acc, dpad=True, seed=1200 + em)
            report(f"bwd-options C={C} extra_mode={em} scale={scale:.3f} acc={acc}: dx {r['dx']:.2f} red {r['red']:.2f}")
            assert passes(r), r
    r = run(lib, x, gamma, beta, G, extra_mode=1, extra_scale=-1.5, acc=(1, 0), dpad=True, seed=1300)      # one destination, wider stride
    report(f"bwd-options C={C} one destination, padded: dx {r['dx']:.2f}")
    assert passes(r), r


# ------------------------------------------------------------------------------------------------ input families
@pytest.mark.parametrize("C0,C1", [(32, 0), (128, 256)])
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_families(lib, fam, C0, C1):
    """B = 2, 5 x 13 pixels, with and without SiLU, both statistics routes: a mean large against the spread (E[x^2] - mean^2 cancels: the reason
    the statistics are fp64), a variance at and far below eps, one group of one utterance constant (var = 0, rstd = 1000, everything finite), a zero
    and a negative gamma, utterances of one batch 3000 apart in scale."""
    C = C0 + C1
    G = groups(C)
    x, gamma, beta = R.family(fam, 2, 5, 13, C, G, seed=1400 + C)
    for silu in (0, 1):
        for route in (0, 1):
            keep = {}
            r = run(lib, x, gamma, beta, G, C0=C0 if C1 else None, route=route, silu=silu, seed=1500 + silu, keep=keep)
            report(f"family {fam} C={C} silu={silu} route={route}: {fmt(r)}")
            assert passes(r), r
            if fam == "const":
                assert float(keep["stats"][0, G // 3, 1]) == 1000.0


# ------------------------------------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("C0,C1", [(32, 0), (16, 16), (128, 256)])
def test_batch_independence(lib, C0, C1):
    """row b of a B = 3 call equals the B = 1 call on that row, bit for bit: y, stats, dx, red and csum (route 1)"""
    C = C0 + C1
    G, B, H, W = groups(C), 3, 10, 13
    x, gamma, beta = R.family("rows3000", B, H, W, C, G, seed=1600 + C)
    kw = dict(C0=C0 if C1 else None, route=1, extra_mode=1, extra_scale=0.5, acc=(1, 0))
    whole = {}
    run(lib, x, gamma, beta, G, seed=1700, keep=whole, **kw)
    for b in range(B):
        one = {}
        run_row(lib, x, gamma, beta, G, b, one, whole, kw)
        for k in ("y", "stats", "dx", "red", "cs0") + (("cs1",) if C1 else ()):
            assert torch.equal(one[k][0], whole[k][b]), (k, b)
    report(f"batch-independence ({C0}, {C1}): rows of B=3 bit-equal to B=1")


def run_row(lib, x, gamma, beta, G, b, one, whole, kw):
    """the B = 1 call on row b with the very dy, extra and prefill rows of the B = 3 call (kept by run() in `whole`)"""
    B, H, W, C = x.shape
    C0 = kw["C0"]
    xd, gd, bd = x[b:b + 1].cuda(), gamma.cuda(), beta.cuda()
    x0 = xd if C0 is None else xd[..., :C0].contiguous()
    x1 = None if C0 is None else xd[..., C0:].contiguous()
    c0, c1 = (C, 0) if C0 is None else (C0, C - C0)
    y = torch.empty(1, H, W, C, device="cuda")
    stats, red = torch.empty(1, G, 2, device="cuda"), torch.empty(1, G, 2, device="cuda")
    cs0 = torch.empty(1, c0, 2, dtype=torch.float64, device="cuda")
    cs1 = torch.empty(1, max(c1, 1), 2, dtype=torch.float64, device="cuda")
    scratch = torch.empty(256 * C * 2, dtype=torch.float64, device="cuda")
    check(lib.buddy_groupnorm_view_fwd(P(x0), c0, c0, P(x1), c1, c1, P(gd), P(bd), G, 0, 1, P(y), None, P(stats), 1, P(cs0), P(cs1) if c1 else None,
                                       P(scratch), 1, H, W, S()))
    dy, extra, dx = whole["dy"][b:b + 1].contiguous(), whole["extra"][b:b + 1].contiguous(), whole["pre"][b:b + 1].contiguous()
    check(lib.buddy_groupnorm_view_bwd(P(x0), c0, c0, P(x1), c1, c1, P(gd), P(bd), P(stats), P(dy), G, 0, 1, P(extra), 1, kw["extra_scale"], P(dx), C,
                                       1, None, 0, 0, C, P(scratch), P(red), 1, H, W, S()))
    torch.cuda.synchronize()
    one.update(y=y, stats=stats, dx=dx, red=red, cs0=cs0, cs1=cs1)
