"""Host: the float64 GroupNorm arbiter (tests/_groupnorm_ref.py) agrees with torch.autograd on float64 F.group_norm; an fp32 emulation of the
kernels' arithmetic in numpy stays within the bounds it returns, for every input family of tests/test_hip_groupnorm.py; and the four GroupNorm
entries (csrc/capi.hip: buddy_groupnorm_act(_bwd), buddy_groupnorm_view_fwd / _bwd) are declared, bound and exported and refuse, with
BUDDY_ERR_ARG and a message and before any launch, every shape their kernels cannot compute.  Nothing here launches anything: every call below
is refused (the pointers are small integers that are never dereferenced)."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _groupnorm_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 2
X, Y, Z, Q, V, T = 64, 128, 192, 256, 320, 384          # stand-ins for non-null device pointers
NEW = ("buddy_groupnorm_view_fwd", "buddy_groupnorm_view_bwd")


@pytest.fixture(scope="module")
def lib():
    from buddy_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the arbiter against autograd
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C0,C1,G", [(32, 0, 8), (128, 256, 32), (4, 4, 2)])
def test_restatement_equals_autograd(C0, C1, G, mode, silu):
    B, H, W, C = 2, 4, 6, C0 + C1
    g = torch.Generator(device="cpu").manual_seed(7 + C + mode)
    x32, gamma, beta = R.family("base", B, H, W, C, G, seed=11 + C)
    parts = [x32[..., :C0].double().requires_grad_(True)] + ([x32[..., C0:].double().requires_grad_(True)] if C1 else [])
    xc = torch.cat(parts, dim=3).permute(0, 3, 1, 2)
    z = F.group_norm(xc, G, gamma.double(), beta.double(), eps=1e-6)
    if silu:
        z = F.silu(z)
    if mode == 1:
        z = z.reshape(B, C, H // 2, 2, W // 2, 2).mean(dim=(3, 5))
    elif mode == 2:
        z = z.repeat_interleave(2, 2).repeat_interleave(2, 3)
    dy = torch.randn(z.permute(0, 2, 3, 1).shape, generator=g)
    grads = torch.autograd.grad(z, parts, dy.double().permute(0, 3, 1, 2))
    gx = torch.cat(grads, dim=3)
    f = R.forward(x32, gamma, beta, G, mode, silu)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(f.y, z.detach().permute(0, 2, 3, 1))
    if mode == 1:
        assert close(f.pooled_raw, F.avg_pool2d(x32.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))
    var = x32.double().reshape(B, H * W, G, C // G).var(dim=(1, 3), unbiased=False)
    assert close(f.stats.mean, x32.double().reshape(B, H * W, G, C // G).mean(dim=(1, 3))) and close(f.stats.rstd, (var + 1e-6).rsqrt())
    assert close(R.backward(x32, gamma, beta, G, dy, mode, silu).dx, gx)
    # the extra gradient and the accumulation are sums on top of that
    extra = torch.randn(B, H, W, C, generator=g)
    pre = torch.randn(B, H, W, C, generator=g)
    acc = (torch.arange(C) >= 4).double()
    b1 = R.backward(x32, gamma, beta, G, dy, mode, silu, extra=extra, extra_mode=1, extra_scale=0.5, prefill=pre, acc=acc)
    assert close(b1.dx, gx + 0.5 * extra.double() + pre.double() * acc)
    ex2 = torch.randn(B, H // 2, W // 2, C, generator=g)
    b2 = R.backward(x32, gamma, beta, G, dy, mode, silu, extra=ex2, extra_mode=2, extra_scale=2.0)
    assert close(b2.dx, gx + 0.5 * ex2.double().repeat_interleave(2, 1).repeat_interleave(2, 2))
    cs, _ = R.chan_sums(x32)
    assert close(cs[:, :, 0], x32.double().sum(dim=(1, 2))) and close(cs[:, :, 1], (x32.double() ** 2).sum(dim=(1, 2)))


# ------------------------------------------------------------------------------------------------ fp32 emulation within the bounds
def emulate(x, gamma, beta, G, dy, silu):
    """the kernels' arithmetic in numpy: statistics in fp64 as E[x^2] - mean^2 with the clamp, everything else in fp32 (no FMA); the backward sums in
    fp32 strips of 8 pixels that go to fp64.  Mode 0.  Returns (y, stats (B, G, 2), dx, red (B, G, 2))."""
    f32 = np.float32
    B, H, W, C = x.shape
    cpg, HW = C // G, H * W
    n = float(cpg * HW)
    xd = x.astype(np.float64).reshape(B, HW, G, cpg)
    mean = xd.sum(axis=(1, 3)) / n
    var = np.maximum((xd * xd).sum(axis=(1, 3)) / n - mean * mean, 0.0)
    st = np.stack([mean, 1.0 / np.sqrt(var + float(f32(1e-6)))], axis=2).astype(f32)
    pc = lambda v: np.repeat(v, cpg, axis=1)[:, None, None, :]
    mean32, rstd32 = pc(st[:, :, 0]), pc(st[:, :, 1])
    one = f32(1.0)
    xh = (x - mean32) * rstd32
    z = xh * gamma + beta
    y = z / (one + np.exp(-z)) if silu else z
    if silu:
        s = one / (one + np.exp(-z))
        d = s * (one + z * (one - s))
    else:
        d = np.ones_like(z)
    dxh = dy * d * gamma
    assert y.dtype == f32 and dxh.dtype == f32

    def strips(a):                                 # (B, H, W, C) fp32 -> (B, G) fp64
        v = a.reshape(B, HW, C)
        pad = (-HW) % 8
        v = np.concatenate([v, np.zeros((B, pad, C), f32)], axis=1).reshape(B, -1, 8, C)
        acc = np.zeros((B, v.shape[1], C), f32)
        for j in range(8):
            acc = acc + v[:, :, j]
        return acc.astype(np.float64).sum(axis=1).reshape(B, G, cpg).sum(axis=2)
    red = np.stack([strips(dxh) / n, strips(dxh * xh) / n], axis=2).astype(f32)
    m1, m2 = pc(red[:, :, 0]), pc(red[:, :, 1])
    dx = rstd32 * (dxh - m1 - xh * m2)
    assert dx.dtype == f32
    return y, st, dx, red


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("C,G", [(32, 8), (384, 32)])
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_fp32_emulation_within_bounds(fam, C, G, silu):
    B, H, W = 2, 5, 13
    x, gamma, beta = R.family(fam, B, H, W, C, G, seed=31 + C)
    dy = torch.randn(B, H, W, C, generator=torch.Generator(device="cpu").manual_seed(5))
    y, st, dx, red = emulate(x.numpy(), gamma.numpy(), beta.numpy(), G, dy.numpy(), silu)
    f = R.forward(x, gamma, beta, G, 0, silu)
    b = R.backward(x, gamma, beta, G, dy, 0, silu)
    ratio = lambda out, ref, bound: float(((torch.from_numpy(np.asarray(out)).double() - ref).abs() / bound).nan_to_num(nan=0.0).max())
    assert np.isfinite(y).all() and np.isfinite(dx).all()
    r = {"y": ratio(y, f.y, f.bound), "mean": ratio(st[:, :, 0], f.stats.mean, f.stats.mean_bound),
         "rstd": ratio(st[:, :, 1], f.stats.rstd, f.stats.rstd_bound), "dx": ratio(dx, b.dx, b.bound), "red": ratio(red, b.red, b.red_bound)}
    print(f"groupnorm-host {fam} C={C} silu={silu}: " + " ".join(f"{k} {v:.2f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    if fam == "const":
        g0, cpg = G // 3, C // G
        assert float(f.stats.rstd[0, g0]) == pytest.approx(1000.0, rel=1e-12) and st[0, g0, 1] == np.float32(1000.0)


def test_bounds_reject_wrong_statistics():
    """what the abs-max gate of test_groupnorm_act_fwd_bwd lets through lies outside the returned bounds: eps = 1e-5, an rstd off by 1e-6"""
    B, H, W, C, G = 2, 5, 13, 32, 8
    x, gamma, beta = R.family("offm50", B, H, W, C, G, seed=3)
    f = R.forward(x, gamma, beta, G)
    wrong = R.forward(x, gamma, beta, G, st=R.stats(x, G, eps=1e-5))
    assert float(((wrong.y - f.y).abs() / f.bound).max()) > 1.0
    x, gamma, beta = R.family("base", B, H, W, C, G, seed=3)
    f = R.forward(x, gamma, beta, G)
    off = f.stats._replace(rstd=f.stats.rstd * (1 + 1e-6))
    assert float(((R.forward(x, gamma, beta, G, st=off).y - f.y).abs() / f.bound).max()) > 1.0
    assert float(((off.rstd - f.stats.rstd).abs() / f.stats.rstd_bound).max()) > 1.0


# ------------------------------------------------------------------------------------------------ the entries
def test_err_arg_value():
    hdr = open(os.path.join(ROOT, "buddy_amd", "csrc", "common.h")).read()
    m = re.search(r"#define\s+BUDDY_ERR_ARG\s+(\d+)", hdr)
    assert m and int(m.group(1)) == ERR_ARG


def test_symbols_declared_bound_and_exported(lib):
    from buddy_amd import _lib
    for s in NEW:                                 # header, signatures and exports agree for every name: tests/test_abi_host.py
        assert s in _lib.EXPORTED and hasattr(lib, s), s


def refused(lib, rc):
    return rc == ERR_ARG and len(lib.buddy_last_error()) > 0


SHAPES = (dict(B=0), dict(H=0), dict(W=0), dict(G=0), dict(G=-1), dict(G=3), dict(G=16), dict(mode=3), dict(mode=-1),
          dict(mode=1, H=5), dict(mode=1, W=7))          # C = 32: G = 3 does not divide it, G = 16 leaves 2 channels per group


def test_old_entries_refusals(lib):
    fwd = lambda x=X, ga=Y, be=Z, y=Q, st=V, sc=T, B=2, H=4, W=6, C=32, G=8, mode=0: \
        lib.buddy_groupnorm_act(x, ga, be, y, st, sc, B, H, W, C, G, mode, 1, None)
    for kw in (dict(x=None), dict(ga=None), dict(be=None), dict(y=None), dict(st=None), dict(sc=None), dict(C=0), dict(C=1028, G=257),
               dict(C=2048, G=32), dict(C=30, G=5)) + SHAPES:
        assert refused(lib, fwd(**kw)), kw
    bwd = lambda x=X, ga=Y, be=Z, st=V, dy=Q, dx=T, sc=X, red=Y, B=2, H=4, W=6, C=32, G=8, mode=0: \
        lib.buddy_groupnorm_act_bwd(x, ga, be, st, dy, dx, sc, red, B, H, W, C, G, mode, 1, None)
    for kw in (dict(x=None), dict(ga=None), dict(be=None), dict(st=None), dict(dy=None), dict(dx=None), dict(sc=None), dict(red=None), dict(C=0),
               dict(C=2048, G=32), dict(C=30, G=5)) + SHAPES:
        assert refused(lib, bwd(**kw)), kw


def test_view_fwd_refusals(lib):
    f = lambda x0=X, ld0=16, C0=16, x1=Y, ld1=16, C1=16, ga=Z, be=Q, G=8, mode=0, y=V, pooled=None, st=T, route=0, cs0=None, cs1=None, sc=X, B=2, \
        H=4, W=6: lib.buddy_groupnorm_view_fwd(x0, ld0, C0, x1, ld1, C1, ga, be, G, mode, 1, y, pooled, st, route, cs0, cs1, sc, B, H, W, None)
    for kw in (dict(x0=None), dict(ga=None), dict(be=None), dict(y=None), dict(st=None), dict(sc=None), dict(C0=0), dict(C1=0), dict(C0=-4),
               dict(C0=1012, ld0=1012, G=257), dict(C0=1024, ld0=1024, C1=1024, ld1=1024), dict(C0=14, C1=18, ld1=20),
               dict(C0=2, ld0=4, C1=30, ld1=32), dict(ld0=12), dict(ld0=18), dict(ld1=12), dict(ld1=18),
               dict(x1=None, C0=32, ld0=28), dict(x1=None, C0=32, ld0=34), dict(x1=None, C0=0),
               dict(route=2), dict(route=-1), dict(route=1), dict(route=1, cs0=Q), dict(route=1, cs1=Q), dict(route=1, x1=None, C0=32, ld0=32),
               dict(pooled=Q), dict(pooled=Q, mode=2)) + SHAPES:
        assert refused(lib, f(**kw)), kw


def test_view_bwd_refusals(lib):
    f = lambda x0=X, ld0=16, C0=16, x1=Y, ld1=16, C1=16, ga=Z, be=Q, st=V, dy=T, G=8, mode=0, extra=None, em=0, dx0=X, ldd0=8, dx1=Y, ldd1=24, \
        Cd0=8, sc=Z, red=Q, B=2, H=4, W=6: lib.buddy_groupnorm_view_bwd(x0, ld0, C0, x1, ld1, C1, ga, be, st, dy, G, mode, 1, extra, em, 1.0,
                                                                      dx0, ldd0, 1, dx1, ldd1, 0, Cd0, sc, red, B, H, W, None)
    for kw in (dict(x0=None), dict(ga=None), dict(be=None), dict(st=None), dict(dy=None), dict(dx0=None), dict(sc=None), dict(red=None),
               dict(C0=0), dict(C1=0), dict(C0=1024, ld0=1024, C1=1024, ld1=1024), dict(C0=14, C1=18, ld1=20), dict(ld0=12), dict(ld0=18),
               dict(ld1=12), dict(ld1=18), dict(x1=None, C0=32, ld0=28),
               dict(Cd0=6, ldd0=8, ldd1=28), dict(Cd0=0), dict(Cd0=32), dict(Cd0=36), dict(ldd0=4), dict(ldd0=10), dict(ldd1=20), dict(ldd1=26),
               dict(dx1=None, Cd0=8), dict(dx1=None, Cd0=32, ldd0=28), dict(dx1=None, Cd0=32, ldd0=34),
               dict(em=1), dict(em=2), dict(extra=V), dict(extra=V, em=3), dict(extra=V, em=-1), dict(extra=V, em=2, H=5), dict(extra=V, em=2, W=7)) \
            + SHAPES:
        assert refused(lib, f(**kw)), kw
