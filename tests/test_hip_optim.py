"""GPU: the optimizer kernels alone (buddy_optim_sqnorm, buddy_optim_step, buddy_optim_ema) against float64 numpy.

Tolerances, derived from fp32 rounding (u = 2^-24), not measured:
  sqnorm   relative 1e-12 to float64: the squares of floats are exact in double, only the summation rounds (a fixed tree over n <= 2^25
           non-negative terms: about log2(n) x 2^-53 ~ 3e-15); equal bits on two runs
  m, v     4 u relative to the sum of the magnitudes of their two terms
  p_new    from p = 0: 1e-6 relative (about eight rounded operations of u each, margin 2); with p of order 1: 2 u |p64| = 2^-23 |p64|
  frozen   p, m, v bit for bit their inputs; the EMA is still updated there
torch's own Adam + clip_grad_norm_ on the same fp32 data is held to the same bounds (no equal bits with torch asserted)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _lib():
    from buddy_amd import _lib
    return _lib, _lib.require_gpu()


def sqnorm(g):
    L, lib = _lib()
    chunk = int(lib.buddy_optim_sqnorm_chunk())
    part = torch.full(((g.numel() + chunk - 1) // chunk,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    L.check(lib.buddy_optim_sqnorm(L.ptr(g), g.numel(), part.data_ptr(), out.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    return out


def test_sqnorm_sizes_bits_and_accuracy():
    _, lib = _lib()
    chunk = int(lib.buddy_optim_sqnorm_chunk())
    for n in (1, 3, chunk + 1, 27736590):
        g = np.random.RandomState(n % 1000).standard_normal(n).astype(np.float32) * np.float32(0.37)
        gd = torch.from_numpy(g).cuda()
        a, b = sqnorm(gd), sqnorm(gd)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), f"n={n}: two runs differ"
        ref = float(np.sum(g.astype(np.longdouble) ** 2, dtype=np.longdouble))       # numpy's pairwise sum in 80-bit
        rel = abs(float(a) - ref) / ref
        print(f"sqnorm n={n}: rel err {rel:.2e}")
        assert rel <= 1e-12, (n, rel)


def reference_step(p, g, m, v, ema, sq, max_norm, b1, b2, eps, lr, t, s, frozen):
    """float64 numpy restatement of clip_grad_norm_ + torch's single-tensor Adam + the reference's EMA"""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    coef = min(1.0, max_norm / (math.sqrt(sq) + 1e-6)) if max_norm > 0 else 1.0
    gc = coef * g
    t1, t2 = b1 * m, (1 - b1) * gc
    s1, s2 = b2 * v, (1 - b2) * gc * gc
    mn, vn = t1 + t2, s1 + s2
    denom = np.sqrt(vn) / math.sqrt(1 - b2 ** t) + eps
    pn = p - (lr / (1 - b1 ** t)) * mn / denom
    mask = np.zeros(p.shape, bool)
    for lo, hi in frozen:
        mask[lo:hi] = True
    mn, vn, pn = np.where(mask, m, mn), np.where(mask, v, vn), np.where(mask, p, pn)
    en = None if ema is None else ema.astype(np.float64) * s + pn * (1 - s)
    return pn, mn, vn, en, np.abs(t1) + np.abs(t2), np.abs(s1) + np.abs(s2), mask


def check(tag, got, p, g, m, v, ema, sq, max_norm, b1, b2, eps, lr, t, s, frozen, from_zero):
    pn, mn, vn, en, msc, vsc, mask = reference_step(p, g, m, v, ema, sq, max_norm, b1, b2, eps, lr, t, s, frozen)
    gp, gm, gv, ge = (None if a is None else a.astype(np.float64) for a in got)
    live = ~mask
    em = (np.abs(gm - mn)[live] / (msc[live] + 1e-300)).max() / U
    ev = (np.abs(gv - vn)[live] / (vsc[live] + 1e-300)).max() / U
    ep = (np.abs(gp - pn)[live] / (np.abs(pn[live]) + 1e-300)).max()
    print(f"{tag}: m err {em:.2f} u, v err {ev:.2f} u, p rel err {ep:.2e}")
    assert em <= 4 and ev <= 4, (tag, em, ev)
    assert ep <= (1e-6 if from_zero else 2 * U), (tag, ep)
    if ge is not None:
        # the EMA reads the fp32 p_new: one rounding of the sum of its two products on top of p_new's own error
        ee = (np.abs(ge - en) / (np.abs(ema.astype(np.float64)) * s + np.abs(pn) * (1 - s) + 1e-300)).max()
        assert ee <= (2e-6 if from_zero else 4 * U), (tag, ee)
    return mask


CASES = [
    # name, n, max_norm, eps, t, with ema, frozen ranges, p from zero
    ("clip_active", 100003, 1.0, 1e-8, 1, True, [], True),
    ("clip_inactive", 100000, 1e9, 1e-8, 1, True, [], True),
    ("no_clip", 4097, 0.0, 1e-8, 1000, True, [], True),
    ("negative_max_norm", 4097, -1.0, 1e-8, 1, False, [], True),
    ("large_eps", 65537, 1.0, 1e-3, 1000, True, [], True),
    ("random_p_t1", 100003, 1.0, 1e-8, 1, True, [], False),
    ("random_p_t1000_no_ema", 100002, 1.0, 1e-3, 1000, False, [], False),
    ("frozen_odd_offset", 100003, 1.0, 1e-8, 1, True, [(4099, 4099 + 32), (100001, 100003)], False),
]


def make(n, from_zero, seed):
    rs = np.random.RandomState(seed)
    g = (rs.standard_normal(n) * np.exp(rs.uniform(-6, 1, n))).astype(np.float32)
    # "of order 1": magnitudes in [0.5, 2), so that the 1e-4-sized update never cancels p (the bound is relative to |p_new|)
    p = np.zeros(n, np.float32) if from_zero else (rs.choice([-1.0, 1.0], n) * rs.uniform(0.5, 2.0, n)).astype(np.float32)
    m = (0.1 * rs.standard_normal(n)).astype(np.float32)
    v = (0.01 * rs.standard_normal(n) ** 2).astype(np.float32)
    ema = rs.standard_normal(n).astype(np.float32)
    return p, g, m, v, ema


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_step_vs_float64(case):
    name, n, max_norm, eps, t, with_ema, frozen, from_zero = case
    L, lib = _lib()
    b1, b2, lr, s = 0.9, 0.999, 1e-4, 0.75
    p, g, m, v, ema = make(n, from_zero, len(name))
    if not with_ema:
        ema = None
    d = [None if a is None else torch.from_numpy(a).cuda() for a in (p, g, m, v, ema)]
    sq = sqnorm(d[1]) if max_norm > 0 else None
    fz = (C.c_longlong * max(2 * len(frozen), 1))(*[x for r in frozen for x in r])
    L.check(lib.buddy_optim_step(L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]), n, None if sq is None else sq.data_ptr(), max_norm, b1, b2,
                                 eps, lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t), s, fz, len(frozen), L.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(d[1].cpu().numpy(), g), "the gradient buffer must stay unclipped"
    got = [None if a is None else a.cpu().numpy() for a in (d[0], d[2], d[3], d[4])]
    sq64 = float(np.sum(g.astype(np.float64) ** 2))
    if name == "clip_active":
        assert math.sqrt(sq64) > max_norm
    if name == "clip_inactive":
        assert math.sqrt(sq64) < max_norm
    mask = check(name, got, p, g, m, v, ema, sq64, max_norm, b1, b2, eps, lr, t, s, frozen, from_zero)
    if frozen:
        assert mask.sum() == 34
        for a, b in ((got[0], p), (got[1], m), (got[2], v)):
            assert a[mask].tobytes() == b[mask].tobytes(), "p, m, v inside a frozen range must keep their bits"
        assert not np.array_equal(got[3][mask], ema[mask]), "the EMA runs inside a frozen range too"


def test_ema_only_launch():
    L, lib = _lib()
    n, s = 100003, 1 / 3
    rs = np.random.RandomState(5)
    p, e = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    pd, ed = torch.from_numpy(p).cuda(), torch.from_numpy(e).cuda()
    L.check(lib.buddy_optim_ema(L.ptr(ed), L.ptr(pd), n, s, L.stream_ptr()))
    torch.cuda.synchronize()
    ref = e.astype(np.float64) * s + p.astype(np.float64) * (1 - s)
    scale = np.abs(e.astype(np.float64)) * s + np.abs(p.astype(np.float64)) * (1 - s)
    assert (np.abs(ed.cpu().numpy() - ref) / scale).max() <= 2 * U


@pytest.mark.parametrize("from_zero,t,eps", [(True, 1, 1e-8), (False, 1000, 1e-3)])
def test_torch_adam_meets_the_same_bounds(from_zero, t, eps):
    """torch.optim.Adam + clip_grad_norm_ on the same fp32 data on the GPU against the same float64 restatement and bounds"""
    n, b1, b2, lr, max_norm = 100003, 0.9, 0.999, 1e-4, 1.0
    p, g, m, v, _ = make(n, from_zero, 11)
    if t == 1:
        m[:] = 0; v[:] = 0            # torch starts its moments at zero at step 1
    prm = torch.nn.Parameter(torch.from_numpy(p).cuda())
    opt = torch.optim.Adam([prm], lr=lr, betas=(b1, b2), eps=eps)
    if t > 1:
        opt.state[prm] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m).cuda(), "exp_avg_sq": torch.from_numpy(v).cuda()}
    prm.grad = torch.from_numpy(g).cuda()
    torch.nn.utils.clip_grad_norm_([prm], max_norm)
    opt.step()
    torch.cuda.synchronize()
    st = opt.state[prm]
    got = (prm.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), None)
    check(f"torch t={t}", got, p, g, m, v, None, float(np.sum(g.astype(np.float64) ** 2)), max_norm, b1, b2, eps, lr, t, 0.0, [], from_zero)
