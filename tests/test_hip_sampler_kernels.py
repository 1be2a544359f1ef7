"""GPU unit tests of the sampler-step kernels (csrc/sampler.hip) behind their C-ABI entries, of the FIR operator and its autograd transpose, of
SDE.scalars_on_device and of EulerHeunSamplerDPS._step_hip with the network and the operator stubbed: every case against the float64 arbiter
tests/_sampler_ref.py, which also supplies the bound.

Bounds are counts of roundings, u = 2^-24 (see the arbiter's docstrings); the FIR keeps 1e-5 of a row's abs-max
(tests/test_hip_kernels.py::test_fir_and_adjoint) and the moments 1e-9 (test_row_ops).  Inputs come from seeded CPU generators; rows of a batch
differ strongly in scale (0.5, -3, 40 / std 0.01, 1, 30) so that a slipped row index shows; every output lies between two guard bands of a
sentinel that must stay untouched.  Every test prints its worst error / bound ratio (pytest -s) in lines starting with "sampler_kernels"
(profiles/sampler_kernels_accuracy.txt)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                 # floats in front of and behind every output (256 bytes: the output itself stays 16-byte aligned)
SENTINEL = -7654.25
GAIN = np.array([0.5, -3.0, 40.0])
STD = np.array([0.01, 1.0, 30.0])
NAN = float("nan")


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


def dev(a):
    """float32 device copy of a numpy array (None stays None)"""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


class Guarded:
    """an output of `shape` between two guard bands; .t is the view handed to the kernel, .get() checks the bands and returns float64 numpy"""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def get(self, raw=False):
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all()), "guard band written"
        a = self.t.cpu().numpy()
        return a if raw else a.astype(np.float64)


def ratio(got, ref, bound):
    """worst |got - ref| / bound; an exact hit on a zero bound counts as 0"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


def rows(rs, B, L, scales):
    s = np.resize(np.asarray(scales, np.float64), B)
    return f32(rs.standard_normal((B, L)) * s[:, None])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- perturb, axpby_rows, row_moments -------------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (3, 85), (4, 64), (257, 1), (3, 5001), (17, 61681)]      # B L = 1, 255, 256, 257, 3 * 5001, 4096 * 256 + 1 (second trip of the capped grid)


@pytest.mark.parametrize("B,L", SIZES)
def test_perturb(lib, B, L):
    rs = np.random.RandomState(B * 7 + L)
    n = B * L
    for s in (0.0, 0.37532, 41.7):
        x, eps = f32(rs.standard_normal(n) * 0.3), f32(rs.standard_normal(n))
        xd, ed, out = dev(x), dev(eps), Guarded((n,))
        check(lib.buddy_perturb(P(xd), P(ed), s, P(out.t), n, S()))
        ref, bound = R.perturb(x, eps, s)
        r = ratio(out.get(), ref, bound)
        print(f"sampler_kernels perturb n {n:>8} scale {s:<8} err/bound {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("B,L", SIZES)
def test_axpby_rows(lib, B, L):
    rs = np.random.RandomState(B * 11 + L)
    x, y = rows(rs, B, L, STD), rows(rs, B, L, STD[::-1])
    a, c = f32(np.resize(GAIN, B) * rs.uniform(0.9, 1.1, B)), f32(np.resize(GAIN[::-1], B) * rs.uniform(0.9, 1.1, B))
    xd, yd, ad, cd = dev(x), dev(y), dev(a), dev(c)
    for with_y in (True, False):
        out = Guarded((B, L))
        check(lib.buddy_axpby_rows(P(xd), P(yd) if with_y else None, P(ad), P(cd) if with_y else None, P(out.t), B, L, S()))
        ref, bound = R.axpby_rows(x, y if with_y else None, a, c)
        r = ratio(out.get(), ref, bound)
        print(f"sampler_kernels axpby_rows B {B:>3} L {L:>6} y {'given' if with_y else 'None '} err/bound {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("L", [1, 255, 256, 257, 65537])
def test_row_moments(lib, L):
    rs = np.random.RandomState(L)
    x = rows(rs, 3, L, STD) + f32([[0.0], [0.25], [0.0]])
    xd, out = dev(x), Guarded((3, 2), torch.float64)
    check(lib.buddy_row_moments(P(xd), P(out.t), 3, L, S()))
    ref, bound = R.row_moments(x)
    r = ratio(out.get(), ref, bound[None, :])
    print(f"sampler_kernels row_moments L {L:>6} err/bound {r:.3e}")
    assert r <= 1.0


# ---- row_scale ------------------------------------------------------------------------------------------------------------------------------

SCALE_L = [2, 3, 4, 5, 1023, 1024, 1025, 4096, 4100, 5001, 65537]
P0 = {0: 0.05, 1: 0.5}
P1 = 5001 ** 0.5


def run_row_scale(lib, x, mode, offset):
    """buddy_row_scale on the rows of x placed `offset` floats behind a 256-byte boundary -> (B,) float32 (numpy), and the same for every row alone"""
    B, L = x.shape
    buf = torch.zeros(B * L + 8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    xs = buf[offset:offset + B * L]
    xs.copy_(torch.from_numpy(x).reshape(-1))
    out = Guarded((B,))
    check(lib.buddy_row_scale(P(xs), P(out.t), B, L, mode, P0[mode], P1, S()))
    got = out.get(raw=True)
    for b in range(B):                              # the same row at the same address, as a batch of one: bit for bit
        one = Guarded((1,))
        check(lib.buddy_row_scale(P(xs[b * L:(b + 1) * L]), P(one.t), 1, L, mode, P0[mode], P1, S()))
        assert bits(one.get(raw=True))[0] == bits(got)[b], f"row {b} of the batch differs from the batch of one"
    return got


@pytest.mark.parametrize("L", SCALE_L)
def test_row_scale(lib, L):
    rs = np.random.RandomState(L)
    x = rows(rs, 3, L, STD)
    for mode in (0, 1):
        ref, bound = R.row_scale(x, mode, P0[mode], P1)
        for offset in ((0, 4, 1) if L % 4 == 0 else (0, 1)):      # L % 4 == 0: 16-byte aligned rows take the float4 path, one float further the scalar path
            r = ratio(run_row_scale(lib, x, mode, offset), ref, bound)
            print(f"sampler_kernels row_scale mode {mode} L {L:>6} offset {offset} err/bound {r:.3f}")
            assert r <= 1.0


@pytest.mark.parametrize("L", [4, 1025, 4096, 65537])
def test_row_scale_dc_offset_and_silence(lib, L):
    """row 0: mean 1, std 1e-2 (the one-pass variance in double has mean^2 / var = 1e4 to spare); row 1: all zero; row 2: plain"""
    rs = np.random.RandomState(L + 1)
    x = np.stack([f32(1.0 + 1e-2 * rs.standard_normal(L)), np.zeros(L, np.float32), f32(rs.standard_normal(L))])
    for mode in (0, 1):
        ref, bound = R.row_scale(x, mode, P0[mode], P1)
        for offset in ((0, 1) if L % 4 == 0 else (0,)):
            got = run_row_scale(lib, x, mode, offset)
            r = ratio(got[[0, 2]], ref[[0, 2]], bound[[0, 2]])
            print(f"sampler_kernels row_scale mode {mode} L {L:>6} offset {offset} dc-offset row err/bound {r:.3f}, silent row {got[1]}")
            assert r <= 1.0
            if mode == 0:
                assert np.isposinf(got[1]) and np.isposinf(ref[1])                # p0 / Tensor.std() of silence
            else:
                assert bits(got[1]) == bits(np.float32(P0[1]) / np.float32(1e-8))


# ---- fill_rows4, scalars_on_device ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
def test_fill_rows4(lib, B):
    v = f32([-2.878231, 19.999975, 2.5e-9, 0.05])
    out = Guarded((4, B))
    check(lib.buddy_fill_rows4(P(out.t), B, float(v[0]), float(v[1]), float(v[2]), float(v[3]), S()))
    assert np.array_equal(bits(out.get(raw=True)), bits(np.repeat(v[:, None], B, axis=1)))


def test_scalars_on_device():
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    args = compose()
    sde, hp, sp = instantiate(args.diff_params), args.diff_params.sde_hp, args.tester.sampling_params.sde_hp
    mid = (sp.sigma_max ** (1 / sp.rho) + 100 / 200 * (sp.sigma_min ** (1 / sp.rho) - sp.sigma_max ** (1 / sp.rho))) ** sp.rho
    for sigma in (hp.sigma_min, hp.sigma_max, hp.sigma_data, sp.sigma_min, sp.sigma_max, 1.0, mid):
        got = sde.scalars_on_device(sigma, 5, "cuda")
        assert got.shape == (4, 5) and got.dtype == torch.float32
        got = got.cpu().numpy()
        assert np.array_equal(bits(got), bits(np.repeat(got[:, :1], 5, axis=1)))
        ref, bound = R.edm_scalars(np.float32(sigma), hp.sigma_data)
        r = ratio(got[:, 0], ref, bound)
        print(f"sampler_kernels scalars_on_device sigma {sigma:<10.4g} err/bound {r:.3f} (cnoise, cin, cskip, cout) = {got[:, 0]}")
        assert r <= 1.0
        if sigma == 1.0:
            assert got[0, 0] == 0.0


# ---- dps_update -----------------------------------------------------------------------------------------------------------------------------

DPS_CONFIGS = {            # lh, lh_scale, den_scale, base is x_hat, d_prev, w_prev, w_cur, d_out, x_den_out
    "euler":         dict(lh=1, lhs=1, dens=1, same_base=1, dprev=0, w=(0.0, 1.0), d_out=1, xd_out=1),
    "heun":          dict(lh=1, lhs=1, dens=0, same_base=0, dprev=1, w=(0.5, 0.5), d_out=1, xd_out=1),
    "heun-uneven":   dict(lh=1, lhs=1, dens=1, same_base=0, dprev=1, w=(0.25, 0.75), d_out=1, xd_out=1),     # not in the sampler: tells w_prev from w_cur
    "no-lh":         dict(lh=0, lhs=0, dens=1, same_base=1, dprev=0, w=(0.0, 1.0), d_out=1, xd_out=1),
    "lh-unscaled":   dict(lh=1, lhs=0, dens=1, same_base=0, dprev=1, w=(0.5, 0.5), d_out=1, xd_out=1),
    "no-d_out":      dict(lh=1, lhs=1, dens=1, same_base=1, dprev=0, w=(0.0, 1.0), d_out=0, xd_out=1),
    "no-x_den_out":  dict(lh=1, lhs=1, dens=0, same_base=0, dprev=1, w=(0.5, 0.5), d_out=1, xd_out=0),
}
DPS_T = [1e-5, 1e-4, 0.5, 10.0]       # sigma_min / sigma_max of conf/diff_params/edm_VCTK.yaml and of the tester's sampling_params.sde_hp (1e-4, 0.5)


@pytest.mark.parametrize("B,L", [(1, 1), (2, 255), (3, 257), (3, 5001), (3, 400001)])
def test_dps_update(lib, B, L):
    """(3, 400001) exceeds the 4096 x 256 elements of one trip of the capped grid and has its row boundaries inside workgroups"""
    rs = np.random.RandomState(B * 13 + L)
    x_hat, x_den, lh = rows(rs, B, L, [0.3, 0.06, 2.0]), rows(rs, B, L, [0.05, 0.5, 0.002]), rows(rs, B, L, [1.0, 30.0, 0.01])
    base, d_prev = rows(rs, B, L, [0.3, 0.06, 2.0]), rows(rs, B, L, [5.0, 0.1, 60.0])
    lhs, dens = f32(np.resize(GAIN[[2, 0, 1]], B)), f32(np.resize(GAIN, B) * 1.0173)
    H = dict(x_hat=x_hat, x_den=x_den, lh=lh, base=base, d_prev=d_prev, lhs=lhs, dens=dens)
    D = {k: dev(v) for k, v in H.items()}
    pick = lambda key, on: (D[key], H[key]) if on else (None, None)
    worst = {}
    for (name, c), t in itertools.product(DPS_CONFIGS.items(), DPS_T):
        dt = -0.31 * t
        (lh_d, lh_h), (lhs_d, lhs_h), (dens_d, dens_h), (dp_d, dp_h) = pick("lh", c["lh"]), pick("lhs", c["lhs"]), pick("dens", c["dens"]), pick("d_prev", c["dprev"])
        base_d, base_h = (D["x_hat"], x_hat) if c["same_base"] else (D["base"], base)
        out, d_out, xd_out = Guarded((B, L)), Guarded((B, L)) if c["d_out"] else None, Guarded((B, L)) if c["xd_out"] else None
        check(lib.buddy_dps_update(P(D["x_hat"]), P(D["x_den"]), P(lh_d), P(lhs_d), P(dens_d), P(base_d), P(dp_d), t, dt, c["w"][0], c["w"][1],
                                   P(out.t), P(d_out.t) if d_out else None, P(xd_out.t) if xd_out else None, B, L, S()))
        ref = R.dps_update(x_hat, x_den, lh_h, lhs_h, dens_h, base_h, dp_h, t, dt, c["w"][0], c["w"][1])
        r_out = ratio(out.get(), ref.out, ref.out_bound)
        r_d = ratio(d_out.get(), ref.d, ref.d_bound) if d_out else 0.0
        worst[name] = max(worst.get(name, (0.0, 0.0)), (r_out, r_d), key=max)
        assert r_out <= 1.0 and r_d <= 1.0, (name, t, r_out, r_d)
        if xd_out:       # the rescaled estimate is the fp32 product itself; without a scale it is a copy
            want = x_den * dens_h[:, None] if dens_h is not None else x_den
            assert want.dtype == np.float32 and np.array_equal(bits(xd_out.get(raw=True)), bits(want)), (name, t)
    for name, (r_out, r_d) in worst.items():
        print(f"sampler_kernels dps_update B {B} L {L:>6} {name:<13} worst over t: out err/bound {r_out:.3f}, d err/bound {r_d:.3f}")


# ---- fir ------------------------------------------------------------------------------------------------------------------------------------

FIR_SHAPES = [(1, 1), (5, 9), (255, 2), (1023, 1023), (1024, 1024), (1025, 1025), (2049, 1), (2049, 2048), (2050, 2049), (700, 3000), (5000, 3000)]


def run_fir(lib, xd, hd, stride, B, L, M, adjoint):
    y = Guarded((B, L))
    check(lib.buddy_fir(P(xd), P(hd), stride, P(y.t), B, L, M, adjoint, S()))
    return y.get(raw=True)


@pytest.mark.parametrize("L,M", FIR_SHAPES)
def test_fir_per_sample(lib, L, M):
    """forward and adjoint per sample against float64; shared, packed per-row and padded per-row filters (the padding holds NaN); white and
    RIR-like decaying filters; the inner-product identity on the kernel's own outputs; row b of the batch == the batch of one, bit for bit"""
    rs = np.random.RandomState(L * 31 + M)
    B = 3
    x, g = rows(rs, B, L, GAIN), rows(rs, B, L, GAIN[::-1])
    xd, gd = dev(x), dev(g)
    for kind in ("white", "decay"):
        h = rs.standard_normal((B, M)) * GAIN[[1, 2, 0], None] * (np.exp(-np.arange(M) / (M / 5)) if kind == "decay" else 1.0)
        h = f32(h)
        hpad = np.full((B, M + 7), NAN, np.float32)
        hpad[:, :M] = h
        for layout, hd, stride, href in (("shared", dev(h[1]), 0, h[1]), ("packed", dev(h), M, h), ("padded", dev(hpad), M + 7, h)):
            y = run_fir(lib, xd, hd, stride, B, L, M, 0)
            gx = run_fir(lib, gd, hd, stride, B, L, M, 1)
            (y64, yb), (gx64, gb) = R.fir(x, href), R.fir(g, href, adjoint=True)
            assert np.isfinite(y).all() and np.isfinite(gx).all(), "filter padding leaked"
            r_f, r_a = ratio(y, y64, yb), ratio(gx, gx64, gb)
            # <fir(x), g> == <x, fir_adj(g)>: the two sides, each within its per-sample bound of the float64 pair, which agrees exactly
            lhs, rhs = (y.astype(np.float64) * g).sum(axis=1), (x * gx.astype(np.float64)).sum(axis=1)
            tol = yb[:, 0] * np.abs(g).sum(axis=1, dtype=np.float64) + gb[:, 0] * np.abs(x).sum(axis=1, dtype=np.float64)
            r_ip = float((np.abs(lhs - rhs) / tol).max())
            print(f"sampler_kernels fir L {L:>4} M {M:>4} {kind:<5} {layout:<6} err/bound forward {r_f:.3f} adjoint {r_a:.3f} inner product {r_ip:.3f}")
            assert r_f <= 1.0 and r_a <= 1.0 and r_ip <= 1.0
            for b in range(B):
                hb = hd if stride == 0 else hd[b]
                assert np.array_equal(bits(run_fir(lib, xd[b:b + 1], hb, stride, 1, L, M, 0)[0]), bits(y[b]))
                assert np.array_equal(bits(run_fir(lib, gd[b:b + 1], hb, stride, 1, L, M, 1)[0]), bits(gx[b]))


def test_fast_apply_RIR_per_utterance_filters():
    """a (3, M) filter: forward == the three single-utterance calls bit for bit, and float64; backward == the float64 adjoint"""
    from buddy_amd.utils.reverb_utils import fast_apply_RIR
    L, M = 2050, 1025
    rs = np.random.RandomState(5)
    x, g = rows(rs, 3, L, GAIN), rows(rs, 3, L, GAIN[::-1])
    h = f32(rs.standard_normal((3, M)) * GAIN[[1, 2, 0], None] * np.exp(-np.arange(M) / (M / 5)))
    xd, hd = dev(x).requires_grad_(True), dev(h)
    y = fast_apply_RIR(xd, hd)
    y.backward(dev(g))
    torch.cuda.synchronize()
    for b in range(3):
        for hb in (hd[b], hd[b:b + 1]):
            assert torch.equal(fast_apply_RIR(xd[b:b + 1].detach(), hb)[0], y[b].detach())
    (y64, yb), (gx64, gb) = R.fir(x, h), R.fir(g, h, adjoint=True)
    r_f, r_b = ratio(y.detach().cpu().numpy(), y64, yb), ratio(xd.grad.cpu().numpy(), gx64, gb)
    print(f"sampler_kernels fast_apply_RIR (3, {M}) filter L {L} err/bound forward {r_f:.3f} backward {r_b:.3f}")
    assert r_f <= 1.0 and r_b <= 1.0
    y1 = fast_apply_RIR(xd.detach(), hd[1])                     # one shared filter for all rows
    assert ratio(y1.cpu().numpy(), *R.fir(x, h[1])) <= 1.0
    with pytest.raises(ValueError):
        fast_apply_RIR(xd.detach(), hd[:2])


# ---- _step_hip with the network and the operator stubbed ------------------------------------------------------------------------------------

class _Fixed:
    def __init__(self, t):
        self.t = t

    def randn(self, shape):
        assert tuple(shape) == tuple(self.t.shape)
        return self.t


STEP_T = {"order 1": (1, 0.0712, 0.0655), "order 2": (2, 0.0712, 0.0655), "order 2, last step": (2, 1.0e-4, 0.0)}


@pytest.mark.parametrize("case", list(STEP_T))
@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("gamma", [0.0, 0.2487])
def test_step_hip_in_isolation(lib, case, rescale, gamma):
    """EulerHeunSamplerDPS.step on fp32 device tensors (_step_hip) with _eval_parts replaced by given tensors that do not depend on its input, so
    the kernels' errors propagate linearly; the bound comes with the arbiter's value (_sampler_ref.step)"""
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.testing.EulerHeunSamplerDPS import EulerHeunSamplerDPS
    order, t_i, t_next = STEP_T[case]
    B, L = 2, 4097
    args = compose(overrides=[f"tester.sampling_params.order={order}",
                              f"tester.posterior_sampling.constraint_speech_magnitude.use={'true' if rescale else 'false'}"])
    smp = EulerHeunSamplerDPS(torch.nn.Identity(), instantiate(args.diff_params), args)
    rs = np.random.RandomState(order * 4 + rescale * 2 + (gamma > 0))
    x, eps = rows(rs, B, L, [0.08, 0.3]), f32(rs.standard_normal((B, L)))
    evals = [(rows(rs, B, L, [30.0, 0.2]), f32([0.011, -3.0]), rows(rs, B, L, [0.002, 0.4])),
             (rows(rs, B, L, [0.5, 8.0]), f32([40.0, 0.5]), rows(rs, B, L, [0.07, 0.01]))]
    on_dev = [tuple(dev(a) for a in e) for e in evals]
    calls = []

    def eval_parts(x_in, t, blind):
        assert x_in.shape == (B, L) and x_in.is_cuda and not blind
        calls.append(float(t))
        return on_dev[len(calls) - 1]
    smp._eval_parts = eval_parts
    smp.noise = [_Fixed(torch.from_numpy(eps[b:b + 1])) for b in range(B)]
    x_next, x_den = smp.step(dev(x), t_i, t_next, gamma, blind=False)
    torch.cuda.synchronize()
    csm = args.tester.posterior_sampling.constraint_speech_magnitude
    (rx, rd), (bx, bd) = R.step(x, eps, t_i, t_next, gamma, order, evals, rescale, csm.speech_scaling)
    t_hat = R.host_scalars(t_i, t_next, gamma)[0]
    two = order == 2 and t_next != 0
    assert calls == ([t_hat, float(np.float32(t_next))] if two else [t_hat])
    r_x = ratio(x_next.cpu().numpy(), rx, bx)
    if two:                          # the corrector returns the raw second estimate
        assert torch.equal(x_den, on_dev[1][2])
        r_d = 0.0
    elif rescale:                    # the first estimate, rescaled
        r_d = ratio(x_den.cpu().numpy(), rd, bd)
        assert np.abs(rd).max() > 0 and not np.array_equal(bits(x_den.cpu().numpy()), bits(evals[0][2]))
    else:
        assert torch.equal(x_den, on_dev[0][2])
        r_d = 0.0
    print(f"sampler_kernels step {case:<18} rescale {rescale!s:<5} gamma {gamma:<6} err/bound x_next {r_x:.3f} x_den {r_d:.3f}")
    assert r_x <= 1.0 and r_d <= 1.0
