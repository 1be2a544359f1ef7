"""GPU: the two optimizer entries of data-parallel training alone -- ``buddy_optim_step_scaled`` (the step on a gradient buffer that holds the SUM
over the ranks, averaged by ``grad_scale`` inside the pass) against float64 numpy, and ``buddy_optim_checksum`` against numpy's uint64
wrap-around arithmetic.

Tolerances of the step: the ones tests/test_hip_optim.py derives from fp32 rounding (u = 2^-24), unchanged -- the scale enters as one more
double multiplication, whose rounding (2^-53) is far below them:
  m, v     4 u relative to the sum of the magnitudes of their two terms
  p_new    from p = 0: 1e-6 relative; with p of order 1: 2 u |p64| = 2^-23 |p64|
  EMA      4 u of its two terms (2e-6 where p starts at 0)
  frozen   p, m, v bit for bit their inputs; the EMA is still updated there
The reference is that file's restatement with g -> grad_scale g and sq -> grad_scale^2 sq, restated here.  With grad_scale = 1 the entry must
give the bytes of ``buddy_optim_step``.  The checksum is an integer: it is compared for equality."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
B1, B2, LR, S = 0.9, 0.999, 1e-4, 0.75


def _lib():
    from buddy_amd import _lib
    return _lib, _lib.require_gpu()


# ---- the references (numpy only: tests/test_ddp_host.py checks checksum_ref by hand without a GPU) -----------------------------------------
def checksum_ref(x):
    """sum_i bits(x[i]) * (2 i + 1) mod 2^64 in numpy's wrap-around uint64 arithmetic"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    k = np.uint64(2) * np.arange(bits.size, dtype=np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):
        return int((bits * k).sum(dtype=np.uint64))


def reference_step(p, g, m, v, ema, sq, max_norm, grad_scale, b1, b2, eps, lr, t, s, frozen):
    """float64: clip_grad_norm_ + torch's single-tensor Adam + the reference's EMA on the AVERAGED gradient grad_scale * g, whose squared
    norm is grad_scale^2 * sq"""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    g = grad_scale * g
    sq = grad_scale * grad_scale * sq
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
    return pn, mn, vn, en, np.abs(t1) + np.abs(t2), np.abs(s1) + np.abs(s2), mask, coef


def errors(got, ref, ema, from_zero):
    """(m error / u, v error / u, p relative error, EMA error relative to its terms) of ``got`` = (p, m, v, ema) against reference_step's tuple"""
    pn, mn, vn, en, msc, vsc, mask, _ = ref
    gp, gm, gv, ge = (None if a is None else a.astype(np.float64) for a in got)
    live = ~mask
    if not live.any():
        return 0.0, 0.0, 0.0, 0.0
    em = (np.abs(gm - mn)[live] / (msc[live] + 1e-300)).max() / U
    ev = (np.abs(gv - vn)[live] / (vsc[live] + 1e-300)).max() / U
    ep = (np.abs(gp - pn)[live] / (np.abs(pn[live]) + 1e-300)).max()
    ee = 0.0 if ge is None else (np.abs(ge - en) / (np.abs(ema.astype(np.float64)) * S + np.abs(pn) * (1 - S) + 1e-300)).max()
    return em, ev, ep, ee


def within(err, from_zero):
    em, ev, ep, ee = err
    return em <= 4 and ev <= 4 and ep <= (1e-6 if from_zero else 2 * U) and ee <= (2e-6 if from_zero else 4 * U)


def make(n, from_zero, seed):
    rs = np.random.RandomState(seed)
    g = (rs.standard_normal(n) * np.exp(rs.uniform(-6, 1, n))).astype(np.float32)
    # "of order 1": magnitudes in [0.5, 2), so that the 1e-4-sized update never cancels p (the bound is relative to |p_new|)
    p = np.zeros(n, np.float32) if from_zero else (rs.choice([-1.0, 1.0], n) * rs.uniform(0.5, 2.0, n)).astype(np.float32)
    m = (0.1 * rs.standard_normal(n)).astype(np.float32)
    v = (0.01 * rs.standard_normal(n) ** 2).astype(np.float32)
    ema = rs.standard_normal(n).astype(np.float32)
    return p, g, m, v, ema


def device_sqnorm(g):
    L, lib = _lib()
    chunk = int(lib.buddy_optim_sqnorm_chunk())
    part = torch.full(((g.numel() + chunk - 1) // chunk,), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    L.check(lib.buddy_optim_sqnorm(L.ptr(g), g.numel(), part.data_ptr(), out.data_ptr(), L.stream_ptr()))
    return out


def run_step(entry, arrays, n, max_norm, grad_scale, eps, t, frozen):
    """one launch of ``buddy_optim_step_scaled`` (or, grad_scale None, ``buddy_optim_step``) on device copies; returns (p, m, v, ema, g) as numpy"""
    L, lib = _lib()
    d = [None if a is None else torch.from_numpy(a).cuda() for a in arrays]
    sq = device_sqnorm(d[1]) if max_norm > 0 else None
    fz = (C.c_longlong * max(2 * len(frozen), 1))(*[x for r in frozen for x in r])
    head = (L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(d[4]), n, None if sq is None else sq.data_ptr(), max_norm, B1, B2, eps,
            LR / (1 - B1 ** t), math.sqrt(1 - B2 ** t), S)
    if entry == "scaled":
        L.check(lib.buddy_optim_step_scaled(*head, grad_scale, fz, len(frozen), L.stream_ptr()))
    else:
        L.check(lib.buddy_optim_step(*head, fz, len(frozen), L.stream_ptr()))
    torch.cuda.synchronize()
    return [None if a is None else a.cpu().numpy() for a in (d[0], d[2], d[3], d[4], d[1])]


SCALES = [1 / 2, 1 / 3, 1 / 8]
CLIPS = ["active", "inactive", "off"]
SIZES = [3, 4097, 100003]


def max_norm_for(clip, avg_norm):
    return {"active": 0.5 * avg_norm, "inactive": 2.0 * avg_norm / min(SCALES), "off": 0.0}[clip]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("grad_scale", SCALES, ids=["half", "third", "eighth"])
def test_scaled_step_vs_float64(grad_scale, clip, n):
    from_zero = n == 4097               # both p bounds run: from p = 0 at one size, p of order 1 at the others
    t = 1
    p, g, m, v, ema = make(n, from_zero, 7 * n + CLIPS.index(clip))
    sq64 = float(np.sum(g.astype(np.float64) ** 2))
    max_norm = max_norm_for(clip, grad_scale * math.sqrt(sq64))
    got = run_step("scaled", (p, g, m, v, ema), n, max_norm, grad_scale, 1e-8, t, [])
    assert np.array_equal(got[4], g), "the gradient buffer must stay as it was: the sum, unscaled and unclipped"
    ref = reference_step(p, g, m, v, ema, sq64, max_norm, grad_scale, B1, B2, 1e-8, LR, t, S, [])
    assert (ref[7] < 1.0) == (clip == "active")
    err = errors(got[:4], ref, ema, from_zero)
    print(f"scale {grad_scale:.3f} clip {clip} n {n}: m {err[0]:.2f} u, v {err[1]:.2f} u, p rel {err[2]:.2e}, ema {err[3]:.2e}")
    assert within(err, from_zero), err


def test_scaled_step_frozen_range_at_an_odd_offset():
    n, grad_scale, frozen = 100003, 1 / 3, [(4099, 4099 + 32), (100001, 100003)]       # 4099 = 4 * 1024 + 3: both ends straddle a 16-byte word
    p, g, m, v, ema = make(n, False, 21)
    sq64 = float(np.sum(g.astype(np.float64) ** 2))
    max_norm = 0.5 * grad_scale * math.sqrt(sq64)
    got = run_step("scaled", (p, g, m, v, ema), n, max_norm, grad_scale, 1e-8, 1, frozen)
    ref = reference_step(p, g, m, v, ema, sq64, max_norm, grad_scale, B1, B2, 1e-8, LR, 1, S, frozen)
    mask = ref[6]
    assert mask.sum() == 34 and np.array_equal(got[4], g)
    assert within(errors(got[:4], ref, ema, False), False)
    for a, b in ((got[0], p), (got[1], m), (got[2], v)):
        assert a[mask].tobytes() == b[mask].tobytes(), "p, m, v inside a frozen range must keep their bits"
    assert not np.array_equal(got[3][mask], ema[mask]), "the EMA runs inside a frozen range too"


@pytest.mark.parametrize("grad_scale", SCALES, ids=["half", "third", "eighth"])
def test_clip_acts_on_the_average_not_on_the_sum(grad_scale):
    """||g|| > max_norm > grad_scale ||g||: the sum would be clipped, the average is not.  A coefficient computed from the norm of the sum
    (the unscaled buffer) is shown to miss the bounds, so the check can tell the two apart."""
    n = 4097
    p, g, m, v, ema = make(n, False, 33)
    sq64 = float(np.sum(g.astype(np.float64) ** 2))
    norm = math.sqrt(sq64)
    max_norm = math.sqrt(grad_scale) * norm                    # the geometric mean of the two norms
    assert norm > max_norm > grad_scale * norm
    got = run_step("scaled", (p, g, m, v, ema), n, max_norm, grad_scale, 1e-8, 1, [])
    ref = reference_step(p, g, m, v, ema, sq64, max_norm, grad_scale, B1, B2, 1e-8, LR, 1, S, [])
    assert ref[7] == 1.0
    assert within(errors(got[:4], ref, ema, False), False)
    # the wrong step: clip coefficient from the unscaled norm, i.e. the averaged gradient shrunk by max_norm / ||g|| < 1 once more
    wrong = reference_step(p, (max_norm / (norm + 1e-6)) * g.astype(np.float64), m, v, ema, sq64, 0.0, grad_scale, B1, B2, 1e-8, LR, 1, S, [])
    assert not within(errors(got[:4], wrong, ema, False), False)
    assert np.array_equal(got[4], g)


@pytest.mark.parametrize("max_norm,frozen", [(1.0, []), (0.0, []), (1e9, [(4099, 4131)])], ids=["clip", "no_clip", "frozen"])
def test_scale_one_keeps_the_bits_of_the_unscaled_entry(max_norm, frozen):
    n = 100003
    arrays = make(n, False, 55)
    a = run_step("scaled", arrays, n, max_norm, 1.0, 1e-8, 3, frozen)
    b = run_step("plain", arrays, n, max_norm, None, 1e-8, 3, frozen)
    for name, x, y in zip(("p", "m", "v", "ema", "g"), a, b):
        assert x.tobytes() == y.tobytes(), name
    assert not np.array_equal(a[0], arrays[0])


@pytest.mark.parametrize("bad", [0.0, -0.5, float("nan"), float("inf")])
def test_grad_scale_must_be_finite_and_positive(bad):
    L, _ = _lib()
    n = 8
    arrays = make(n, False, 1)
    with pytest.raises(L.BuddyHipError):
        run_step("scaled", arrays, n, 0.0, bad, 1e-8, 1, [])


# ---- the checksum ----------------------------------------------------------------------------------------------------------------------------
def device_checksum(x, misalign):
    """``x``: float32 numpy -> the device checksum; ``misalign``: the buffer starts 4 bytes past a 16-byte boundary.  Workspace and output
    hold garbage before the call."""
    L, lib = _lib()
    n = x.size
    chunk = int(lib.buddy_optim_sqnorm_chunk())
    buf = torch.empty(n + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    d = buf[1:1 + n] if misalign else buf[:n]
    assert d.data_ptr() % 16 == (4 if misalign else 0)
    d.copy_(torch.from_numpy(x))
    assert d.cpu().numpy().tobytes() == x.tobytes(), "the copy to the device must keep every bit pattern"
    part = torch.full(((n + chunk - 1) // chunk,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    out = torch.full((1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    L.check(lib.buddy_optim_checksum(L.ptr(d), n, part.data_ptr(), out.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    return int(out.cpu().numpy().view(np.uint64)[0])


def random_bits(n, seed):
    """floats of arbitrary bit patterns except NaNs (a copy might quieten a signalling NaN): exponent field below all-ones"""
    rs = np.random.RandomState(seed)
    bits = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    bits = np.where((bits >> 23) & 0xFF == 0xFF, bits & np.uint32(0xBFFFFFFF), bits).astype(np.uint32)
    return bits.view(np.float32).copy()


def flip(x, i, bit=0):
    y = x.copy()
    y.view(np.uint32)[i] ^= np.uint32(1 << bit)
    return y


@pytest.mark.parametrize("misalign", [True, False], ids=["plus4bytes", "aligned"])
def test_checksum_equals_numpy_uint64(misalign):
    _, lib = _lib()
    chunk = int(lib.buddy_optim_sqnorm_chunk())
    for n in (1, 3, 4, chunk - 1, chunk, chunk + 1, 100003):
        x = random_bits(n, n % 977)
        got, ref = device_checksum(x, misalign), checksum_ref(x)
        print(f"checksum n={n} misalign={misalign}: {got:#018x}")
        assert got == ref, (n, hex(got), hex(ref))


def test_checksum_notices_every_single_edit():
    _, lib = _lib()
    chunk = int(lib.buddy_optim_sqnorm_chunk())
    n = chunk + 1027                     # two workgroups; the second has full words, and a scalar tail on the misaligned buffer
    x = random_bits(n, 5)
    base = device_checksum(x, True)
    assert base == checksum_ref(x)
    i, j = 17, chunk + 500
    assert x.view(np.uint32)[i] != x.view(np.uint32)[j]
    swapped = x.copy()
    swapped[[i, j]] = x[[j, i]]
    edits = {"first element, lowest bit": flip(x, 0), "first element, sign bit": flip(x, 0, 31), "last element": flip(x, n - 1),
             "first element of the second chunk": flip(x, chunk), "two unequal elements swapped": swapped}
    for name, y in edits.items():
        got = device_checksum(y, True)
        assert got == checksum_ref(y), name
        assert got != base, name
    z = np.zeros(5, np.float32)
    nz = z.copy()
    nz[3] = -0.0
    a, b = device_checksum(z, True), device_checksum(nz, True)
    assert a == 0 and b == checksum_ref(nz) == 0x80000000 * 7 and a != b, "-0.0 and 0.0 are different bit patterns"


def test_checksum_rejects_bad_arguments():
    L, lib = _lib()
    x = torch.zeros(8, device="cuda")
    w = torch.zeros(2, dtype=torch.int64, device="cuda")
    for args in ((None, 8, w.data_ptr(), w.data_ptr()), (L.ptr(x), 0, w.data_ptr(), w.data_ptr()), (L.ptr(x), 8, None, w.data_ptr()),
                 (L.ptr(x), 8, w.data_ptr(), w.data_ptr() + 4)):
        with pytest.raises(L.BuddyHipError):
            L.check(lib.buddy_optim_checksum(*args, L.stream_ptr()))
