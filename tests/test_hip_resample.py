"""GPU: the rational polyphase resampler (csrc/resample.hip) through the C ABI against float64 scipy (resample_poly with the same taps), at ragged
lengths and every audio ratio the real-recording path meets; exact tap layout, row independence, guard words, argument errors.

Tolerance, per case and elementwise: |y - y64| <= (T + 3) 2^-23 S max|x| with T = ceil(Nh / up) taps per output and S = max over the polyphase
branches of sum_k |h[p + k up]|: the taps rounded to fp32 (2^-24 S max|x|), one rounding per fused multiply-add of a running sum that never
exceeds S max|x| (T 2^-24 S max|x|), doubled.  S is 1.98 .. 2.10 and T <= 145 here, so the bound is <= 3.7e-5 max|x|; measured maxima are two
orders below it (profiles/resample_accuracy.txt)."""
import math

import numpy as np
import pytest
import torch
from scipy import signal

from buddy_amd import _lib
from buddy_amd.utils.resample import design_filter, out_length, resample

pytestmark = pytest.mark.gpu

RATIOS = [(1, 3), (3, 1), (1, 2), (2, 1), (3, 2), (160, 441), (441, 160)]
LENGTHS = [1, 7, 1023, 1024, 1025, 4097, 50001]
GUARD = 64


def oracle(x, up, down, h):
    return signal.resample_poly(np.asarray(x, np.float64), up, down, axis=-1, window=np.asarray(h, np.float64) / up, padtype="constant")


def bound(h, up, xmax):
    T = math.ceil(len(h) / up)
    S = max(np.abs(h[p::up]).sum() for p in range(up))
    return (T + 3) * 2.0 ** -23 * S * xmax


def call(x, h32, up, down, Lout=None, fill=float("nan")):
    """buddy_resample on x (B, Lin) -> (rc, the whole NaN-filled allocation of B * Lout + GUARD floats)"""
    lib = _lib.require_gpu()
    B, Lin = x.shape
    Lout = out_length(Lin, up, down) if Lout is None else Lout
    buf = torch.full((B * max(Lout, 0) + GUARD,), fill, dtype=torch.float32, device="cuda")
    rc = lib.buddy_resample(_lib.ptr(x), B, Lin, _lib.ptr(h32), h32.numel(), up, down, _lib.ptr(buf), Lout, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, buf


def run(x, h32, up, down):
    rc, buf = call(x, h32, up, down)
    assert rc == 0, _lib.load().buddy_last_error().decode()
    B, Lout = x.shape[0], out_length(x.shape[1], up, down)
    assert torch.isnan(buf[B * Lout:]).all(), "guard words written"
    y = buf[:B * Lout].reshape(B, Lout)
    assert torch.isfinite(y).all()
    return y


def taps(up, down):
    h = design_filter(up, down)
    return h, torch.from_numpy(h.astype(np.float32)).cuda()


@pytest.mark.parametrize("up,down", RATIOS)
def test_against_float64_scipy(up, down):
    h, h32 = taps(up, down)
    rs = np.random.RandomState(up * 1000 + down)
    for Lin in LENGTHS:
        for B in (1, 3):
            x = rs.standard_normal((B, Lin)).astype(np.float32)
            y = run(torch.from_numpy(x).cuda(), h32, up, down).cpu().numpy().astype(np.float64)
            ref = oracle(x, up, down, h)
            assert y.shape == ref.shape == (B, math.ceil(Lin * up / down))
            err, tol = np.abs(y - ref).max(), bound(h, up, np.abs(x).max())
            print(f"resample {up:>3}/{down:<3} Lin {Lin:>6} B {B}  max|err| {err:.3e}  bound {tol:.3e}")
            assert err <= tol


@pytest.mark.parametrize("up,down,zeros,Lin", [(1, 16, 24, 40000), (2, 1, 10000, 3000), (1, 1024, 24, 70000)])
def test_input_span_longer_than_one_stage(up, down, zeros, Lin):
    """a large down / up or a very long filter: the inputs of one output tile exceed one LDS stage and are staged in several segments"""
    h = design_filter(up, down, zeros=zeros)
    h32 = torch.from_numpy(h.astype(np.float32)).cuda()
    x = np.random.RandomState(7).standard_normal((2, Lin)).astype(np.float32)
    y = run(torch.from_numpy(x).cuda(), h32, up, down).cpu().numpy().astype(np.float64)
    ref = oracle(x, up, down, h)
    err, tol = np.abs(y - ref).max(), bound(h, up, np.abs(x).max())
    print(f"resample {up}/{down} Nh {len(h)} Lin {Lin}  max|err| {err:.3e}  bound {tol:.3e}")
    assert y.shape == ref.shape and err <= tol


def test_rows_are_independent():
    for up, down in [(160, 441), (3, 1), (1, 3)]:
        _, h32 = taps(up, down)
        x = torch.randn(3, 4097, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        x[1] = 0
        y = run(x, h32, up, down)
        assert torch.equal(y[1], torch.zeros_like(y[1]))
        for r in (0, 2):
            assert torch.equal(y[r], run(x[r:r + 1].contiguous(), h32, up, down)[0])


@pytest.mark.parametrize("up,down", RATIOS)
def test_tap_layout_exact(up, down):
    """a unit impulse at m reads out the taps h[n*down - m*up + c]: a shifted phase or an off-by-one at either edge cannot pass"""
    h, h32 = taps(up, down)
    hf, c = h.astype(np.float32), (len(h) - 1) // 2
    for Lin in (7, 1025):
        Lout = out_length(Lin, up, down)
        ms = [0, Lin - 1, Lin // 3]
        x = torch.zeros(len(ms), Lin, device="cuda")
        for r, m in enumerate(ms):
            x[r, m] = 1.0
        y = run(x, h32, up, down).cpu()
        for r, m in enumerate(ms):
            idx = np.arange(Lout, dtype=np.int64) * down - m * up + c
            ok = (idx >= 0) & (idx < len(h))
            want = np.where(ok, hf[np.clip(idx, 0, len(h) - 1)], np.float32(0))
            assert torch.equal(y[r], torch.from_numpy(want)), (up, down, Lin, m)


def test_degenerate_filter_copies():
    x = torch.randn(3, 5000, device="cuda")
    y = run(x, torch.ones(1, device="cuda"), 1, 1)
    assert torch.equal(y, x)


def test_argument_errors():
    lib = _lib.require_gpu()
    h, h32 = taps(3, 2)
    x = torch.randn(2, 100, device="cuda")
    Lout = out_length(100, 3, 2)
    he = torch.ones(4, device="cuda")
    hbig = torch.zeros(65539, device="cuda")
    P = _lib.ptr
    y = torch.full((2 * 400 + GUARD,), float("nan"), device="cuda")
    st = _lib.stream_ptr()
    bad = {
        "B < 1": (P(x), 0, 100, P(h32), len(h), 3, 2, P(y), Lout),
        "Lin < 1": (P(x), 2, 0, P(h32), len(h), 3, 2, P(y), 0),
        "up < 1": (P(x), 2, 100, P(h32), len(h), 0, 2, P(y), 0),
        "down < 1": (P(x), 2, 100, P(h32), len(h), 3, 0, P(y), Lout),
        "gcd": (P(x), 2, 100, P(h32), len(h), 6, 4, P(y), Lout),
        "up > 1024": (P(x), 2, 100, P(h32), len(h), 1025, 2, P(y), out_length(100, 1025, 2)),
        "down > 1024": (P(x), 2, 100, P(h32), len(h), 3, 1025, P(y), out_length(100, 3, 1025)),
        "Nh even": (P(x), 2, 100, P(he), 4, 3, 2, P(y), Lout),
        "Nh > 65537": (P(x), 2, 100, P(hbig), 65539, 3, 2, P(y), Lout),
        "Lout - 1": (P(x), 2, 100, P(h32), len(h), 3, 2, P(y), Lout - 1),
        "Lout + 1": (P(x), 2, 100, P(h32), len(h), 3, 2, P(y), Lout + 1),
        "x null": (None, 2, 100, P(h32), len(h), 3, 2, P(y), Lout),
        "h null": (P(x), 2, 100, None, len(h), 3, 2, P(y), Lout),
        "y null": (P(x), 2, 100, P(h32), len(h), 3, 2, None, Lout),
    }
    assert lib.buddy_resample(P(x), 2, 100, P(h32), len(h), 3, 2, P(y), Lout, st) == 0      # the good call, so that a stale message cannot pass
    y.fill_(float("nan"))
    for why, a in bad.items():
        rc = lib.buddy_resample(*a, st)
        torch.cuda.synchronize()
        assert rc == 2, why                                          # BUDDY_ERR_ARG
        assert lib.buddy_last_error().decode().startswith("buddy_resample"), why
        assert torch.isnan(y).all(), why
    with pytest.raises(_lib.BuddyHipError):
        resample(torch.zeros(1, 100, device="cuda"), 16000, 1)        # 1 / 16000: `down` above 1024, through the Python entry


def test_round_trip_16k_48k_16k():
    rs = np.random.RandomState(5)
    X = np.fft.rfft(rs.standard_normal((2, 8000)))
    X[:, int(0.8 * X.shape[1]):] = 0                                  # band-limited to 0.4 of the 16 kHz rate
    x = np.fft.irfft(X, 8000).astype(np.float32)
    xg = torch.from_numpy(x).cuda()
    y1 = resample(xg, 16000, 48000)
    y2 = resample(y1, 48000, 16000)
    assert y1.shape == (2, 24000) and y2.shape == (2, 8000)
    assert torch.equal(resample(xg[0], 16000, 48000), y1[0])           # (L,) in, (L,) out
    hu, hd = design_filter(3, 1), design_filter(1, 3)
    r1 = oracle(x, 3, 1, hu)
    r2 = oracle(r1, 1, 3, hd)
    tol = bound(hu, 3, np.abs(x).max()) + bound(hd, 1, np.abs(r1).max())
    err = np.abs(y2.cpu().numpy().astype(np.float64) - r2).max()
    print(f"round trip 16k -> 48k -> 16k  max|err| {err:.3e}  bound {tol:.3e}")
    assert err <= tol
