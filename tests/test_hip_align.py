"""GPU: the time alignment (csrc/align.hip, buddy_amd/utils/metrics.py align) against its float64 restatement tests/_align_ref.py: the correlation
element by element on ragged rows with NaN behind every row, the lag and flags exactly, undefined rows, row independence, the trimmed pair with
guard words around it, the effect on ``evaluate``, the tester writing the further columns and the stand-alone tool reading them back.  Seeded white
noise unless stated."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _align_ref as A  # noqa: E402
import _metrics_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_clean, synth_rir  # noqa: E402
from buddy_amd.utils import metrics as M  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 12345.0
ERR_ARG = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    return _lib.require_gpu()


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def padded(rows, ld, fill=np.nan):
    """rows of their own lengths -> (B, ld) float32 on the device with ``fill`` behind every row (NaN: a read past the end would show)"""
    out = np.full((len(rows), ld), fill, np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return torch.from_numpy(out).cuda()


def guarded(n, dtype, fill):
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


def split(buf, n, fill):
    """the first n words; asserts the guard words behind them are intact"""
    a = buf.cpu().numpy()
    assert np.all(a[n:] == fill), "guard words overwritten"
    return a[:n]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def xcorr_lag(lib, es, xs, K, ld=None):
    """buddy_xcorr_lag on rows of their own lengths (NaN behind each, guard words behind every output): lag (B,), out (B, 2), flags (B,), r (B, 2K + 1)"""
    B, lens = len(es), [len(e) for e in es]
    ld = max(lens) + 5 if ld is None else ld
    e_d, x_d, lens_d = padded(es, ld), padded(xs, ld), dev_i32(lens)
    nl = 2 * K + 1
    lag, flags = guarded(B, torch.int32, -77), guarded(B, torch.int32, -77)
    out, r = guarded(2 * B, torch.float64, SENTINEL), guarded(B * nl, torch.float64, SENTINEL)
    nbytes = lib.buddy_xcorr_lag_workspace(B, max(lens), K)
    assert nbytes > 0
    ws = guarded(nbytes // 8, torch.float64, SENTINEL)
    rc = lib.buddy_xcorr_lag(_lib.ptr(e_d), _lib.ptr(x_d), lens_d.data_ptr(), B, ld, K, lag.data_ptr(), out.data_ptr(), flags.data_ptr(), r.data_ptr(),
                             ws.data_ptr(), nbytes, _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    split(ws, nbytes // 8, SENTINEL)
    return split(lag, B, -77), split(out, 2 * B, SENTINEL).reshape(B, 2), split(flags, B, -77), split(r, B * nl, SENTINEL).reshape(B, nl)


# ---- 1. r against the restatement ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ragged_rows(T):
    """pairs of the lengths T - 1, T, T + 1, 2T + 3 (T = samples per chunk), 2, 3 and 257: the estimate is the clean row delayed by 2 plus noise, with
    an offset so that the means matter"""
    rs = np.random.RandomState(101)
    es, xs = [], []
    for n in (T - 1, T, T + 1, 2 * T + 3, 2, 3, 257):
        x = rs.standard_normal(n).astype(np.float32)
        e = (A.shift(x, min(2, n - 1)) + 0.25 * rs.standard_normal(n) + 0.5).astype(np.float32)
        es.append(e)
        xs.append(x)
    return tuple(es), tuple(xs)


@pytest.mark.parametrize("which", ["0", "1", "Lt-1", "Lt", "Lt+1"])
def test_r_vs_reference(lib, which):
    """r_out element by element against the float64 restatement, on one ragged batch with NaN behind every row (so r must come out finite), for the
    windows K = 0, 1, Lt - 1, Lt, Lt + 1 (Lt = lags per tile; 2K + 1 then lies on both sides of two tiles) and the row lengths around the chunk size
    T; the rows of 2, 3 and 257 samples have K >= n from K = Lt - 1 on.

    The bound, u = 2^-53.  The fp32 inputs convert to double exactly.  A term of r[k] is fl(fl(e - me) fl(x - mx)): each subtraction rounds once
    (relative u of its result), the product once (not at all inside a fused multiply-add), so |term - e~ x~| <= 3u |e~| |x~| to first order.  Adding
    N <= n terms in any order rounds at most N - 1 times, each time by at most u times a partial sum that is at most sum |terms|: (n - 1) u
    sum_m |e~[m + k]| |x~[m]| more.  Together <= (n + 2) u S[k], stated as (n + 4) u S[k], S[k] = sum_m |e~[m + k]| |x~[m]|.  On top comes the rounding of the
    two means themselves: a mean from n - 1 additions and a division is off by at most n u mean|e|, which moves every e~ by that much and r[k] by
    at most n u (mean|e| sum_m |x~[m]| + mean|x| sum_m |e~[m + k]|), the sums over the m of lag k.  F[k] is the sum of the two figures
    (``_align_ref.bound``); it holds for the library and, with room, for the restatement (its mean is exactly rounded), so they differ by at most
    2 F[k].  Asserted: |got - want| <= 4 F[k].  The worst measured ratio |got - want| / F[k] is printed; profiles/align_accuracy.txt records the lines."""
    T, Lt = lib.buddy_align_tile(), lib.buddy_align_lag_tile()
    K = {"0": 0, "1": 1, "Lt-1": Lt - 1, "Lt": Lt, "Lt+1": Lt + 1}[which]
    es, xs = ragged_rows(T)
    lag, out, flags, r = xcorr_lag(lib, es, xs, K)
    assert np.all(np.isfinite(r)), "r is not finite: something behind a row's end was read"
    worst = 0.0
    for b, (e, x) in enumerate(zip(es, xs)):
        want, F = A.xcorr(e, x, K)[0], A.bound(e, x, K)
        err = np.abs(r[b] - want)
        ratio = float(np.max(np.where(F > 0, err / np.where(F > 0, F, 1.0), 0.0)))
        worst = max(worst, ratio)
        print(f"xcorr K {K:4d} row {b} n {len(e):5d}: max |got - want| {err.max():.3e}  max F {F.max():.3e}  worst ratio {ratio:.2e} (asserted <= 4)")
        assert np.all(err <= 4.0 * F), (b, int(np.argmax(err - 4.0 * F)) - K)
        assert np.all(r[b][F == 0.0] == 0.0)                                              # lags without a common sample
        if K >= 2 and len(e) >= 257:
            assert lag[b] == 2 and flags[b] == 1                                          # what the rows were built with
    print(f"xcorr K {K:4d}: worst ratio over the batch {worst:.2e}")


# ---- 2. the lag, exactly -------------------------------------------------------------------------------------------------------------------------
K_EXACT, N_EXACT = 24, 3000


@functools.lru_cache(maxsize=None)
def shifted_pairs():
    """per true shift d in 0, +-1, +-(K - 1), +-K: a copy delayed by d plus 10 % independent noise, the same inverted, and a low-passed (speech-like)
    pair; cut from a longer signal, so nothing is zero-filled"""
    rs = np.random.RandomState(202)
    K, n = K_EXACT, N_EXACT
    b_lp, a_lp = signal.butter(4, 0.25)
    es, xs, truth = [], [], []
    for d in (0, 1, -1, K - 1, -(K - 1), K, -K):
        for kind in ("noisy", "inverted", "lowpass"):
            src = rs.standard_normal(n + 2 * K + 200)
            if kind == "lowpass":
                src = signal.lfilter(b_lp, a_lp, src)[200:]
            x = src[K:K + n]
            e = src[K - d:K - d + n] + 0.1 * np.std(src) * rs.standard_normal(n)         # e[m + d] = x[m] + noise
            es.append((-e if kind == "inverted" else e).astype(np.float32))
            xs.append(x.astype(np.float32))
            truth.append((d, kind))
    return tuple(es), tuple(xs), tuple(truth)


def rho_frac_bounds(e, x, K, d, r, F):
    """first-order bounds on rho and frac from the bound F on r: rho = r[d] / sqrt(Ee Ex), each energy within (n + 4) u E + 2 n u mean|.| sum|.~| of its
    exact value (the same derivation, k = 0, both factors the same signal), a square root, a product and a division of u each; frac =
    0.5 (a - c) / (a - 2b + c) by its partial derivatives in a, b, c, and three roundings of u"""
    n = len(e)
    et, xt = A.centred(e), A.centred(x)
    ee, xx = float(np.dot(et, et)), float(np.dot(xt, xt))
    rel = lambda v, vt, en: (n + 4) * U + 2.0 * n * U * float(np.mean(np.abs(v.astype(np.float64)))) * float(np.sum(np.abs(vt))) / en
    rho = r[d + K] / math.sqrt(ee * xx)
    f_rho = F[d + K] / math.sqrt(ee * xx) + abs(rho) * (0.5 * (rel(e, et, ee) + rel(x, xt, xx)) + 3.0 * U)
    f_frac = 0.0
    if abs(d) < K:
        a, b, c = abs(r[d + K - 1]), abs(r[d + K]), abs(r[d + K + 1])
        Fa, Fb, Fc = F[d + K - 1], F[d + K], F[d + K + 1]
        den = a - 2.0 * b + c
        if den < 0.0:
            f_frac = 0.5 * ((Fa + Fc) / abs(den) + abs(a - c) * (Fa + 2.0 * Fb + Fc) / den ** 2) + 6.0 * U * abs(0.5 * (a - c) / den)
    return f_rho, f_frac


def test_lag_is_exact(lib):
    """lag and bits 0..2 of flags equal the restatement's for the true shifts 0, +-1, +-(K - 1), +-K (edge bit at +-K) of a noisy copy, an inverted copy
    and a low-passed pair, 3000 samples (two chunks), K = 24.  Asserted of the inputs first, in the restatement: the runner-up |r| lies below |r[d]|
    by at least 1000 times the asserted bound 4 F of test_r_vs_reference, so no rounding can decide a case.  rho and frac within 4 times their
    first-order bounds (``rho_frac_bounds``)."""
    K = K_EXACT
    es, xs, truth = shifted_pairs()
    lag, out, flags, r = xcorr_lag(lib, es, xs, K)
    for b, (e, x, (d, kind)) in enumerate(zip(es, xs, truth)):
        wd, wrho, wfrac, wflags, wr = A.lag(e, x, K)
        F = A.bound(e, x, K)
        a = np.abs(wr)
        runner_up = np.max(np.delete(a, wd + K))
        assert wd == d and a[wd + K] - runner_up >= 1000.0 * 4.0 * F.max(), (d, kind, a[wd + K], runner_up, F.max())
        assert wflags == 1 | (2 if abs(d) == K else 0) | (4 if kind == "inverted" else 0), (d, kind, wflags)
        assert lag[b] == wd and (flags[b] & 7) == wflags == flags[b], (d, kind, lag[b], flags[b])
        f_rho, f_frac = rho_frac_bounds(e, x, K, wd, wr, F)
        print(f"lag d {d:4d} {kind:>8}: rho got {out[b, 0]:.15f} want {wrho:.15f} diff {abs(out[b, 0] - wrho):.2e} bound {4 * f_rho:.2e}; "
              f"frac got {out[b, 1]:+.12f} want {wfrac:+.12f} diff {abs(out[b, 1] - wfrac):.2e} bound {4 * f_frac:.2e}")
        assert abs(out[b, 0] - wrho) <= 4.0 * f_rho and abs(out[b, 1] - wfrac) <= 4.0 * f_frac, (d, kind)
        assert np.all(np.abs(r[b] - wr) <= 4.0 * F)


# ---- 3. undefined rows, 4. row independence ---------------------------------------------------------------------------------------------------------
def test_undefined_rows_disturb_nothing(lib):
    """an all-zero estimate, a constant reference and a row of length 1: flag 0, lag 0, rho NaN, frac 0; the defined rows between them equal their
    single-row results bit for bit"""
    rs = np.random.RandomState(303)
    n, K = 700, 9
    x = [rs.standard_normal(n).astype(np.float32) for _ in range(3)]
    good = [(A.shift(v, s) + 0.1 * rs.standard_normal(n)).astype(np.float32) for v, s in zip(x, (4, -9, 0))]
    es = [good[0], np.zeros(n, np.float32), good[1], rs.standard_normal(n).astype(np.float32), np.ones(1, np.float32), good[2]]
    xs = [x[0], rs.standard_normal(n).astype(np.float32), x[1], np.full(n, 0.375, np.float32), np.full(1, 2.0, np.float32), x[2]]
    lag, out, flags, r = xcorr_lag(lib, es, xs, K)
    for b in (1, 3, 4):
        assert flags[b] == 0 and lag[b] == 0 and math.isnan(out[b, 0]) and out[b, 1] == 0.0, b
        assert A.lag(es[b], xs[b], K)[3] == 0
    assert lag[[0, 2, 5]].tolist() == [4, -9, 0] and flags[[0, 2, 5]].tolist() == [1, 3, 1]
    for b in (0, 2, 5):
        l1, o1, f1, r1 = xcorr_lag(lib, [es[b]], [xs[b]], K, ld=n)
        assert l1[0] == lag[b] and f1[0] == flags[b] and np.array_equal(bits(o1[0]), bits(out[b])) and np.array_equal(bits(r1[0]), bits(r[b])), b


def test_rows_do_not_depend_on_their_batch(lib):
    """every row of the ragged batch alone (its own length as the stride) equals the same row inside the batch bit for bit: lag, out and r_out"""
    T, Lt = lib.buddy_align_tile(), lib.buddy_align_lag_tile()
    K = Lt + 1
    es, xs = ragged_rows(T)
    lag, out, flags, r = xcorr_lag(lib, es, xs, K)
    for b in range(len(es)):
        l1, o1, f1, r1 = xcorr_lag(lib, [es[b]], [xs[b]], K, ld=len(es[b]))
        assert l1[0] == lag[b] and f1[0] == flags[b], b
        assert np.array_equal(bits(o1[0]), bits(out[b])) and np.array_equal(bits(r1[0]), bits(r[b])), b


def test_xcorr_lag_refuses_bad_arguments(lib):
    B, n, K = 2, 100, 5
    e, x = torch.zeros(B, n, device="cuda"), torch.zeros(B, n, device="cuda")
    lens, lag, flags = dev_i32([n, n]), guarded(B, torch.int32, -77), guarded(B, torch.int32, -77)
    out = guarded(2 * B, torch.float64, SENTINEL)
    nbytes = lib.buddy_xcorr_lag_workspace(B, n, K)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    st = _lib.stream_ptr()
    good = [_lib.ptr(e), _lib.ptr(x), lens.data_ptr(), B, n, K, lag.data_ptr(), out.data_ptr(), flags.data_ptr(), None, ws.data_ptr(), nbytes, st]
    assert lib.buddy_xcorr_lag(*good) == 0                                                 # r_out may be NULL
    for i in (0, 1, 2, 6, 7, 8, 10):                                                       # every other pointer
        args = list(good)
        args[i] = None
        assert lib.buddy_xcorr_lag(*args) == ERR_ARG and b"null" in lib.buddy_last_error(), i
    for i, v in ((3, 0), (3, 65536), (4, n - 1), (5, -1), (5, 65536), (11, nbytes - 8)):
        args = list(good)
        args[i] = v
        assert lib.buddy_xcorr_lag(*args) == ERR_ARG, (i, v)
    args = list(good)
    args[2] = dev_i32([n, 0]).data_ptr()
    assert lib.buddy_xcorr_lag(*args) == ERR_ARG
    torch.cuda.synchronize()
    assert split(lag, B, -77).tolist() == [0, 0] and split(flags, B, -77).tolist() == [0, 0] and np.isnan(split(out, 2 * B, SENTINEL)[0])


# ---- 5. the trimmed pair ---------------------------------------------------------------------------------------------------------------------------
def test_align_pair_equals_slicing(lib):
    """eo, xo equal numpy slicing exactly for the lags 0, +-1, +-(n - 1) and mixed signs in one ragged batch; zeros to the end of every row; guard words
    before and behind both outputs untouched; |d| >= n and every null pointer are refused"""
    rs = np.random.RandomState(404)
    lens = [300, 300, 300, 257, 257, 1, 64, 511]
    lags = [0, 1, -1, 256, -256, 0, -37, 129]
    es, xs = [rs.standard_normal(n).astype(np.float32) for n in lens], [rs.standard_normal(n).astype(np.float32) for n in lens]
    B, ld, ldo = len(lens), 520, 390
    e_d, x_d, lens_d, lag_d = padded(es, ld), padded(xs, ld), dev_i32(lens), dev_i32(lags)
    eo, xo = guarded(B * ldo + GUARD, torch.float32, SENTINEL), guarded(B * ldo + GUARD, torch.float32, SENTINEL)      # GUARD words in front as well
    lens_o = guarded(B, torch.int32, -77)
    st = _lib.stream_ptr()
    good = [_lib.ptr(e_d), _lib.ptr(x_d), lens_d.data_ptr(), lag_d.data_ptr(), B, ld, eo.data_ptr() + 4 * GUARD, xo.data_ptr() + 4 * GUARD, ldo,
            lens_o.data_ptr(), st]
    assert lib.buddy_align_pair(*good) == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    assert split(lens_o, B, -77).tolist() == [n - abs(d) for n, d in zip(lens, lags)]
    for buf, rows, sign in ((eo, es, 1), (xo, xs, -1)):
        a = buf.cpu().numpy()
        assert np.all(a[:GUARD] == SENTINEL) and np.all(a[GUARD + B * ldo:] == SENTINEL), "guard words overwritten"
        got = a[GUARD:GUARD + B * ldo].reshape(B, ldo)
        for b, (n, d) in enumerate(zip(lens, lags)):
            want = A.trim(es[b], xs[b], d)[0 if sign == 1 else 1]
            assert len(want) == n - abs(d) and np.array_equal(got[b, :len(want)], want) and np.all(got[b, len(want):] == 0.0), (b, d)
    for i in (0, 1, 2, 3, 6, 7, 9):
        args = list(good)
        args[i] = None
        assert lib.buddy_align_pair(*args) == ERR_ARG and b"null" in lib.buddy_last_error(), i
    for bad in ([300] + lags[1:], [-300] + lags[1:], lags[:5] + [1] + lags[6:], lags[:5] + [-1] + lags[6:]):                # |d| >= n
        args = list(good)
        keep = dev_i32(bad)
        args[3] = keep.data_ptr()
        assert lib.buddy_align_pair(*args) == ERR_ARG, bad
    for i, v in ((4, 0), (5, 510), (8, 381)):                                              # B, a stride below the longest row, ldo below the longest overlap
        args = list(good)
        args[i] = v
        assert lib.buddy_align_pair(*args) == ERR_ARG, (i, v)


# ---- 6. the effect on evaluate ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_aligned_equals_hand_trimmed(lib, monkeypatch):
    """evaluate(shifted estimate, clean, align=50) equals evaluate of the hand-trimmed pair, given in the same (B, L) layout with lens, bit for bit in
    all four values; align=None equals the call without the keyword bit for bit and never reaches buddy_xcorr_lag (a counting wrapper on the
    library's function); a 3-sample shift of a noisy copy of white noise costs more than 10 dB SI-SDR as it is and less than 0.01 dB aligned"""
    fs, L, shifts = 16000, 16000, (3, -5, 0)                                            # the delays the estimates are cut with
    rs = np.random.RandomState(505)
    xs = [synth_clean(60 + b, L + 64)[32:32 + L] for b in range(3)]
    es = [(synth_clean(60 + b, L + 64)[32 - d:32 - d + L] + 0.3 * np.std(xs[b]) * rs.standard_normal(L)).astype(np.float32) for b, d in enumerate(shifts)]
    e_d, x_d = torch.from_numpy(np.stack(es)).cuda(), torch.from_numpy(np.stack(xs)).cuda()
    calls = []
    real = lib.buddy_xcorr_lag
    monkeypatch.setattr(lib, "buddy_xcorr_lag", lambda *a: (calls.append(1), real(*a))[1])
    plain, none = M.evaluate(e_d, x_d, fs), M.evaluate(e_d, x_d, fs, align=None)
    assert not calls and none.alignment is None and plain.alignment is None
    assert np.array_equal(bits(plain.values.numpy()), bits(none.values.numpy())) and torch.equal(plain.flags, none.flags)
    assert torch.equal(plain.samples, none.samples) and torch.equal(plain.kept_frames, none.kept_frames)
    got = M.evaluate(e_d, x_d, fs, align=50)
    assert len(calls) == 1
    al = got.alignment
    want = [A.lag(e, x, 800) for e, x in zip(es, xs)]
    lags = [w[0] for w in want]
    assert lags == list(shifts)                                # of the inputs: the restatement finds the delays they were cut with
    assert al.max_lag == 800 and al.lag.tolist() == lags and al.flags.tolist() == [w[3] for w in want] and got.samples.tolist() == [L - abs(d) for d in lags]
    assert torch.equal(al.lens, got.samples) and al.est.shape == al.ref.shape == (3, L)
    he, hx = np.zeros((3, L), np.float32), np.zeros((3, L), np.float32)
    for b, d in enumerate(lags):
        te, tx = A.trim(es[b], xs[b], d)
        he[b, :len(te)], hx[b, :len(tx)] = te, tx
    assert np.array_equal(al.est.cpu().numpy(), he) and np.array_equal(al.ref.cpu().numpy(), hx)
    hand = M.evaluate(torch.from_numpy(he).cuda(), torch.from_numpy(hx).cuda(), fs, lens=[L - abs(d) for d in lags])
    assert np.array_equal(bits(got.values.numpy()), bits(hand.values.numpy())) and torch.equal(got.flags, hand.flags) and got.flags.tolist() == [15] * 3
    assert torch.equal(got.kept_frames, hand.kept_frames) and torch.equal(got.frames, hand.frames)
    for b, w in enumerate(want):
        assert abs(float(al.rho[b]) - w[1]) < 1e-9 and abs(float(al.frac[b]) - w[2]) < 1e-6, b
    # the illustration, on white noise
    src = rs.standard_normal(L + 8)
    x = src[4:4 + L].astype(np.float32)
    noise = 0.1 * rs.standard_normal(L + 8)
    e0, e3 = (src + noise)[4:4 + L].astype(np.float32), (src + noise)[1:1 + L].astype(np.float32)                             # e3[m + 3] = e0[m]
    pair = lambda e: (torch.from_numpy(e)[None].cuda(), torch.from_numpy(x)[None].cuda())
    s0 = float(M.evaluate(*pair(e0), fs, values=("si_sdr",)).values[0, 0])
    s3 = float(M.evaluate(*pair(e3), fs, values=("si_sdr",)).values[0, 0])
    a3 = M.evaluate(*pair(e3), fs, values=("si_sdr",), align=50)
    print(f"SI-SDR of a noisy copy: {s0:.4f} dB; delayed by 3 samples: {s3:.4f} dB; delayed and aligned: {float(a3.values[0, 0]):.4f} dB (lag {int(a3.alignment.lag[0])})")
    assert s0 - s3 > 10.0 and int(a3.alignment.lag[0]) == 3 and abs(float(a3.values[0, 0]) - s0) < 0.01


# ---- 7. the tester and the tool ----------------------------------------------------------------------------------------------------------------
SMALL = ["tester.sampling_params.T=3", "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "network.nf=32", "tester.noise.generator=philox",
         "tester.sub_batches=1", "+gpu=0", "tester.overriden_name=run", "+allow_random_init=true"]
EXTRA = ["lag_in", "lag_out", "lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out", "align_flags_in", "align_flags_out"]


def _run_tester(tmp, tag, extra):
    import test as cli
    data = os.path.join(tmp, "data")
    if not os.path.exists(data):
        for u, n_rir in enumerate((3000, 2400)):
            for sub, x in (("clean", synth_clean(u, 16000)), ("rir", np.concatenate([np.zeros(37, np.float32), synth_rir(u, n_rir)]))):
                d = os.path.join(data, sub, "p001")
                os.makedirs(d, exist_ok=True)
                wavfile.write(os.path.join(d, f"p001_{u:03d}.wav"), 16000, x.astype(np.float32))
    out = os.path.join(tmp, tag)
    torch.manual_seed(0)                                      # +allow_random_init draws the network from torch's generator: the same weights in every run
    t = cli.main(["--config-name=conf_VCTK.yaml", "tester=informed_dereverberation_DPS", *SMALL, f"model_dir={out}", f"dset.test.path={data}",
                  "dset.test.num_examples=2", "+batch_size=2", *extra])
    return t, os.path.join(out, "run", "informed_dereverberation", "VCTK_16k_4s_time")


def _files(base):
    return {os.path.relpath(os.path.join(dp, f), base): open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(base) for f in fs
            if f.endswith((".csv", ".wav"))}


def _same(a, b):
    return (isinstance(a, float) and math.isnan(a) and math.isnan(b)) or a == b


def test_tester_and_tool_write_the_alignment_columns(tmp_path):
    """informed mode, two utterances of one second: with metrics.align.use the run writes the same two files, metrics.csv with the eight further
    columns behind the usual ones and |lag| <= K = 800, values equal to evaluate(..., align=50) on the written wavs; with align.use=false the csv and wav
    files equal, byte for byte, those of a run whose metrics block has no align key; tools/evaluate.py --align on the written folder gives the
    tester's rows"""
    tmp = str(tmp_path)
    t_on, on = _run_tester(tmp, "on", ["tester.metrics.use=true", "tester.metrics.align.use=true"])
    assert sorted(f for f in os.listdir(on) if f.endswith(".csv")) == ["metrics.csv", "metrics_summary.csv"]
    rows = R.read_csv(os.path.join(on, "metrics.csv"))
    plain_cols = ["file", "samples"] + [f"{m}_{k}" for m in M.VALUES for k in ("in", "out", "delta")] + ["flags_in", "flags_out", "kept_frames", "frames"]
    assert list(rows[0]) == plain_cols + EXTRA == list(t_on.metrics_report[0]) and len(rows) == 2
    names = [r["file"] for r in rows]
    rd = {s: torch.from_numpy(np.stack([wavfile.read(os.path.join(on, s, n + ".wav"))[1] for n in names])).cuda() for s in ("original", "degraded", "reconstructed")}
    inp, out = M.evaluate(rd["degraded"], rd["original"], 16000, align=50), M.evaluate(rd["reconstructed"], rd["original"], 16000, align=50)
    for b, r in enumerate(rows):
        assert abs(r["lag_in"]) <= 800 and abs(r["lag_out"]) <= 800 and r["samples"] == 16000 - abs(r["lag_out"])
        assert r["lag_in"] == int(inp.alignment.lag[b]) and r["lag_out"] == int(out.alignment.lag[b]) and r["lag_ms_out"] == 1000.0 * r["lag_out"] / 16000.0
        assert _same(r["xcorr_in"], float(inp.alignment.rho[b])) and _same(r["xcorr_out"], float(out.alignment.rho[b]))
        assert r["align_flags_in"] == int(inp.alignment.flags[b]) and r["align_flags_out"] == int(out.alignment.flags[b]) and int(r["align_flags_in"]) & 1
        for q, m in enumerate(M.VALUES):
            assert _same(r[m + "_in"], float(inp.values[b, q])) and _same(r[m + "_out"], float(out.values[b, q])), (b, m)
    summ = [s["value"] for s in R.read_csv(os.path.join(on, "metrics_summary.csv"))]
    assert summ == [f"{m}_{k}" for m in M.VALUES for k in ("in", "out", "delta")] + ["lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out"]
    _, off = _run_tester(tmp, "off", ["tester.metrics.use=true", "tester.metrics.align.use=false"])
    _, bare = _run_tester(tmp, "bare", ["tester.metrics={use: true, values: [si_sdr, stoi, estoi, lsd]}"])
    f_off, f_bare, f_on = _files(off), _files(bare), _files(on)
    assert sorted(f_off) == sorted(f_bare) == sorted(f_on) and "metrics.csv" in f_off and f_off == f_bare
    assert open(os.path.join(off, "metrics.csv")).readline().strip().split(",") == plain_cols
    assert all(f_on[f] == f_off[f] for f in f_on if f.endswith(".wav"))                    # the wavs do not depend on the report
    saved = open(os.path.join(on, "metrics.csv")).read()
    os.remove(os.path.join(on, "metrics.csv"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), on, "--align"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "lag_ms_out" in p.stdout
    again = open(os.path.join(on, "metrics.csv")).read()     # the same header and lines, the files in name order
    assert again.splitlines()[0] == saved.splitlines()[0] and sorted(again.splitlines()[1:]) == sorted(saved.splitlines()[1:])
