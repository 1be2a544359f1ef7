"""GPU: the noise tracker and post-filter (csrc/denoise.hip, buddy_amd/utils/denoise.py) against the float64 restatement
tests/_denoise_ref.py: the spectra, the gains on the GPU's own spectra, the synthesis on random gains, the whole call, and reproducibility.

Rows: the eight edge lengths 1, 127, 128, 129, 511, 512, 513, 700 (4, 4, 4, 5, 7, 7, 8, 9 frames: below, at and above one hop and one frame, frame
counts that are no multiple of the four frames of a workgroup), 12 000 samples of bursts plus noise at 10 dB, 12 000 samples of weak noise with a
unit 1 kHz tone from sample 3000 on, 2000 zeros followed by 4000 samples of noise, and 1000 zeros.  Each row runs alone; the tone row, the
silence-led row and the row of 513 samples also run as one ragged batch with NaN behind every row."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _denoise_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import denoise as D  # noqa: E402

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
GUARD = 64
SENTINEL = 12345.0
FFT_C = 45 * U24 * math.sqrt(512.0)                  # the transform's constant of DESIGN.md sections 17 and 21
RULES = ("wiener", "lsa")


@functools.lru_cache(maxsize=None)
def rows():
    """name -> float32 row, read-only; made once"""
    out = {f"edge{L}": R.white(L, 0.1, 100 + L) for L in R.EDGE_LENGTHS}
    out["bursts"] = R.noisy_bursts(10.0, L=12000, seed=2, start=0.1)[0]
    out["tone"] = R.tone_row()
    out["silence"] = R.silence_led()
    out["zero"] = np.zeros(1000, np.float32)
    for v in out.values():
        v.setflags(write=False)
    return out


BATCH = ("tone", "silence", "edge513")
NAMES = tuple(f"edge{L}" for L in R.EDGE_LENGTHS) + ("bursts", "tone", "silence", "zero")


def padded(rws, ld):
    out = np.full((len(rws), ld), np.nan, np.float32)
    for b, r in enumerate(rws):
        out[b, :len(r)] = r
    return torch.from_numpy(out).cuda()


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def raw_spectra(rws):
    """the C entry on NaN-padded rows with spare frames and guard words behind the output -> (B, ldt, 257, 2) float32 on the host"""
    lib = _lib.require_gpu()
    B, ln = len(rws), [len(r) for r in rws]
    ld, ldt = max(ln) + 5, max(R.frames(n) for n in ln) + 3
    x_d, lens_d = padded(rws, ld), dev_i32(ln)
    n = B * ldt * R.BINS * 2
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    rc = lib.buddy_denoise_spectra(_lib.ptr(x_d), lens_d.data_ptr(), B, ld, _lib.ptr(buf), ldt, _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert np.all(a[n:] == SENTINEL), "guard words overwritten"
    return a[:n].reshape(B, ldt, R.BINS, 2)


@functools.lru_cache(maxsize=None)
def gpu_spectra(name):
    """(T, 257, 2) float32: the GPU's spectra of a row run alone"""
    Y = D.spectra_hip(torch.from_numpy(rows()[name].copy())[None].cuda())[0].cpu().numpy()
    Y.setflags(write=False)
    return Y


def as_complex(Y):
    return Y[..., 0].astype(np.float64) + 1j * Y[..., 1].astype(np.float64)


# ---- 1. spectra ----------------------------------------------------------------------------------------------------------------------------------
def test_frame_counts():
    lib = _lib.load()
    assert tuple(D.frames(L) for L in R.EDGE_LENGTHS) == R.EDGE_FRAMES == tuple(lib.buddy_denoise_frames(L) for L in R.EDGE_LENGTHS)
    for name in NAMES:
        assert gpu_spectra(name).shape == (R.frames(len(rows()[name])), R.BINS, 2)


def test_spectra_vs_restatement():
    """per (frame, bin): |got - want| <= 45 * 2^-24 * sqrt(512) * ||w x_t||_2 (nine radix-2 stages at about 5u each in the 2-norm, Parseval).  Asserted
    on the CPU first: the restatement of the same row shifted by one sample misses that bound by more than 1e3 times it."""
    w = R.window()
    for name in ("bursts", "tone"):
        r = rows()[name]
        n = len(r) - 1
        tol = FFT_C * np.linalg.norm(w * R.frame_matrix(r[:n]), axis=1)
        miss = np.abs(R.spectra(r[1:]) - R.spectra(r[:n])) / tol[:, None]
        assert miss.max() > 1e3, miss.max()
    worst = 0.0

    def check(got, r, who):
        nonlocal worst
        T = R.frames(len(r))
        assert np.all(got[T:] == SENTINEL), who                                           # nothing written behind the row's frames
        tol = FFT_C * np.linalg.norm(w * R.frame_matrix(r), axis=1)
        err = np.abs(as_complex(got[:T]) - R.spectra(r))
        assert np.all(err <= tol[:, None]), (who, float((err[tol > 0] / tol[tol > 0, None]).max()))
        if (tol > 0).any():
            worst = max(worst, float((err[tol > 0] / tol[tol > 0, None]).max()))
        assert not got[:T][tol == 0].any(), who                                           # an all-zero frame has an all-zero spectrum, exactly

    for name in NAMES:
        check(raw_spectra([rows()[name]])[0], rows()[name], name)
    got = raw_spectra([rows()[k] for k in BATCH])
    for b, name in enumerate(BATCH):
        check(got[b], rows()[name], "batch " + name)
        T = R.frames(len(rows()[name]))
        assert np.array_equal(got[b, :T].view(np.uint32), gpu_spectra(name).view(np.uint32)), name      # a row's bits do not depend on its batch
    print(f"spectra: worst error / bound {worst:.4f}")


# ---- 2. gains on the GPU's own spectra -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tracked(name, rule):
    """the restatement on the GPU's spectra of a row, in float64 and in longdouble -> (G64, S64, dG, dS relative, what the run reached)"""
    Y = gpu_spectra(name)
    pw = (Y[..., 0].astype(np.float64) ** 2 + Y[..., 1].astype(np.float64) ** 2)[None]
    r = rows()[name]
    phi = R.row_floor(r)
    G, S, seen = R.track(pw, [phi], len(r), rule)
    Gl, Sl, _ = R.track(pw, [phi], len(r), rule, dtype=np.longdouble)
    dG = float(np.abs(G - Gl).max())
    dS = float((np.abs(S - Sl) / Sl).max())
    return G[0], S[0], dG, dS, seen


def test_reference_reaches_every_branch():
    assert tracked("tone", "lsa")[4]["capped"] > 0                                       # Pbar > 0.99: the capped probability
    seen = tracked("bursts", "lsa")[4]
    assert seen["ag_min"] < 0.1 and seen["ag_max"] > 10.0                                # both branches of E1
    assert tracked("silence", "lsa")[4]["floored"] > 0                                   # the row floor phi engages
    print({k: tracked(k, "lsa")[4] for k in ("tone", "bursts", "silence")})


@pytest.mark.parametrize("rule", RULES)
def test_gains_vs_restatement(rule):
    """|gpu - ref| <= 2^-24 |ref| + 100 d, d the largest float64 / longdouble difference of the restatement on that input (absolute for G, relative
    for sigma^2): the recursion's own round-off sensitivity, times 100 for a device exp and E1 a few ulp off numpy's, plus the one fp32 rounding of
    the stored value"""
    lines = []
    for name in NAMES[:-1]:
        r = rows()[name]
        Y = torch.from_numpy(gpu_spectra(name).copy())[None].cuda()
        G, S = D.gains_hip(Y, [len(r)], [R.row_floor(r)], rule)
        G, S = G[0].cpu().numpy().astype(np.float64), S[0].cpu().numpy().astype(np.float64)
        Gr, Sr, dG, dS, _ = tracked(name, rule)
        eG = np.abs(G - Gr) / (U24 * np.abs(Gr) + 100.0 * dG)
        eS = np.abs(S - Sr) / (U24 * np.abs(Sr) + 100.0 * dS * np.abs(Sr))
        lines.append(f"{rule:6s} {name:8s} d_G {dG:.2e} d_sigma2 {dS:.2e}  error / bound: G {eG.max():.3f} sigma2 {eS.max():.3f}")
        print(lines[-1])
        assert np.isfinite(G).all() and np.isfinite(S).all(), name
        assert eG.max() <= 1.0 and eS.max() <= 1.0, lines[-1]


@pytest.mark.parametrize("rule", RULES)
def test_scaled_row_gives_bit_equal_gains(rule):
    for name in ("bursts", "silence", "edge129"):
        x = torch.from_numpy(rows()[name].copy())[None].cuda()
        a, b = D.denoise(x, gain=rule, keep_gains=True), D.denoise(x * 4096.0, gain=rule, keep_gains=True)
        assert torch.equal(a.G.view(torch.int32), b.G.view(torch.int32)), name
        assert torch.equal((a.out * 4096.0).view(torch.int32), b.out.view(torch.int32)), name


# ---- 3. synthesis --------------------------------------------------------------------------------------------------------------------------------
def synthesis_bound(Z, L, ref):
    """per output sample: the inverse transform's 45 * 2^-24 * sqrt(512) * ||Z_t||_2 / 512 per frame sample (the norm over the full Hermitian spectrum;
    the constant's margin takes the one fp32 rounding of each product G Y), carried through sum_t w e_t / sum_t w^2, plus the fp32 rounding of the
    result"""
    T = R.frames(L)
    full = np.sqrt(np.abs(Z[:, 0]) ** 2 + np.abs(Z[:, 256]) ** 2 + 2.0 * np.sum(np.abs(Z[:, 1:256]) ** 2, axis=1))
    e = FFT_C * full / 512.0
    w = R.window()
    num, den = np.zeros(R.P + (T - 1) * R.H + R.N), np.zeros(R.P + (T - 1) * R.H + R.N)
    for t in range(T):
        num[t * R.H:t * R.H + R.N] += w * e[t]
        den[t * R.H:t * R.H + R.N] += w * w
    return num[R.P:R.P + L] / den[R.P:R.P + L] + U24 * np.abs(ref)


def test_synthesis_vs_restatement():
    worst = 0.0
    for name in NAMES[:-1]:
        r = rows()[name]
        L, T = len(r), R.frames(len(r))
        Yg = gpu_spectra(name)
        g = np.random.RandomState(len(r)).uniform(0.0, 1.0, (T, R.BINS)).astype(np.float32)
        got = D.synthesis_hip(torch.from_numpy(Yg.copy())[None].cuda(), torch.from_numpy(g)[None].cuda(), [L])[0].cpu().numpy().astype(np.float64)
        Z = g.astype(np.float64) * as_complex(Yg)
        ref = R.synthesis(as_complex(Yg), g.astype(np.float64), L)
        tol = synthesis_bound(Z, L, ref)
        err = np.abs(got - ref)
        assert np.all(err <= tol), (name, float((err[tol > 0] / tol[tol > 0]).max()))
        assert not got[tol == 0].any(), name
        if (tol > 0).any():
            worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()))
    print(f"synthesis: worst error / bound {worst:.4f}")


def test_unit_gains_return_the_input():
    worst = 0.0
    for L in R.EDGE_LENGTHS:
        r = rows()[f"edge{L}"]
        Yg = gpu_spectra(f"edge{L}")
        one = torch.ones(1, Yg.shape[0], R.BINS, dtype=torch.float32, device="cuda")
        got = D.synthesis_hip(torch.from_numpy(Yg.copy())[None].cuda(), one, [L])[0].cpu().numpy().astype(np.float64)
        tol = synthesis_bound(as_complex(Yg), L, r.astype(np.float64))
        err = np.abs(got - r.astype(np.float64))
        assert np.all(err <= tol), (L, float((err / tol).max()))
        worst = max(worst, float((err / tol).max()))
    print(f"unit gains: worst error / bound {worst:.4f}")


# ---- 4. the whole call ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def whole(name, rule, fp32):
    return R.denoise(rows()[name], rule, -15.0, fp32)


def check_whole(res, b, name, rule):
    """row b of a ``Denoised`` against the restatement: the output within max(32 D32, 2^-20) max|ref|, D32 the difference of the restatement's
    fp32-rounded and float64 runs relative to max|ref|; each statistic within max(32 |its own fp32 / float64
    difference|, 2^-20 |ref|); flags and frames exact"""
    r = rows()[name]
    L = len(r)
    ref, ref32 = whole(name, rule, False), whole(name, rule, True)
    got = res.out[b].cpu().numpy().astype(np.float64)
    assert not got[L:].any(), name
    assert int(res.flags[b]) == ref["flags"] and int(res.frames[b]) == ref["frames"] and int(res.samples[b]) == L, name
    top = float(np.abs(ref["out"]).max())
    if top == 0.0:
        assert not got.any() and all(math.isnan(float(v[b])) for v in (res.snr_est_db, res.noise_db, res.att_db)), name
        return 0.0
    d32 = float(np.abs(ref32["out"] - ref["out"]).max()) / top
    ratio = float(np.abs(got[:L] - ref["out"]).max()) / (max(32.0 * d32, 2.0 ** -20) * top)
    assert ratio <= 1.0, (name, rule, ratio, d32)
    for key in ("snr_est_db", "noise_db", "att_db"):
        want, v = ref[key], float(getattr(res, key)[b])
        if math.isinf(want):
            assert v == want, (name, key)
            continue
        tol = max(32.0 * abs(ref32[key] - want), 2.0 ** -20 * abs(want))
        print(f"{rule:6s} {name:8s} {key:10s} {v:12.6f} ref {want:12.6f} error / bound {abs(v - want) / tol:.3f}")
        assert abs(v - want) <= tol, (name, rule, key, v, want, tol)
    return ratio


@pytest.mark.parametrize("rule", RULES)
def test_denoise_vs_restatement(rule):
    for name in NAMES:
        x = torch.from_numpy(rows()[name].copy())[None].cuda()
        res = D.denoise(x, gain=rule, keep_gains=(name == "zero"))
        ratio = check_whole(res, 0, name, rule)
        print(f"{rule:6s} {name:8s} output error / bound {ratio:.3f}")
        if name == "zero":
            assert int(res.flags[0]) == D.ZERO and bool((res.G == 1.0).all()) and not bool(res.sigma2.any())
    assert D.flag_text(D.ZERO | D.SHORT) == "ZERO|SHORT"


# ---- 5. reproducibility --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_batch_and_rerun_are_bit_equal(rule):
    rws = [rows()[k] for k in BATCH]
    ln = [len(r) for r in rws]
    xb = padded(rws, max(ln) + 5)
    a = D.denoise(xb, lens=ln, gain=rule, keep_gains=True)
    b = D.denoise(xb, lens=ln, gain=rule, keep_gains=True)
    for key in ("out", "G", "sigma2"):
        assert torch.equal(getattr(a, key).view(torch.int32), getattr(b, key).view(torch.int32)), key
    for key in ("snr_est_db", "noise_db", "att_db"):
        assert np.array_equal(getattr(a, key).numpy().view(np.uint64), getattr(b, key).numpy().view(np.uint64)), key
    for i, name in enumerate(BATCH):
        check_whole(a, i, name, rule)
        one = D.denoise(torch.from_numpy(rws[i].copy())[None].cuda(), gain=rule, keep_gains=True)
        T = R.frames(ln[i])
        assert torch.equal(one.out[0].view(torch.int32), a.out[i, :ln[i]].view(torch.int32)), name
        assert torch.equal(one.G[0].view(torch.int32), a.G[i, :T].view(torch.int32)) and torch.equal(one.sigma2[0].view(torch.int32), a.sigma2[i, :T].view(torch.int32))
        for key in ("snr_est_db", "noise_db", "att_db"):
            assert getattr(one, key).numpy().view(np.uint64)[0] == getattr(a, key).numpy().view(np.uint64)[i], (name, key)


def test_refusals():
    x = torch.zeros(1, 1000)
    with pytest.raises(_lib.BuddyHipError):
        D.denoise(x)
    with pytest.raises(ValueError):
        D.denoise(x.cuda(), gain="mmse")
    with pytest.raises(ValueError):
        D.denoise(x.cuda(), floor_db=3.0)
    with pytest.raises(ValueError):
        D.denoise(x.cuda(), lens=[1001])
