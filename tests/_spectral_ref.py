"""float64 numpy restatement of the spectral distortion measures of DESIGN.md section 21, written from the definitions: the oracle of
tests/test_spectral_host.py and tests/test_hip_spectral.py.  Per pair (estimate e, clean reference x) at 16 kHz, frames of 400 samples at hop 160 under
w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 401), all FULL frames, 512-point transform, bins 0..256:

  CD        real cepstra c[0..24] of 0.5 ln(|X|^2 + d) (the estimate scaled by g), each coefficient's mean over the frames removed per signal,
            (10 / ln 10) sqrt(dc0^2 + 2 sum dcn^2) clipped to [0, 10], mean over the frames
  LLR       order 12, autocorrelation of the windowed frames, r[0] *= 1 + 1e-9, Levinson-Durbin, ln(a_e R_x a_e / a_x R_x a_x) clipped to [0, 2], mean over
            the frames whose two r[0] are positive
  fwSegSNR  23 triangular mel bands of the magnitude spectra, band SNR decided by comparison (35, -10, or 10 log10), weights X_j^0.2, mean over the
            frames with a positive weight sum

g = sqrt(||x||^2 / ||e||^2) (zero-mean moments; 1 when ||e||^2 = 0), d = 1e-8 (||x||^2 / L) sum w^2.

``dtype=np.float32`` rounds the resampler output, the windowed frames and the transform (scipy.fft on float32 input, the magnitude rounded once) to single
precision -- the stages the device runs in fp32; everything else stays float64.  The difference between the two runs is the ``D32`` of the whole-call test."""
import csv
import math

import numpy as np
import scipy.fft
from scipy import signal

import _metrics_ref as MR
from buddy_amd.utils import resample as RS

FS, FRAME, HOP, NFFT, NBIN, NCEP, ORDER, NBANDS = 16000, 400, 160, 512, 257, 25, 12, 23
WINDOW = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(FRAME, dtype=np.float64) + 1.0) / 401.0)
W2 = float(np.sum(WINDOW * WINDOW))


def frames_of(n):
    return (n - FRAME) // HOP + 1 if n >= FRAME else 0


def mel_bands():
    """(23, 257) float64: triangles of height 1 between 25 points equally spaced in mel from 0 to 8000 Hz, over the bin frequencies k 16000 / 512"""
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    pts = [700.0 * (10.0 ** (m / 2595.0) - 1.0) for m in np.linspace(0.0, mel(8000.0), NBANDS + 2)]
    f = np.arange(NBIN, dtype=np.float64) * (FS / NFFT)
    M = np.zeros((NBANDS, NBIN))
    for j in range(NBANDS):
        lo, c, hi = pts[j], pts[j + 1], pts[j + 2]
        M[j] = np.maximum(0.0, np.minimum((f - lo) / (c - lo), (hi - f) / (hi - c)))
    return M


def to_16k(x, fs, dtype=np.float64):
    """the project's resampler in float64 with the fp32 taps the device holds; ``dtype`` rounds the result"""
    x = np.asarray(x, np.float64)
    if fs == FS:
        return x
    up, down = RS.ratio(fs, FS)
    h = RS.design_filter(up, down).astype(np.float32).astype(np.float64)
    y = signal.resample_poly(x, up, down, window=h / up, padtype="constant")
    assert len(y) == RS.out_length(len(x), up, down)
    return y.astype(dtype).astype(np.float64)


def framed(x, dtype=np.float64):
    """(F, 400) windowed full frames; window and product rounded to ``dtype``"""
    F = frames_of(len(x))
    if F == 0:
        return np.zeros((0, FRAME))
    idx = np.arange(F)[:, None] * HOP + np.arange(FRAME)[None, :]
    w = WINDOW.astype(dtype).astype(np.float64)
    return (w[None, :] * np.asarray(x, np.float64)[idx]).astype(dtype).astype(np.float64)


def spectra(x, dtype=np.float64):
    """(F, 257) float64 magnitudes of the 512-point transform of every windowed full frame (scipy.fft in ``dtype``, the magnitude rounded to it)"""
    fr = framed(x, dtype).astype(dtype)
    if not len(fr):
        return np.zeros((0, NBIN))
    X = scipy.fft.rfft(fr, NFFT, axis=1).astype(np.complex128)
    return np.sqrt(X.real * X.real + X.imag * X.imag).astype(dtype).astype(np.float64)


def gain_floor(e, x):
    """(g, d) of one pair at 16 kHz"""
    ee, xx, _, _, _ = MR.moments(e, x)
    return (math.sqrt(xx / ee) if ee > 0.0 else 1.0), 1e-8 * (xx / len(x)) * W2


def cepstra(S, d):
    """(F, 25): c[n] = (1/512) sum_{k = 0..511} 0.5 ln(S[k]^2 + d) cos(2 pi k n / 512), the bins above 256 by even symmetry"""
    L = 0.5 * np.log(S * S + d)
    full = np.concatenate([L, L[:, NBIN - 2:0:-1]], axis=1)
    k, n = np.arange(NFFT)[:, None], np.arange(NCEP)[None, :]
    return full @ np.cos(2.0 * np.pi * ((k * n) % NFFT) / NFFT) / NFFT


def cd(X, E, g, d):
    """(CD dB, flag) from magnitude spectra (F, 257) of the clean and the estimated signal"""
    if len(X) < 1 or not d > 0.0:
        return float("nan"), 0
    cx, ce = cepstra(X, d), cepstra(g * E, d)
    dc = (cx - cx.mean(axis=0, keepdims=True)) - (ce - ce.mean(axis=0, keepdims=True))
    v = (10.0 / math.log(10.0)) * np.sqrt(dc[:, 0] ** 2 + 2.0 * np.sum(dc[:, 1:] ** 2, axis=1))
    return float(np.mean(np.clip(v, 0.0, 10.0))), 1


def fwsegsnr(X, E, g, M=None):
    """(fwSegSNR dB, flag, counted frames) from magnitude spectra (F, 257)"""
    M = mel_bands() if M is None else M
    if len(X) < 1:
        return float("nan"), 0, 0
    Xb, Eb = X @ M.T, (g * E) @ M.T
    num, den = Xb * Xb, (Xb - Eb) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = np.where(den <= num * 10.0 ** -3.5, 35.0, np.where(num <= den * 0.1, -10.0, 10.0 * np.log10(num / den)))
    W = Xb ** 0.2
    sw = W.sum(axis=1)
    ok = sw > 0.0
    if not ok.any():
        return float("nan"), 0, 0
    return float(np.mean((W * snr).sum(axis=1)[ok] / sw[ok])), 1, int(ok.sum())


def autocorr(s, p=ORDER):
    return np.array([float(np.sum(s[:len(s) - k] * s[k:])) for k in range(p + 1)])


def levinson(r, p=ORDER):
    """(a with a[0] = 1, prediction error) of the autocorrelation r[0..p]; stops where the error is no longer positive"""
    a = np.zeros(p + 1)
    a[0] = 1.0
    err = float(r[0])
    for i in range(1, p + 1):
        if not err > 0.0:
            break
        k = -(r[i] + float(np.sum(a[1:i] * r[i - 1:0:-1]))) / err
        a[1:i] = a[1:i] + k * a[i - 1:0:-1]
        a[i] = k
        err *= 1.0 - k * k
    return a, err


def llr(e, x):
    """(LLR, flag, counted frames, the smallest normalised prediction error E_p / r[0] of either signal over the counted frames)"""
    fx, fe = framed(x), framed(e)
    vals, worst = [], float("inf")
    for sx, se in zip(fx, fe):
        rx, re = autocorr(sx), autocorr(se)
        if not (rx[0] > 0.0 and re[0] > 0.0):
            continue
        rx[0] *= 1.0 + 1e-9
        re[0] *= 1.0 + 1e-9
        ax, ex = levinson(rx)
        ae, ee = levinson(re)
        i = np.arange(ORDER + 1)
        R = rx[np.abs(i[:, None] - i[None, :])]
        vals.append(min(max(math.log((ae @ R @ ae) / (ax @ R @ ax)), 0.0), 2.0))
        worst = min(worst, ex / rx[0], ee / re[0])
    if not vals:
        return float("nan"), 0, 0, worst
    return float(np.mean(vals)), 1, len(vals), worst


def evaluate(e, x, fs, dtype=np.float64):
    """((CD, LLR, fwSegSNR), flags, frames, LLR frames, fwSegSNR frames) of one pair at rate ``fs``, as utils.spectral.evaluate reports it"""
    e16, x16 = to_16k(e, fs, dtype), to_16k(x, fs, dtype)
    g, d = gain_floor(e16, x16)
    X, E = spectra(x16, dtype), spectra(e16, dtype)
    c, f0 = cd(X, E, g, d)
    l, f1, nl, _ = llr(e16, x16)
    s, f2, ns = fwsegsnr(X, E, g)
    return np.array([c, l, s]), f0 | f1 << 1 | f2 << 2, len(X), nl, ns


# ---- the test signals ----------------------------------------------------------------------------------------------------------------------
GAP = (3000, 4000)                                   # exact zeros in both signals: frames 19..22 (160 f >= 3000, 160 f + 400 <= 4000) are all zero
LENS = (12000, 7777, 400 + 159)


def ar_noise(seed, n, fs=FS):
    """second-order AR noise (poles of radius sqrt(0.8)) under a 3 Hz amplitude modulation, float32; the samples of GAP (scaled to ``fs``) are zero"""
    rs = np.random.RandomState(seed)
    x = signal.lfilter([1.0], [1.0, -1.6, 0.8], rs.standard_normal(n + 200))[200:]
    x = 0.05 * x * (1.0 + 0.5 * np.sin(2.0 * np.pi * 3.0 * np.arange(n) / fs))
    k = fs // FS
    x[GAP[0] * k:GAP[1] * k] = 0.0
    return x.astype(np.float32)


def pairs(fs=FS):
    """(estimates, clean signals) of the three cases: convolved with a decaying-noise tail, with added noise, identical; lengths LENS scaled to ``fs``"""
    k = fs // FS
    xs = [ar_noise(10 + b, n * k, fs) for b, n in enumerate(LENS)]
    rs = np.random.RandomState(99)
    t = np.arange(1200 * k)
    h = np.concatenate([[1.0], 0.25 * rs.standard_normal(len(t)) * np.exp(-t / (300.0 * k)) / math.sqrt(k)])
    e0 = signal.fftconvolve(xs[0].astype(np.float64), h)[:len(xs[0])]
    e1 = xs[1].astype(np.float64) + 0.02 * rs.standard_normal(len(xs[1]))
    es = [e0, e1, xs[2].astype(np.float64)]
    for e in es[:2]:
        e[GAP[0] * k:GAP[1] * k] = 0.0
    return [e.astype(np.float32) for e in es], xs


def read_csv(path):
    """the rows of a report as dicts: empty fields -> NaN; ``file`` / ``value`` stay text; flags, lags, counts and ``n`` -> int; the rest float"""
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            row = {}
            for k, v in r.items():
                if k in ("file", "value"):
                    row[k] = v
                elif k.startswith(("flags", "align_flags", "frames", "llr_frames", "fwsegsnr_frames")) or k in ("samples", "n", "lag_in", "lag_out"):
                    row[k] = float("nan") if v == "" else int(v)
                else:
                    row[k] = float("nan") if v == "" else float(v)
            out.append(row)
    return out
