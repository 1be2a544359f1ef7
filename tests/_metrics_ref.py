"""float64 numpy / scipy restatement of the evaluation metrics of DESIGN.md section 17, written from the definitions: the oracle of
tests/test_metrics_host.py and tests/test_hip_metrics.py.  Per pair (estimate e, clean reference x) of L samples at rate fs:

  SI-SDR   both means removed, a = <e,x> / max(||x||^2, 1e-30), 10 log10(||a x||^2 / max(||a x - e||^2, 1e-30))
  STOI / ESTOI (Taal et al. 2011; Jensen & Taal 2016) at 10 kHz: the project's polyphase resampler (scipy.signal.resample_poly with the taps the
           device holds); window w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257), 256 samples at hop 128, all FULL frames; frames of the clean signal with
           20 log10(||w x_f|| + eps) > max - 40 are kept and both signals rebuilt by overlap-add; 512-point transform, 15 third-octave bands from
           150 Hz; segments of 30 frames; eps = 2^-52
  LSD      the estimate scaled by sqrt(||x||^2 / ||e||^2) (zero-mean moments), same frames at the signals' own rate without frame removal, bins 0..256,
           floor 1e-8 mean P, mean over frames of the rms over bins of 10 log10((P + d) / (Q + d))

``dtype=np.float32`` rounds the resampler output, the windowed frames (the rebuilt signals with them) and the transform (scipy.fft on float32 input)
to single precision -- the stages the device runs in fp32; everything else stays float64.  The difference between the two runs is the ``d32`` of the
whole-call test."""
import csv
import math

import numpy as np
import scipy.fft
from scipy import signal

from buddy_amd.utils import resample as RS

FRAME, HOP, NFFT, SEG, J = 256, 128, 512, 30, 15
EPS = 2.0 ** -52
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138), (138, 174),
         (174, 219))
WINDOW = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(FRAME, dtype=np.float64) + 1.0) / 257.0)


def frames_of(n):
    return (n - FRAME) // HOP + 1 if n >= FRAME else 0


def moments(e, x):
    """(||e||^2, ||x||^2, <e,x>, SI-SDR dB, flag) with both means removed, float64; the formula and clamps of utils.metrics.si_sdr"""
    e, x = np.asarray(e, np.float64), np.asarray(x, np.float64)
    e, x = e - e.mean(), x - x.mean()
    ee, xx, ex = float(np.sum(e * e)), float(np.sum(x * x)), float(np.sum(e * x))
    a = ex / max(xx, 1e-30)
    t = a * x
    with np.errstate(divide="ignore"):
        s = 10.0 * np.log10(np.sum(t * t) / max(float(np.sum((t - e) ** 2)), 1e-30))
    return ee, xx, ex, float(s), int(xx > 0.0 and len(x) >= 2)


def to_10k(x, fs, dtype=np.float64):
    """the project's resampler in float64 with the fp32 taps the device holds; ``dtype`` rounds the result"""
    x = np.asarray(x, np.float64)
    if fs == 10000:
        return x.astype(dtype).astype(np.float64)
    up, down = RS.ratio(fs, 10000)
    h = RS.design_filter(up, down).astype(np.float32).astype(np.float64)
    y = signal.resample_poly(x, up, down, window=h / up, padtype="constant")
    assert len(y) == RS.out_length(len(x), up, down)
    return y.astype(dtype).astype(np.float64)


def framed(x, dtype=np.float64):
    """(F, 256) windowed full frames, each product rounded to ``dtype``"""
    F = frames_of(len(x))
    if F == 0:
        return np.zeros((0, FRAME))
    idx = np.arange(F)[:, None] * HOP + np.arange(FRAME)[None, :]
    w = WINDOW.astype(dtype).astype(np.float64)
    return (w[None, :] * np.asarray(x, np.float64)[idx]).astype(dtype).astype(np.float64)


def frame_energies_db(x):
    """E[f] of step (d), float64 throughout"""
    fr = framed(x)
    return 20.0 * np.log10(np.sqrt(np.sum(fr * fr, axis=1)) + EPS)


def kept_frames(x):
    E = frame_energies_db(x)
    return np.nonzero(E > E.max() - 40.0)[0] if len(E) else np.zeros(0, np.int64)


def threshold_margin_db(x):
    """smallest |E[f] - (max E - 40)| of a row: the select test requires 1e-3 dB"""
    E = frame_energies_db(x)
    return float(np.abs(E - (E.max() - 40.0)).min()) if len(E) else float("inf")


def rebuild(x, src, dtype=np.float64):
    """overlap-add of the kept windowed frames at hop 128, in order; (K - 1) 128 + 256 samples (0 for K = 0)"""
    K = len(src)
    if K == 0:
        return np.zeros(0)
    fr = framed(x, dtype)[src]
    out = np.zeros((K - 1) * HOP + FRAME)
    for j in range(K):
        out[j * HOP:j * HOP + FRAME] += fr[j]
    return out.astype(dtype).astype(np.float64)


def spectra(x, dtype=np.float64):
    """(257, M) complex: the 512-point transform of every windowed full frame (scipy.fft in ``dtype``)"""
    fr = framed(x, dtype).astype(dtype)
    return scipy.fft.rfft(fr, NFFT, axis=1).T.astype(np.complex128) if len(fr) else np.zeros((NFFT // 2 + 1, 0), np.complex128)


def band_spectra(x, dtype=np.float64, bands=BANDS):
    """(J, M) float64"""
    P = np.abs(spectra(x, dtype)) ** 2
    return np.stack([np.sqrt(P[lo:hi].sum(axis=0)) for lo, hi in bands])


def stoi_scores(X, Y):
    """(STOI, ESTOI, flag) from band spectra (J, M) of the clean and the estimated signal, float64"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    Jn, M = X.shape
    S = M - (SEG - 1)
    if S < 1:
        return float("nan"), float("nan"), 0
    d = de = 0.0
    for m in range(SEG, M + 1):
        xs, ys = X[:, m - SEG:m], Y[:, m - SEG:m]
        c = np.sqrt(np.sum(xs * xs, axis=1, keepdims=True)) / (np.sqrt(np.sum(ys * ys, axis=1, keepdims=True)) + EPS)
        yc = np.minimum(c * ys, xs * CLIP)
        xn = xs - xs.mean(axis=1, keepdims=True)
        xn = xn / (np.sqrt(np.sum(xn * xn, axis=1, keepdims=True)) + EPS)
        yn = yc - yc.mean(axis=1, keepdims=True)
        yn = yn / (np.sqrt(np.sum(yn * yn, axis=1, keepdims=True)) + EPS)
        d += float(np.sum(xn * yn))
        yr = ys - ys.mean(axis=1, keepdims=True)
        yr = yr / (np.sqrt(np.sum(yr * yr, axis=1, keepdims=True)) + EPS)
        xc = xn - xn.mean(axis=0, keepdims=True)
        xc = xc / (np.sqrt(np.sum(xc * xc, axis=0, keepdims=True)) + EPS)
        yq = yr - yr.mean(axis=0, keepdims=True)
        yq = yq / (np.sqrt(np.sum(yq * yq, axis=0, keepdims=True)) + EPS)
        de += float(np.sum(xc * yq))
    return d / (Jn * S), de / (SEG * S), 1


def stoi(e, x, fs, dtype=np.float64, drop=None):
    """(STOI, ESTOI, flag, K, F) of one pair.  ``drop``: leave out kept frame number ``drop`` (the sensitivity check of the whole-call test)"""
    x10, e10 = to_10k(x, fs, dtype), to_10k(e, fs, dtype)
    src = kept_frames(x10)
    K, F = len(src), frames_of(len(x10))
    if drop is not None:
        src = np.delete(src, drop)
    X, Y = band_spectra(rebuild(x10, src, dtype), dtype), band_spectra(rebuild(e10, src, dtype), dtype)
    s, es, fl = stoi_scores(X, Y) if len(src) else (float("nan"), float("nan"), 0)
    return s, es, fl, K, F


def lsd(e, x, dtype=np.float64):
    """(LSD dB, flag) at the signals' own rate"""
    ee, xx, _, _, _ = moments(e, x)
    g = math.sqrt(xx / ee) if ee > 0.0 else 1.0
    P = np.abs(spectra(x, dtype)) ** 2
    Q = g * g * np.abs(spectra(e, dtype)) ** 2
    if P.shape[1] == 0 or not P.mean() > 0.0:
        return float("nan"), 0
    d = 1e-8 * P.mean()
    t = 10.0 * np.log10((P + d) / (Q + d))
    return float(np.mean(np.sqrt(np.mean(t * t, axis=0)))), 1


def evaluate(e, x, fs, dtype=np.float64):
    """((SI-SDR, STOI, ESTOI, LSD), flags, K, F) of one pair, as utils.metrics.evaluate reports it"""
    _, _, _, s, f0 = moments(e, x)
    st, es, f1, K, F = stoi(e, x, fs, dtype)
    ls, f3 = lsd(e, x, dtype)
    return np.array([s, st, es, ls]), f0 | f1 << 1 | f1 << 2 | f3 << 3, K, F


def gap_signal(u):
    """the clean test signals of the select and whole-call tests at 16 kHz: synth_clean(u, 24000) with samples 6000..8999 multiplied by 1e-4"""
    from buddy_amd.synth import synth_clean
    x = synth_clean(u, 24000).copy()
    x[6000:9000] *= np.float32(1e-4)
    return x


def read_csv(path):
    """the rows of a report as dicts: empty fields -> NaN; ``file`` / ``value`` stay text; flags, counts and ``n`` -> int; the rest float"""
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            row = {}
            for k, v in r.items():
                if k in ("file", "value"):
                    row[k] = v
                elif k.startswith("flags") or k in ("samples", "kept_frames", "frames", "n"):
                    row[k] = int(v)
                else:
                    row[k] = float("nan") if v == "" else float(v)
            out.append(row)
    return out
