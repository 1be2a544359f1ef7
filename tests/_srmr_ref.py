"""Float64 restatement of the SRMR of DESIGN.md section 18 in numpy / scipy (``fftconvolve``, ``lfilter``), written from the definition and sharing no
code with ``buddy_amd/utils/srmr.py``: the oracle of tests/test_srmr_host.py and tests/test_hip_srmr.py.  One switch (``fp32=True``) forms the
envelope the way an fp32 device does: the fp32 taps, float32 products and float32 running sums over the taps.  Also the test signal ``speechlike``
and a reader for the CSV report."""
import csv
import math

import numpy as np
from scipy import signal

FS = 16000
J, K = 23, 8
W, H = 4096, 1024


def erb(f):
    return np.asarray(f, np.float64) / 9.26449 + 24.7


def centres():
    """23 centre frequencies, highest first"""
    c = 9.26449 * 24.7
    return np.array([-c + math.exp(i * (math.log(125.0 + c) - math.log(8000.0 + c)) / 23.0) * (8000.0 + c) for i in range(1, 24)])


_taps = []


def taps():
    """complex128 taps per channel, highest channel first"""
    if not _taps:
        for cf in centres():
            b = 2.0 * math.pi * 1.019 * float(erb(cf))
            peak = (3.0 / b) ** 3 * math.exp(-3.0)
            n = 1
            last = 1
            while n < 16000:                                     # the last n >= 1 with an envelope of at least 1e-4 of the peak
                t = n / 16000.0
                if t ** 3 * math.exp(-b * t) >= 1e-4 * peak:
                    last = n
                n += 1
            t = np.arange(last + 1) / 16000.0
            g = t ** 3 * np.exp(-b * t) * np.exp(2j * np.pi * cf * t)
            gain = abs(np.sum(g * np.exp(-2j * np.pi * cf * np.arange(last + 1) / 16000.0)))
            _taps.append(g / gain)
    return _taps


def taps32():
    """(re, im) float32 arrays per channel: what the device holds"""
    return [(g.real.astype(np.float32), g.imag.astype(np.float32)) for g in taps()]


def envelope(x, fp32=False):
    """(23, L) float64: env_j[n] = |sum_t g_j[t] x[n - t]|, causal.  ``fp32``: the fp32 taps, every product and every running sum rounded to float32,
    taps ascending, the magnitude in float32 too"""
    x = np.asarray(x, np.float64)
    L = len(x)
    out = np.zeros((J, L))
    if not fp32:
        for j, g in enumerate(taps()):
            out[j] = np.abs(signal.fftconvolve(x, g)[:L])
        return out
    x32 = x.astype(np.float32)
    for j, (gr, gi) in enumerate(taps32()):
        re, im = np.zeros(L, np.float32), np.zeros(L, np.float32)
        for t in range(min(len(gr), L)):
            re[t:] += gr[t] * x32[:L - t]
            im[t:] += gi[t] * x32[:L - t]
        out[j] = np.sqrt(re * re + im * im).astype(np.float64)
    return out


def modulation_centres():
    return 4.0 * 32.0 ** (np.arange(8) / 7.0)


def modulation_lower_edges():
    return modulation_centres() * (math.sqrt(1.0 + 1.0 / 16.0) - 0.25)


def modulation_filters():
    """[(b, a)] * 8, normalised to a[0] = 1"""
    out = []
    for f in modulation_centres():
        w = math.tan(math.pi * f / 16000.0)
        b0 = w / 2.0
        b = np.array([b0, 0.0, -b0])
        a = np.array([1.0 + b0 + w * w, 2.0 * w * w - 2.0, 1.0 - b0 + w * w])
        out.append((b / a[0], a / a[0]))
    return out


def frames_of(n):
    return (n - W) // H + 1 if n >= W else 0


def window():
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * (np.arange(W) + 1.0) / (W + 1.0))


def frame_energies(env):
    """env (..., L) -> E (..., 8, M): the energies of the windowed full frames of every band-pass output (``lfilter``, zero initial state)"""
    env = np.asarray(env, np.float64)
    M = frames_of(env.shape[-1])
    E = np.zeros(env.shape[:-1] + (K, M))
    h = window()
    for k, (b, a) in enumerate(modulation_filters()):
        v = signal.lfilter(b, a, env, axis=-1)
        for m in range(M):
            E[..., k, m] = np.sum((h * v[..., m * H:m * H + W]) ** 2, axis=-1)
    return E


def scores(ebar, M, erbs, low):
    """ebar (J, 8) with the channels in ASCENDING centre frequency, ``erbs`` (J,) likewise, ``low`` (8,) -> (SRMR, K*, BW, flag).  Every sum runs
    element by element in index order (cumsum), as the device's does.  No frame or no energy: (NaN, NaN, NaN, 0); a zero denominator: NaN with
    K* and BW, flag 0"""
    nan = float("nan")
    ebar = np.asarray(ebar, np.float64)
    if M < 1:
        return nan, nan, nan, 0
    A = np.array([np.cumsum(r)[-1] for r in ebar])
    run = np.cumsum(A)
    total = run[-1]
    if not total > 0.0:
        return nan, nan, nan, 0
    first = int(np.nonzero(run > 0.9 * total)[0][0])
    bw = float(erbs[first])
    ks = 5 + sum(1 for k in (5, 6, 7) if bw >= low[k])
    num = den = 0.0
    for r in ebar:
        for k in range(4):
            num += r[k]
        for k in range(4, ks):
            den += r[k]
    if not den > 0.0:
        return nan, float(ks), bw, 0
    return num / den, float(ks), bw, 1


def from_envelope(env):
    """stages 2 and 3 on a (23, L) envelope, highest channel first -> dict(srmr, kstar, bw, flag, frames, energies (23, 8) in that order)"""
    M = frames_of(env.shape[-1])
    E = frame_energies(env)
    ebar = E.mean(axis=-1) if M else np.full((J, K), np.nan)
    s, ks, bw, fl = scores(ebar[::-1], M, erb(centres())[::-1], modulation_lower_edges())
    return dict(srmr=s, kstar=ks, bw=bw, flag=fl, frames=M, energies=ebar)


def to_16k(x, fs):
    """the project's resampler in float64 with the fp32 taps the device holds (scipy multiplies a given window by ``up`` itself)"""
    from buddy_amd.utils import resample as RS
    x = np.asarray(x, np.float64)
    if fs == FS:
        return x
    up, down = RS.ratio(fs, FS)
    h = RS.design_filter(up, down).astype(np.float32).astype(np.float64)
    y = signal.resample_poly(x, up, down, window=h / up, padtype="constant")
    assert len(y) == RS.out_length(len(x), up, down)
    return y


def srmr(x, fs=FS, fp32=False):
    x16 = to_16k(x, fs)
    if fp32:
        x16 = x16.astype(np.float32).astype(np.float64)
    return from_envelope(envelope(x16, fp32))


def speechlike(u, L):
    """coloured noise under a raised half-sine envelope of 4 + u / 2 Hz: energy in the low modulation bands, as speech has"""
    rs = np.random.RandomState(99 + u)
    n = rs.standard_normal(L + 64)
    x = np.convolve(n, np.exp(-np.arange(64) / 8.0))[64:64 + L]
    t = np.arange(L) / 16000.0
    return x * np.maximum(0.0, np.sin(2.0 * np.pi * (4.0 + 0.5 * u) * t)) ** 2


def read_csv(path):
    """the rows of a report as dicts: empty fields -> NaN; ``file`` / ``value`` stay text; flags, counts and ``n`` -> int; the rest float"""
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            row = {}
            for k, v in r.items():
                if k in ("file", "value"):
                    row[k] = v
                elif k.startswith(("flags", "samples", "frames", "kstar")) or k == "n":
                    row[k] = int(v)
                else:
                    row[k] = float("nan") if v == "" else float(v)
            out.append(row)
    return out
