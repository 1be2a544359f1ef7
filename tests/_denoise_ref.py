"""Float64 restatement of DESIGN.md section 27 (noise power tracker and spectral post-filter) for tests/test_denoise_host.py and
tests/test_hip_denoise.py, and the signals both use.  numpy / scipy on the host; nothing here touches the GPU.

Frames of N = 512 at hop H = 128 overhanging both ends by P = 384; window w[i] = 0.5 - 0.5 cos(2 pi (i + 1) / 513); Y = DFT(w frame); the tracker of
Gerkmann & Hendriks with the decision-directed Wiener / log-spectral-amplitude gain per bin; synthesis sum_t w x^_t / sum_t w^2.

``fp32=True`` rounds the stages the device runs in single precision -- the window product, the forward transform (scipy.fft on float32 input), the
stored G and sigma^2, the product G Y and the inverse transform -- and leaves the rest float64.  The difference between the two runs is the ``D32``
of the whole-call test.  ``track`` runs in any numpy float type: its float64 / longdouble difference is the recursion's own round-off sensitivity."""
import math

import numpy as np
import scipy.fft

N, H, P, BINS = 512, 128, 384, 257
ZERO, SHORT, NO_SPEECH = 1, 2, 4
XI1 = 10.0 ** 1.5
XI_MIN = 10.0 ** -2.5
FLOOR = 1e-10
EULER = "0.57721566490153286060651209008240243104215933593992"


def frames(L):
    return (int(L) - 1 + P) // H + 1


def full_frames(L):
    return (int(L) - N) // H + 1 if int(L) >= N else 0


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(N, dtype=np.float64) + 1.0) / (N + 1.0))


def frame_matrix(x):
    """(T, 512) float64: frame t = samples t H - P .. t H - P + 511, zeros outside the row"""
    x = np.asarray(x, np.float64)
    T = frames(len(x))
    xp = np.zeros(P + (T - 1) * H + N)
    xp[P:P + len(x)] = x
    return xp[np.arange(T)[:, None] * H + np.arange(N)[None, :]]


def spectra(x, fp32=False):
    """(T, 257) complex128"""
    fr = frame_matrix(x)
    if fp32:
        return scipy.fft.rfft(window().astype(np.float32)[None, :] * fr.astype(np.float32), axis=1).astype(np.complex128)
    return np.fft.rfft(window()[None, :] * fr, axis=1)


def row_floor(x):
    x = np.asarray(x, np.float64)
    return FLOOR * N * float(np.mean(x * x))


def expint_e1(x):
    """E1(x), x > 0, in x's float type: the power series below 1, the continued fraction (modified Lentz) from 1 on"""
    x = np.asarray(x)
    dt = x.dtype.type
    out = np.empty_like(x)
    lo = x < 1
    if lo.any():
        xl = x[lo]
        term, total = np.ones_like(xl), np.zeros_like(xl)
        for n in range(1, 41):
            term = term * (-xl / dt(n))
            total = total + term / dt(n)
        out[lo] = -dt(EULER) - np.log(xl) - total
    if (~lo).any():
        xh = x[~lo]
        b = xh + dt(1)
        c = np.full_like(xh, dt(1e300))
        d = dt(1) / b
        h = d.copy()
        eps = np.finfo(x.dtype).eps
        for i in range(1, 401):
            an = -dt(i) * dt(i)
            b = b + dt(2)
            d = dt(1) / (an * d + b)
            c = b + an / c
            de = c * d
            h = h * de
            if np.all(np.abs(de - dt(1)) <= eps):
                break
        out[~lo] = h * np.exp(-xh)
    return out


def track(power, phi, L, gain="lsa", floor_db=-15.0, dtype=np.float64):
    """power (R, T, 257): |Y|^2 of R rows of one length L; phi (R,) > 0.  Returns G, sigma2 (R, T, 257) in ``dtype`` and a dict of what the run
    reached: ``capped`` bin-frames with Pbar > 0.99, ``ag_min`` / ``ag_max`` of the exponential integral's argument, ``floored`` bin-frames at phi."""
    dt = np.dtype(dtype).type
    pw = np.asarray(power).astype(dtype)
    R, T, K = pw.shape
    assert T == frames(L) and K == BINS
    ph = np.asarray(phi).astype(dtype).reshape(R, 1)
    full = full_frames(L)
    first = pw[:, 3:3 + min(8, full)] if full else pw
    sig = np.maximum(first.sum(axis=1) / dt(first.shape[1]), ph)
    pbar, a2 = np.full((R, K), dt(0.5)), np.zeros((R, K), dtype)
    gmin = dt(10.0 ** (floor_db / 20.0))
    # the constants are the double values the device holds, in either type: the two runs differ in their arithmetic alone
    xi1, c9, c1, c8, c2, c98, c02, cap, one = dt(XI1), dt(0.9), dt(0.1), dt(0.8), dt(0.2), dt(0.98), dt(0.02), dt(0.99), dt(1)
    G, S = np.empty((R, T, K), dtype), np.empty((R, T, K), dtype)
    seen = dict(capped=0, ag_min=math.inf, ag_max=0.0, floored=0)
    for t in range(T):
        y2 = pw[:, t]
        p = one / (one + (one + xi1) * np.exp(-(y2 / sig) * (xi1 / (one + xi1))))
        pbar = c9 * pbar + c1 * p
        over = pbar > cap
        p = np.where(over, np.minimum(p, cap), p)
        sig = np.maximum(c8 * sig + c2 * (p * sig + (one - p) * y2), ph)
        gam = np.clip(y2 / sig, dt(1e-6), dt(1e3))
        xi = np.maximum(c98 * a2 / sig + c02 * np.maximum(gam - one, dt(0)), dt(XI_MIN))
        a = xi / (one + xi)
        if gain == "lsa":
            ag = a * gam
            g = np.minimum(a * np.exp(expint_e1(ag) / dt(2)), one)
            seen["ag_min"], seen["ag_max"] = min(seen["ag_min"], float(ag.min())), max(seen["ag_max"], float(ag.max()))
        else:
            assert gain == "wiener"
            g = a
        g = np.maximum(g, gmin)
        a2 = g * g * y2
        G[:, t], S[:, t] = g, sig
        seen["capped"] += int(over.sum())
        seen["floored"] += int((sig == ph).sum())
    return G, S, seen


def synthesis(Y, G, L, fp32=False):
    """Y (T, 257) complex, G (T, 257) -> (L,) float64"""
    T = frames(L)
    if fp32:
        g = np.asarray(G).astype(np.float32)
        Z = np.empty(Y.shape, np.complex64)
        Z.real, Z.imag = g * Y.real.astype(np.float32), g * Y.imag.astype(np.float32)
        xh = scipy.fft.irfft(Z, n=N, axis=1).astype(np.float64)
    else:
        xh = np.fft.irfft(np.asarray(G, np.float64) * Y, n=N, axis=1)
    w = window()
    num, den = np.zeros(P + (T - 1) * H + N), np.zeros(P + (T - 1) * H + N)
    for t in range(T):                                   # t ascending: the order of the device's four-term sums
        num[t * H:t * H + N] += w * xh[t]
        den[t * H:t * H + N] += w * w
    return num[P:P + L] / den[P:P + L]


def stats(x, out, Y, sigma2):
    """snr_est_db, noise_db, att_db, flags of one row; sigma2 as stored (T, 257)"""
    x, out = np.asarray(x, np.float64), np.asarray(out, np.float64)
    flags = SHORT if len(x) < N else 0
    sx = float(np.sum(x * x))
    if not sx > 0.0:
        return math.nan, math.nan, math.nan, flags | ZERO
    s2 = np.asarray(sigma2, np.float64)
    num, den = float(np.sum(np.maximum(np.abs(Y) ** 2 - s2, 0.0))), float(np.sum(s2))
    if not num > 0.0:
        flags |= NO_SPEECH
    so = float(np.sum(out * out))
    w2 = float(np.sum(window() ** 2))
    return (10.0 * math.log10(num / den) if num > 0.0 else -math.inf, 10.0 * math.log10(den / s2.size / w2),
            10.0 * math.log10(sx / so) if so > 0.0 else math.inf, flags)


def denoise(x, gain="lsa", floor_db=-15.0, fp32=False):
    """one row -> dict(out, G, sigma2, Y, snr_est_db, noise_db, att_db, flags, frames, seen)"""
    x = np.asarray(x, np.float64)
    L, T = len(x), frames(len(x))
    Y = spectra(x, fp32)
    phi = row_floor(x)
    if not phi > 0.0:
        G, S, seen = np.ones((T, BINS)), np.zeros((T, BINS)), {}
    else:
        G, S, seen = track((np.abs(Y) ** 2)[None], [phi], L, gain, floor_db)
        G, S = G[0], S[0]
    if fp32:
        G, S = G.astype(np.float32).astype(np.float64), S.astype(np.float32).astype(np.float64)
    out = synthesis(Y, G, L, fp32) if phi > 0.0 else np.zeros(L)
    snr, noise, att, flags = stats(x, out, Y, S)
    return dict(out=out, G=G, sigma2=S, Y=Y, snr_est_db=snr, noise_db=noise, att_db=att, flags=flags, frames=T, seen=seen, phi=phi)


# ---- the signals of the tests ---------------------------------------------------------------------------------------------------------------------
FS = 16000
EDGE_LENGTHS = (1, 127, 128, 129, 511, 512, 513, 700)
EDGE_FRAMES = (4, 4, 4, 5, 7, 7, 8, 9)


def bursts(L=48000, seed=0, fs=FS, start=0.5):
    """clean "speech": raised-cosine-squared bursts of 150 ms every 300 ms from ``start`` s on; burst k is white noise through exp(-j / a_k), 64 taps,
    a_k cycling through 2, 4, 8, 16, at unit standard deviation under the envelope; the row has unit mean square.  Returns (row, burst mask)"""
    rs = np.random.RandomState(seed)
    M, step = int(0.15 * fs), int(0.3 * fs)
    env = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(M) / M)) ** 2
    x, mask = np.zeros(L), np.zeros(L, bool)
    for k, s in enumerate(range(int(start * fs), L - M + 1, step)):
        h = np.exp(-np.arange(64) / (2.0, 4.0, 8.0, 16.0)[k % 4])
        b = np.convolve(rs.standard_normal(M + 63), h, mode="valid")
        x[s:s + M] = env * b / b.std()
        mask[s:s + M] = True
    return x / math.sqrt(np.mean(x * x)), mask


def noisy_bursts(snr_db, L=48000, seed=0, fs=FS, start=0.5):
    """(noisy float32, clean float64, noise float64, burst mask): white noise at ``snr_db`` below the clean row's unit mean square"""
    clean, mask = bursts(L, seed, fs, start)
    noise = 10.0 ** (-snr_db / 20.0) * np.random.RandomState(1000 + seed).standard_normal(L)
    return (clean + noise).astype(np.float32), clean, noise, mask


def white(L, std, seed):
    return (std * np.random.RandomState(seed).standard_normal(L)).astype(np.float32)


def tone_row(L=12000, seed=3, fs=FS):
    """0.01 N(0, 1) with a unit 1 kHz tone from sample 3000 on"""
    x = 0.01 * np.random.RandomState(seed).standard_normal(L)
    n = np.arange(L)
    x[3000:] += np.sin(2.0 * np.pi * 1000.0 * n[3000:] / fs)
    return x.astype(np.float32)


def silence_led(zeros=2000, L=6000, seed=4):
    x = np.zeros(L, np.float32)
    x[zeros:] = white(L - zeros, 0.05, seed)
    return x


def gap_mask(mask, fs=FS, margin=256, start=0.5):
    """samples more than ``margin`` from every burst, after ``start`` s"""
    near = np.convolve(mask.astype(np.float64), np.ones(2 * margin + 1), mode="same") > 0.5
    out = ~near
    out[:int(start * fs)] = False
    return out


def si_sdr(est, ref):
    est, ref = np.asarray(est, np.float64), np.asarray(ref, np.float64)
    s = (np.dot(est, ref) / np.dot(ref, ref)) * ref
    return 10.0 * math.log10(np.dot(s, s) / np.dot(est - s, est - s))
