"""float64 numpy restatement of the time alignment (include/buddy_hip.h, buddy_xcorr_lag and buddy_align_pair), independent of
the library: the windowed cross-correlation of the zero-mean signals lag by lag, the tie rule, rho, frac and the flags, the trimmed pair, and the
first-order rounding bound the GPU tests assert against."""
import math

import numpy as np

U = 2.0 ** -53


def centred(v):
    """v minus its mean in float64; the mean from an exactly rounded sum"""
    v = np.asarray(v, dtype=np.float64)
    return v - math.fsum(v.tolist()) / len(v)


def xcorr(e, x, K):
    """r[k + K] = sum_m e~[m + k] x~[m] over 0 <= m < n, 0 <= m + k < n, k = -K..K (zero where there is no such m), and the centred signals"""
    et, xt = centred(e), centred(x)
    n = len(et)
    r = np.zeros(2 * K + 1)
    for k in range(-K, K + 1):
        lo, hi = max(0, -k), min(n, n - k)
        if hi > lo:
            r[k + K] = np.dot(et[lo + k:hi + k], xt[lo:hi])
    return r, et, xt


def peak(r, K):
    """the k of the largest |r[k]|; ties to the smallest |k|, then to k >= 0"""
    a = np.abs(r)
    best = None
    for k in range(-K, K + 1):
        key = (a[k + K], -abs(k), k)
        if best is None or key > best[0]:
            best = (key, k)
    return best[1]


def lag(e, x, K):
    """(d, rho, frac, flags, r) of one pair as buddy_xcorr_lag defines them"""
    e, x = np.asarray(e, dtype=np.float64), np.asarray(x, dtype=np.float64)
    n = len(e)
    if n < 2 or not (np.all(np.isfinite(e)) and np.all(np.isfinite(x))):
        return 0, math.nan, 0.0, 0, None
    r, et, xt = xcorr(e, x, K)
    ee, xx = float(np.dot(et, et)), float(np.dot(xt, xt))
    if not (ee > 0.0 and xx > 0.0):
        return 0, math.nan, 0.0, 0, r
    d = peak(r, K)
    rho = r[d + K] / math.sqrt(ee * xx)
    frac = 0.0
    if abs(d) < K:
        a, b, c = abs(r[d + K - 1]), abs(r[d + K]), abs(r[d + K + 1])
        den = a - 2.0 * b + c
        if den < 0.0:
            frac = 0.5 * (a - c) / den
    flags = 1 | (2 if K > 0 and abs(d) == K else 0) | (4 if rho < 0.0 else 0)
    return d, rho, frac, flags, r


def trim(e, x, d):
    """the pair shifted by d and cut to its overlap"""
    n = len(e)
    return np.asarray(e)[max(d, 0):max(d, 0) + n - abs(d)], np.asarray(x)[max(-d, 0):max(-d, 0) + n - abs(d)]


def shift(x, d, fill=0.0):
    """x delayed by d samples (d < 0: advanced), same length, ``fill`` where nothing moved in"""
    x = np.asarray(x)
    out = np.full_like(x, fill)
    n = len(x)
    if d >= 0:
        out[d:] = x[:n - d]
    else:
        out[:n + d] = x[-d:]
    return out


def bound(e, x, K):
    """first-order bound F[k + K] on |computed r[k] - exact r[k]| of ANY double evaluation of the definition from the fp32 inputs (derivation: the
    docstring of tests/test_hip_align.py::test_r_vs_reference): (n + 4) u sum_m |e~[m + k]| |x~[m]| for the terms and their sum, plus
    n u (mean|e| sum_m |x~[m]| + mean|x| sum_m |e~[m + k]|) over the same m for the rounding of the two means; u = 2^-53"""
    et, xt = centred(e), centred(x)
    n = len(et)
    ae, ax = np.abs(et), np.abs(xt)
    ce, cx = np.concatenate([[0.0], np.cumsum(ae)]), np.concatenate([[0.0], np.cumsum(ax)])
    me, mx = float(np.mean(np.abs(np.asarray(e, dtype=np.float64)))), float(np.mean(np.abs(np.asarray(x, dtype=np.float64))))
    F = np.zeros(2 * K + 1)
    for k in range(-K, K + 1):
        lo, hi = max(0, -k), min(n, n - k)
        if hi > lo:
            s = float(np.dot(ae[lo + k:hi + k], ax[lo:hi]))
            F[k + K] = (n + 4) * U * s + n * U * (me * (cx[hi] - cx[lo]) + mx * (ce[hi + k] - ce[lo + k]))
    return F
