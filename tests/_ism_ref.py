"""float64 numpy restatement of the shoebox image-source response of DESIGN.md section 20, independent of the library: what tests/test_rooms_host.py
checks on closed forms and tests/test_hip_rooms.py compares the kernel against.  A room is 16 doubles: L (3), s (3), r (3), beta (6: x0 x1 y0 y1 z0 z1), c."""
import math

import numpy as np

HW = 40


def room(L, s, r, beta, c=343.0):
    beta = [beta] * 6 if np.isscalar(beta) else list(beta)
    return np.array(list(L) + list(s) + list(r) + beta + [c], dtype=np.float64)


def _axis(L, s, r, b0, b1, dmax, max_order):
    """every (m, q) of one axis whose offset can lie inside dmax: offsets, gains, orders"""
    mm = int(math.floor(dmax / (2.0 * L))) + 1
    m = np.repeat(np.arange(-mm, mm + 1), 2)
    q = np.tile(np.array([0, 1]), 2 * mm + 1)
    X = 2.0 * m * L + (1 - 2 * q) * s - r
    e0, e1 = np.abs(m - q), np.abs(m)
    g = np.power(float(b0), e0.astype(np.float64)) * np.power(float(b1), e1.astype(np.float64))      # numpy's 0 ** 0 is 1
    o = e0 + e1
    keep = np.abs(X) <= dmax
    if max_order >= 0:
        keep &= o <= max_order
    return X[keep], g[keep], o[keep]


def images(rm, fs, N, max_order=-1):
    """(tau [samples], A) of every image with tau < N (and order <= max_order), in no particular order"""
    rm = np.asarray(rm, dtype=np.float64)
    L, s, r, beta, c = rm[0:3], rm[3:6], rm[6:9], rm[9:15], float(rm[15])
    dmax = c * N / fs
    ax = [_axis(L[a], s[a], r[a], beta[2 * a], beta[2 * a + 1], dmax, max_order) for a in range(3)]
    assert len(ax[0][0]) * len(ax[1][0]) * len(ax[2][0]) < 5e7, "restatement: lattice too large for one broadcast"
    d = np.sqrt(ax[0][0][:, None, None] ** 2 + ax[1][0][None, :, None] ** 2 + ax[2][0][None, None, :] ** 2)
    g = ax[0][1][:, None, None] * ax[1][1][None, :, None] * ax[2][1][None, None, :]
    o = ax[0][2][:, None, None] + ax[1][2][None, :, None] + ax[2][2][None, None, :]
    tau = d * fs / c
    keep = tau < N
    if max_order >= 0:
        keep &= o <= max_order
    return tau[keep], (g / (4.0 * np.pi * d))[keep]


def rir(rm, fs, N, max_order=-1, chunk=20000):
    """h (N,) float64; M (N,) images per sample; A (N,) = sum |A_i sinc w|; G (N,) = sum |A_i| w"""
    tau, amp = images(rm, fs, N, max_order)
    h, A, G = np.zeros(N), np.zeros(N), np.zeros(N)
    M = np.zeros(N, dtype=np.int64)
    taps = np.arange(2 * HW + 1)
    for i in range(0, len(tau), chunk):
        t, a = tau[i:i + chunk, None], amp[i:i + chunk, None]
        n = np.floor(t).astype(np.int64) + taps[None, :]                 # covers every n with n - 2 Hw < tau < n
        x = n - HW - t
        ok = (np.abs(x) < HW) & (n >= 0) & (n < N)
        w = 0.5 * (1.0 + np.cos(np.pi * x / HW))
        sw = np.sinc(x) * w
        nn = n[ok]
        h += np.bincount(nn, weights=(a * sw)[ok], minlength=N)
        A += np.bincount(nn, weights=np.abs(a * sw)[ok], minlength=N)
        G += np.bincount(nn, weights=(np.abs(a) * w)[ok], minlength=N)
        M += np.bincount(nn, minlength=N)
    return h, M, A, G


def bound(h, M, A, G):
    """the bound of the GPU tests: output rounding, M double additions plus a few ulp of sin / cos / sqrt, the delay's relative rounding times the slope"""
    N = len(h)
    return 2.0 ** -23 * np.abs(h) + (M + 64) * 2.0 ** -53 * A + 16.0 * (N + HW) * 2.0 ** -53 * G


def naive(rm, fs, N, max_order):
    """the definition as a plain triple loop over the images of order <= max_order (small caps only)"""
    rm = np.asarray(rm, dtype=np.float64)
    L, s, r, beta, c = rm[0:3], rm[3:6], rm[6:9], rm[9:15], float(rm[15])
    K = max_order + 1
    per_axis = []
    for a in range(3):
        lst = []
        for m in range(-K, K + 1):
            for q in (0, 1):
                o = abs(m - q) + abs(m)
                if o <= max_order:
                    lst.append((2.0 * m * L[a] + (1 - 2 * q) * s[a] - r[a], beta[2 * a] ** abs(m - q) * beta[2 * a + 1] ** abs(m), o))
        per_axis.append(lst)
    h = np.zeros(N)
    count = 0
    for X, gx, ox in per_axis[0]:
        for Y, gy, oy in per_axis[1]:
            for Z, gz, oz in per_axis[2]:
                if ox + oy + oz > max_order:
                    continue
                count += 1
                d = math.sqrt(X * X + Y * Y + Z * Z)
                tau, amp = d * fs / c, gx * gy * gz / (4.0 * math.pi * d)
                for n in range(N):
                    x = n - HW - tau
                    if abs(x) < HW:
                        sinc = 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)
                        h[n] += amp * sinc * 0.5 * (1.0 + math.cos(math.pi * x / HW))
    return h, count
