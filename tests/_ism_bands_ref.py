"""float64 numpy restatement of the banded shoebox response of DESIGN.md section 22, independent of the library, on top of tests/_ism_ref.py: the band
responses u_k, the causal FIR-bank combination h, and the per-sample quantities of their bounds.  A banded room is the 16 doubles of _ism_ref.room (its
own six coefficients are not read), beta (nb, 6) and air (nb,) or None."""
import math

import numpy as np

import _ism_ref as R

HW = R.HW
U = 2.0 ** -53
GAIN_ULPS = 24.0          # see gain_term


def band_images(rm, beta, air, fs, N, max_order=-1):
    """tau [samples], d [m], o (n_img,) and amp (nb, n_img) of every image with tau < N (and order <= max_order), in no particular order"""
    rm, beta = np.asarray(rm, dtype=np.float64), np.asarray(beta, dtype=np.float64).reshape(-1, 6)
    L, s, r, c = rm[0:3], rm[3:6], rm[6:9], float(rm[15])
    air = np.zeros(len(beta)) if air is None else np.asarray(air, dtype=np.float64)
    dmax = c * N / fs
    per_band = [[R._axis(L[a], s[a], r[a], bk[2 * a], bk[2 * a + 1], dmax, max_order) for a in range(3)] for bk in beta]
    ax = per_band[0]                                   # offsets and orders do not depend on the band
    assert len(ax[0][0]) * len(ax[1][0]) * len(ax[2][0]) < 5e7, "restatement: lattice too large for one broadcast"
    d = np.sqrt(ax[0][0][:, None, None] ** 2 + ax[1][0][None, :, None] ** 2 + ax[2][0][None, None, :] ** 2)
    o = ax[0][2][:, None, None] + ax[1][2][None, :, None] + ax[2][2][None, None, :]
    tau = d * fs / c
    keep = tau < N
    if max_order >= 0:
        keep &= o <= max_order
    amp = []
    for k, axk in enumerate(per_band):
        g = axk[0][1][:, None, None] * axk[1][1][None, :, None] * axk[2][1][None, None, :]
        amp.append((g * np.exp(-air[k] * d) / (4.0 * np.pi * d))[keep])
    return tau[keep], d[keep], o[keep], np.stack(amp)


def rir_bands(rm, beta, air, fs, N, max_order=-1, chunk=20000):
    """u (nb, N) float64; M (N,) images per sample; A (nb, N) = sum |A_k sinc w|; G (nb, N) = sum |A_k| w; E (nb, N) = sum e_k |A_k sinc w| with
    e_k = o + GAIN_ULPS + 8 air_k d, the gains' rounding per image in units of 2^-53 (gain_term)"""
    tau, d, o, amp = band_images(rm, beta, air, fs, N, max_order)
    nb = amp.shape[0]
    airv = np.zeros(nb) if air is None else np.asarray(air, dtype=np.float64)
    u, A, G, E = (np.zeros((nb, N)) for _ in range(4))
    M = np.zeros(N, dtype=np.int64)
    taps = np.arange(2 * HW + 1)
    for i in range(0, len(tau), chunk):
        t = tau[i:i + chunk, None]
        n = np.floor(t).astype(np.int64) + taps[None, :]                 # covers every n with n - 2 Hw < tau < n
        x = n - HW - t
        ok = (np.abs(x) < HW) & (n >= 0) & (n < N)
        w = 0.5 * (1.0 + np.cos(np.pi * x / HW))
        sw = np.sinc(x) * w
        nn = n[ok]
        M += np.bincount(nn, minlength=N)
        for k in range(nb):
            a = amp[k, i:i + chunk, None]
            e = (o[i:i + chunk, None] + GAIN_ULPS + 8.0 * airv[k] * d[i:i + chunk, None]) * np.ones_like(x)
            u[k] += np.bincount(nn, weights=(a * sw)[ok], minlength=N)
            A[k] += np.bincount(nn, weights=np.abs(a * sw)[ok], minlength=N)
            G[k] += np.bincount(nn, weights=(np.abs(a) * w)[ok], minlength=N)
            E[k] += np.bincount(nn, weights=(e * np.abs(a * sw))[ok], minlength=N)
    return u, M, A, G, E


def band_bound(N, M, A, G, E):
    """(nb, N): section 20's bound per band without the output-rounding term (u is double) -- M double additions plus a few ulp of sin / cos / sqrt
    on A, the delay's relative rounding times the slope on G -- plus the gains' rounding E 2^-53.

    gain_term: the kernel forms b^e by repeated squaring, at most e - 1 roundings whatever the order of the products, so an axis pair
    b0^|m - q| b1^|m| carries at most o_a of them, the three axes with their two products o + 2, the attenuation exp(-air d) one product, 2 for a
    1-ulp exp and 5 air d for the rounding of its argument (d itself carries a few): at most o + 5 + 5 air d.  The restatement's own gains (six
    np.power of 1 ulp, five products, exp, one product) carry at most 19 + 3 air d.  Together o + 24 + 8 air d units of 2^-53 per image, linear in
    the order."""
    return (M[None, :] + 64) * U * A + 16.0 * (N + HW) * U * G + U * E


def combine(u, bank):
    """h (N,) = sum_k sum_j bank[k][j] u_k[n - j], causal, zero below sample 0; S (N,) = sum_k sum_j |bank[k][j] u_k[n - j]|"""
    N = u.shape[1]
    h = sum(np.convolve(bank[k], u[k])[:N] for k in range(len(bank)))
    S = sum(np.convolve(np.abs(bank[k]), np.abs(u[k]))[:N] for k in range(len(bank)))
    return h, S


def h_bound(h, bank, ub, S):
    """2^-23 |h| for the one fp32 rounding, the band bounds ``ub`` (nb, N) pushed through sum |bank|, (nb Nh + 8) 2^-53 S for the double sum"""
    nb, Nh = bank.shape
    N = len(h)
    pushed = sum(np.convolve(np.abs(bank[k]), ub[k])[:N] for k in range(nb))
    return 2.0 ** -23 * np.abs(h) + pushed + (nb * Nh + 8) * U * S


def naive_bands(rm, beta, air, fs, N, max_order):
    """the definition as a plain triple loop over the images of order <= max_order (small caps only): u (nb, N)"""
    rm, beta = np.asarray(rm, dtype=np.float64), np.asarray(beta, dtype=np.float64).reshape(-1, 6)
    L, s, r, c = rm[0:3], rm[3:6], rm[6:9], float(rm[15])
    nb = len(beta)
    air = [0.0] * nb if air is None else [float(v) for v in air]
    K = max_order + 1
    pairs = [(m, q) for m in range(-K, K + 1) for q in (0, 1) if abs(m - q) + abs(m) <= max_order]
    u = np.zeros((nb, N))
    for mx, qx in pairs:
        for my, qy in pairs:
            for mz, qz in pairs:
                mq = ((mx, qx), (my, qy), (mz, qz))
                if sum(abs(m - q) + abs(m) for m, q in mq) > max_order:
                    continue
                off = [2.0 * m * L[a] + (1 - 2 * q) * s[a] - r[a] for a, (m, q) in enumerate(mq)]
                d = math.sqrt(off[0] ** 2 + off[1] ** 2 + off[2] ** 2)
                tau = d * fs / c
                for k in range(nb):
                    g = 1.0
                    for a, (m, q) in enumerate(mq):
                        g *= beta[k][2 * a] ** abs(m - q) * beta[k][2 * a + 1] ** abs(m)             # Python's 0.0 ** 0 is 1.0
                    amp = g * math.exp(-air[k] * d) / (4.0 * math.pi * d)
                    for n in range(N):
                        x = n - HW - tau
                        if abs(x) < HW:
                            sinc = 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)
                            u[k, n] += amp * sinc * 0.5 * (1.0 + math.cos(math.pi * x / HW))
    return u
