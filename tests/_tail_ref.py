"""float64 numpy restatement of the diffuse late tail of DESIGN.md section 28, independent of the library: what tests/test_tail_host.py checks on
closed forms and tests/test_hip_tail.py compares the kernels against.  Rows come in groups of D consecutive rows; with t_n = (n - Hw) / fs:

  n_d = Hw + half_up(min_rows |s - r| fs / c);  n_f = n_d + half_up(0.5 ms fs / 1000);  n_x = n_d + half_up(ms fs / 1000);  n_e = n_x + R
  E_k = sum_rows sum_{n_f <= n < n_x} u_k[n]^2;  S_k = D sum_{n_f <= n < n_x} exp(-2 delta_k t_n);  A_k = sqrt(E_k / S_k), 0 with flag 4 where E_k = 0
  th(n) = (pi / 2) clip((n - n_x + 1/2) / R, 0, 1);  out_k[n] = cos th u_k[n] + sin th A_k exp(-delta_k t_n) z[n] / nu,  u_k[n] = 0 for n >= n_e
  n <= n_e: the pure response of n samples, flag 2
"""
import math

import numpy as np

HW = 40
PURE, ZERO = 2, 4
EPS = 2.0 ** -53


def half_up(x):
    return int(math.floor(x + 0.5))


def window(rooms, fs, tail_ms, R, D=1):
    """(G, 4) int64: n_d, n_f, n_x, n_e per group"""
    rooms = np.asarray(rooms, dtype=np.float64).reshape(-1, 16)
    out = []
    for g in range(len(rooms) // D):
        rows = rooms[g * D:(g + 1) * D]
        lag = min(math.sqrt(sum((float(r[3 + a]) - float(r[6 + a])) ** 2 for a in range(3))) * fs / float(r[15]) for r in rows)
        n_d = HW + half_up(lag)
        n_x = n_d + half_up(tail_ms * 1e-3 * fs)
        out.append((n_d, n_d + half_up(0.5 * tail_ms * 1e-3 * fs), n_x, n_x + R))
    return np.array(out, dtype=np.int64)


def times(n0, n1, fs):
    return (np.arange(n0, n1, dtype=np.float64) - HW) / float(fs)


def fit(u, n_f, n_x, delta, fs, D=1):
    """u (B, nb, >= n_x) -> (A (G, nb), flags (G,), E (G, nb), S (G, nb)); n_f, n_x per group; delta (G, nb)"""
    u = np.asarray(u, dtype=np.float64)
    B, nb = u.shape[:2]
    G = B // D
    A, E, S, flags = np.zeros((G, nb)), np.zeros((G, nb)), np.zeros((G, nb)), np.zeros(G, dtype=np.int32)
    for g in range(G):
        a, b = int(n_f[g]), int(n_x[g])
        t = times(a, b, fs)
        for k in range(nb):
            E[g, k] = float(np.sum(u[g * D:(g + 1) * D, k, a:b] ** 2))
            S[g, k] = D * float(np.sum(np.exp(-2.0 * delta[g, k] * t)))
            if E[g, k] > 0.0:
                A[g, k] = math.sqrt(E[g, k] / S[g, k])
            else:
                flags[g] |= ZERO
    return A, flags, E, S


def fit_bound(W, D, delta, n_x, fs):
    """relative bound of ONE evaluation of A: each sum of m non-negative terms carries at most (m + c) 2^-53 whatever its order -- E: m = W D terms,
    one rounding each for the square; S: W terms, each exp with its argument's two roundings (|2 delta t| 2^-52 relative on the value) and two ulp of
    exp, then the product with D; the quotient and the square root add 2 more, and the root halves what the sums carry"""
    arg = abs(2.0 * float(delta) * (int(n_x) - HW) / fs)
    return (0.5 * ((W * D + 1) + (W + 5 + 2.0 * arg)) + 2.0) * EPS


def mix(u, n, n_x, R, delta, A, z, fs, D=1, nu=None):
    """u (B, nb, len >= n_x + R) float64, z (B, n) -> (out (B, nb, n), bound (B, nb, n) of ONE evaluation in double).  The bound per sample, in units
    of 2^-53: the angle (pi / 2) x carries two roundings, at most pi absolute, and cos and sin two ulp each: 6 absolute on either, so 6 |u| and
    6 |env| with env = A exp(-delta t) z / nu; the argument of exp carries two roundings, 2 |delta t| relative on its value, and exp two ulp; the
    products, the quotient and the sum add at most 2 on the u part and 6 on the tail: 8 |u| + (14 + 2 |delta t|) |env|.  Nothing below n_x."""
    u = np.asarray(u, dtype=np.float64)
    B, nb = u.shape[:2]
    out, bound = np.zeros((B, nb, n)), np.zeros((B, nb, n))
    idx = np.arange(n)
    t = (idx.astype(np.float64) - HW) / float(fs)
    for b in range(B):
        g = b // D
        nx, ne = int(n_x[g]), int(n_x[g]) + int(R)
        th = (np.pi / 2.0) * np.clip((idx - nx + 0.5) / float(R), 0.0, 1.0)
        for k in range(nb):
            uu = np.zeros(n)
            m = min(n, ne)
            uu[:m] = u[b, k, :m]
            env = A[g, k] * np.exp(-delta[g, k] * t) * np.asarray(z[b], dtype=np.float64) / (1.0 if nu is None else float(nu[b]))
            o = np.cos(th) * uu + np.sin(th) * env
            o[:nx] = uu[:nx]
            out[b, k] = o
            bd = EPS * (8.0 * np.abs(uu) + (14.0 + 2.0 * np.abs(delta[g, k] * t)) * np.abs(env))
            bd[:nx] = 0.0
            bound[b, k] = bd
    return out, bound


def hybrid(u, n, win, R, delta, z, fs, D=1, nu=None):
    """the whole definition on given image-source parts u (B, nb, len): (out (B, nb, n), A (G, nb), flags (B,), bound)"""
    u = np.asarray(u, dtype=np.float64)
    B, nb = u.shape[:2]
    A, fl, _, _ = fit(u, win[:, 1], win[:, 2], delta, fs, D)
    out, bound = mix(u, n, win[:, 2], R, delta, A, z, fs, D, nu)
    flags = np.repeat(fl, D)
    for b in range(B):
        if n <= int(win[b // D, 3]):
            out[b], bound[b], flags[b] = u[b, :, :n], 0.0, PURE
    return out, A, flags, bound


def field_nu(taps):
    """(D,) the analytic standard deviation of the plane-wave field with scale waves^(-1/2): taps (waves, D, W)"""
    taps = np.asarray(taps, dtype=np.float64)
    return np.sqrt((taps ** 2).sum(axis=(0, 2)) / taps.shape[0])
