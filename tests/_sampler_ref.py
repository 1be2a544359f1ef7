"""Float64 arbiter of the sampler-step kernels (csrc/sampler.hip) and of one sampler step: numpy only, nothing imported from the library.

Every function restates the reference expression on the fp32 inputs promoted to double and returns the value together with the error bound the
fp32 kernel has to meet, so that the tests only compare.  The bounds are counts of roundings: with u = 2^-24 a bound is (fp32 roundings on the
path) x u x (the sum of the magnitudes of the terms, in float64).  Host scalars (sigma, dt, the perturbation's scale, p0, p1) are rounded to fp32
first, as the C entries receive them.

No tests in this module (tests/test_sampler_kernels_host.py, tests/test_hip_sampler_kernels.py use it)."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
FIR_TOL = 1e-5            # of a row's abs-max: the bound of tests/test_hip_kernels.py::test_fir_and_adjoint
MOMENTS_TOL = 1e-9        # of the abs-max over the rows: the bound of tests/test_hip_kernels.py::test_row_ops


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def f32s(v):
    """a host scalar as the C entry receives it: rounded to fp32, held as a Python float"""
    return float(np.float32(v))


def _col(v):
    return f64(v).reshape(-1, 1)


def perturb(x, eps, s):
    """x + s eps (reference EulerHeunSampler.py:41-45) -> (value, 2u (|x| + |s eps|))"""
    x, eps, s = f64(x), f64(eps), f32s(s)
    return x + s * eps, 2 * U * (np.abs(x) + np.abs(s * eps))


def axpby_rows(x, y, a, c):
    """a[b] x[b] + c[b] y[b], y = None: a[b] x[b] -> (value, 3u (|a x| + |c y|))"""
    ax = _col(a) * f64(x)
    if y is None:
        return ax, 3 * U * np.abs(ax)
    cy = _col(c) * f64(y)
    return ax + cy, 3 * U * (np.abs(ax) + np.abs(cy))


def row_moments(x):
    """(B, 2): sum and sum of squares per row -> (value, (2,) bound per column: 1e-9 of the column's abs-max over the rows)"""
    x = f64(x)
    m = np.stack([x.sum(axis=1), (x * x).sum(axis=1)], axis=1)
    return m, MOMENTS_TOL * np.abs(m).max(axis=0)


def row_scale(x, mode, p0, p1=1.0):
    """mode 0: p0 / std_unbiased(row), the std two-pass; mode 1: p0 / (||row||_2 / p1 + 1e-8) -> (value (B,), 4u |value|).
    The roundings: the square root to fp32, up to two divisions and one add."""
    x, p0, p1 = f64(x), f32s(p0), f32s(p1)
    L = x.shape[1]
    with np.errstate(divide="ignore"):
        if mode == 0:
            mean = x.sum(axis=1, keepdims=True) / L
            v = p0 / np.sqrt(((x - mean) ** 2).sum(axis=1) / (L - 1))
        else:
            v = p0 / (np.sqrt((x * x).sum(axis=1)) / p1 + 1e-8)
    with np.errstate(invalid="ignore"):
        return v, 4 * U * np.abs(v)


DpsUpdate = namedtuple("DpsUpdate", "out d x_den out_bound d_bound")


def dps_update(x_hat, x_den, lh, lh_scale, den_scale, base, d_prev, t, dt, w_prev, w_cur):
    """the comment block above dps_update_kernel (reference EulerHeunSamplerDPS.py:128-157, diff_params/edm.py:83-96):
        x_den' = x_den den_scale[b]                       d = -t (x_den' - x_hat) / t^2 + lh_scale[b] lh
        out    = base + dt (w_prev d_prev + w_cur d)
    lh, lh_scale, den_scale, d_prev may be None.  With S_d = (|x_den'| + |x_hat|) / t + |lh_scale lh| (the sum: the subtraction cancels)
        |d - d64| <= 12u S_d          |out - out64| <= 16u (|base| + |dt| (|w_cur| S_d + |w_prev d_prev|))
    (at most 14 roundings on the longest path)."""
    x_hat, x_den, base = f64(x_hat), f64(x_den), f64(base)
    t, dt, w_prev, w_cur = f32s(t), f32s(dt), f32s(w_prev), f32s(w_cur)
    xd = x_den if den_scale is None else x_den * _col(den_scale)
    d = -t * ((xd - x_hat) / (t * t))
    S = (np.abs(xd) + np.abs(x_hat)) / t
    if lh is not None:
        g = f64(lh) if lh_scale is None else _col(lh_scale) * f64(lh)
        d = d + g
        S = S + np.abs(g)
    acc, A = w_cur * d, abs(w_cur) * S
    if d_prev is not None:
        acc = acc + w_prev * f64(d_prev)
        A = A + np.abs(w_prev * f64(d_prev))
    return DpsUpdate(base + dt * acc, d, xd, 16 * U * (np.abs(base) + abs(dt) * A), 12 * U * S)


def edm_scalars(sigma, sigma_data):
    """(cnoise, cin, cskip, cout) of diff_params/edm.py:44-75 in float64 -> (value (4,), 8u |value|): at most six fp32 roundings, pow / log at 1 ulp"""
    s, sd = float(sigma), float(sigma_data)
    v = np.array([0.25 * np.log(s), (sd * sd + s * s) ** -0.5, sd * sd / (s * s + sd * sd), s * sd * (sd * sd + s * s) ** -0.5], dtype=np.float64)
    return v, 8 * U * np.abs(v)


def fir(x, h, adjoint=False):
    """rows of x (B, L); h shared (M,) or per row (B, M); zero outside [0, L)
        forward: y[n] = sum_m h[m] x[n - m]        adjoint: y[n] = sum_m h[m] x[n + m]
    -> (y (B, L), (B, 1) bound: 1e-5 of the row's abs-max)"""
    x, h = f64(x), f64(h)
    B, L = x.shape
    y = np.empty_like(x)
    for b in range(B):
        hb = h if h.ndim == 1 else h[b]
        y[b] = np.convolve(x[b][::-1], hb)[:L][::-1] if adjoint else np.convolve(x[b], hb)[:L]
    return y, FIR_TOL * np.abs(y).max(axis=1, keepdims=True)


def host_scalars(t_i, t_iplus1, gamma, dtype=np.float32):
    """the schedule arithmetic the sampler does on the host in fp32 (EulerHeunSampler.py:41-45): (t_hat, sqrt(t_hat^2 - t_i^2), t_iplus1 - t_hat)"""
    t_i, t_iplus1, gamma = dtype(float(t_i)), dtype(float(t_iplus1)), dtype(float(gamma))
    t_hat = t_i + gamma * t_i
    return float(t_hat), float((t_hat ** 2 - t_i ** 2) ** dtype(0.5)), float(t_iplus1 - t_hat)


def step(x, eps, t_i, t_iplus1, gamma, order, evals, rescale, speech_scaling=0.05):
    """One sampler step as the reference takes it (EulerHeunSamplerDPS.py:115-157): stochastic perturbation, first evaluation, magnitude rescale
    of the FIRST x_den only (``rescale``), Euler, and for order 2 with t_iplus1 != 0 the Heun corrector on the RAW second x_den.
    ``evals``: per evaluation (likelihood gradient, its per-row scale or None, Tweedie estimate) -- the network / operator part, given.
    -> (x_next, x_den), (bound of x_next, bound of x_den).

    The bounds are the single-kernel bounds propagated linearly: the perturbation's error enters the first update with 1 + |dt| / t_hat and the
    first integrand with 1 / t_hat, the rescale factor (4u relative, row_scale) enters through x_den' ((4 + 1) u |x_den'| on the returned one);
    x_prime's error enters the corrector with 0.5 |dt| / t_iplus1, d1's with 0.5 |dt|, x_hat's (the base) with 1.  x_den of the corrector is
    returned untouched: bound 0."""
    t_hat, ps, dt = host_scalars(t_i, t_iplus1, gamma)
    x_hat, e_hat = perturb(x, eps, ps)
    lh, lhs, x_den = evals[0]
    x_den = f64(x_den)
    scale = row_scale(x_den, 0, speech_scaling)[0] if rescale else None
    r1 = dps_update(x_hat, x_den, lh, lhs, scale, x_hat, None, t_hat, dt, 0.0, 1.0)
    e_scale = 4 * U * np.abs(r1.x_den) if rescale else 0.0
    e_out1 = r1.out_bound + e_hat * (1 + abs(dt) / t_hat) + abs(dt) / t_hat * e_scale
    e_d1 = r1.d_bound + (e_hat + e_scale) / t_hat
    e_den1 = 5 * U * np.abs(r1.x_den) if rescale else np.zeros_like(x_den)
    if order == 2 and f32s(t_iplus1) != 0:
        t2 = f32s(t_iplus1)
        lh2, lhs2, x_den2 = evals[1]
        r2 = dps_update(r1.out, x_den2, lh2, lhs2, None, x_hat, r1.d, t2, dt, 0.5, 0.5)
        e_out2 = r2.out_bound + e_hat + 0.5 * abs(dt) * e_d1 + 0.5 * abs(dt) / t2 * e_out1
        return (r2.out, r2.x_den), (e_out2, np.zeros_like(r2.x_den))
    return (r1.out, r1.x_den), (e_out1, e_den1)
