"""The float64 restatement of the paired comparison (buddy_amd/utils/compare.py, csrc/compare.hip), in numpy on ``rng.words``.
The sums are ``math.fsum`` (exact, rounded once), so every bound of the GPU tests is the kernels' own.  Nothing here is imported by the package."""
import math

import numpy as np

from buddy_amd.utils import rng

BOOT, SIGN = 11, 12
EPS = 2.0 ** -53


def indices(key, n, draw):
    """the n ranks of one resample: (w n) >> 32 in 64-bit integers, w the first n words of draw ``draw`` of purpose 11"""
    return ((rng.words(key, BOOT, draw, n).astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def indices_all(key, n, R, draw0=0):
    """``indices`` of the draws draw0 .. draw0 + R - 1 in one pass over the blocks: (R, n)"""
    blocks = (n + 3) // 4
    w = rng.philox4x32_10((np.arange(blocks, dtype=np.uint64)[None, :], np.arange(draw0, draw0 + R, dtype=np.uint64)[:, None], BOOT, 0), key)
    return ((w.reshape(R, 4 * blocks)[:, :n].astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def bootstrap(d, key, R, draw0=0, idx=None):
    """d: one column (unsorted).  -> means (R,), medians (R,), bound (R,): the resample means by fsum, the medians by np.median of the drawn values, and
    the bound of the kernel's mean, (n + 4) EPS sum cnt |s| / n (see ``mean_bound``).  ``idx``: ``indices_all(key, n, R, draw0)`` where the caller
    has it already"""
    s = np.sort(np.asarray(d, dtype=np.float64))
    n = s.size
    idx = indices_all(key, n, R, draw0) if idx is None else idx
    means, meds, bound = np.empty(R), np.empty(R), np.empty(R)
    for r in range(R):
        v = s[idx[r]]
        means[r] = math.fsum(v) / n
        meds[r] = np.median(v)
        bound[r] = mean_bound(v)
    return means, meds, bound


def mean_bound(v):
    """The kernel's resample mean is a sum of at most n products cnt[k] s[k] (cnt an integer below 2^13: one rounding each) added in some fixed
    order (at most n - 1 additions on any path) and one division: (1 + EPS)^(n + 1) - 1 <= (n + 2) EPS for n <= 8192, relative to sum cnt |s| / n.
    The restatement's fsum / n carries one rounding of the sum and one of the quotient: two more.  (n + 4) EPS sum |v| / n."""
    n = len(v)
    return (n + 4) * EPS * math.fsum(np.abs(v)) / n


def interval(values, k):
    """[theta*_(k), theta*_(R-1-k)]"""
    s = np.sort(values)
    return s[k], s[len(s) - 1 - k]


def total_order_sort(row):
    """``row`` sorted ascending with -0 below +0 (the order of the radix key); equal to np.sort wherever the value is not a zero"""
    b = np.ascontiguousarray(row, dtype=np.float64).view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    key = np.where(neg, ~b, b | np.uint64(1 << 63))
    return np.asarray(row, dtype=np.float64)[np.argsort(key, kind="stable")]


def signs(key, n, P, draw0=0, exhaustive=False):
    """(patterns, n) array of +-1: random patterns from purpose 12 (bit j & 31 of sample j >> 5 of draw draw0 + r), or all 2^n patterns (bit j of r)"""
    j = np.arange(n)
    if exhaustive:
        r = np.arange(2 ** n, dtype=np.int64)
        bits = (r[:, None] >> j[None, :]) & 1
    else:
        blocks = ((n + 31) // 32 + 3) // 4
        w = rng.philox4x32_10((np.arange(blocks, dtype=np.uint64)[None, :], np.arange(draw0, draw0 + P, dtype=np.uint64)[:, None], SIGN, 0), key)
        w = w.reshape(P, 4 * blocks)
        bits = (w[:, j >> 5] >> (j & 31).astype(np.uint32)) & np.uint32(1)
    return 1.0 - 2.0 * bits.astype(np.float64)


def sign_flip(d, key, P, draw0=0):
    """-> T (patterns,), T_obs, bound, exhaustive.  Exhaustive when 2^n <= P.  The sums by fsum; bound = n EPS sum |d|: the kernel adds n terms
    into one accumulator (n - 1 roundings, the negations are exact), the restatement rounds once"""
    d = np.asarray(d, dtype=np.float64)
    n = d.size
    ex = n <= 30 and 2 ** n <= P
    sg = signs(key, n, P, draw0, ex)
    T = np.array([math.fsum(row * d) for row in sg])
    return T, math.fsum(d), n * EPS * math.fsum(np.abs(d)), ex


def p_value(T, thr, exhaustive):
    count = int(np.sum(np.abs(T) >= thr))
    return count / len(T) if exhaustive else (1.0 + count) / (1.0 + len(T))


def p_range(T, tobs, bound, exhaustive):
    """[p_lo, p_hi]: the p-value with the comparison |T| >= |T_obs| moved by the kernel's error on both sides (2 bound), up and down.  In the
    exhaustive mode the first and the last pattern are T_obs and -T_obs by construction (the same additions, every term negated in the last: the
    GPU tests require those bits), so they count whatever the rounding and are left out of the moving"""
    a, t = np.abs(T), abs(tobs)
    if exhaustive:
        a = a.copy()
        a[0] = a[-1] = np.inf
    return p_value(a, t + 2.0 * bound, exhaustive), p_value(a, t - 2.0 * bound, exhaustive)


def sign_test(wins, losses):
    m, k = wins + losses, min(wins, losses)
    if m == 0:
        return 1.0
    return min(1.0, (2 * sum(math.comb(m, i) for i in range(k + 1))) / (1 << m))


def holm(p):
    p = list(p)
    order = sorted(range(len(p)), key=lambda i: p[i])
    out, run = [0.0] * len(p), 0.0
    for j, i in enumerate(order):
        run = max(run, min(1.0, (len(p) - j) * p[i]))
        out[i] = run
    return out


def paired_column(d, label, seed, R, P, level):
    """the GPU part of ``compare.paired`` for one column of differences: the four interval edges and the sign-flip p-value"""
    key = rng.stream_key(seed, label)
    k = int(math.floor((1.0 - level) * R / 2.0 + 1e-9))
    means, meds, _ = bootstrap(d, key, R)
    T, tobs, _, ex = sign_flip(d, key, P)
    return interval(means, k), interval(meds, k), p_value(T, abs(tobs), ex), ex
