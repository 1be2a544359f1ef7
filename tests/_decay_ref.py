"""A float64 numpy restatement of the blind decay time of DESIGN.md section 30 (steps 1-5), written from the definition and independent of
csrc/decay.hip: np.fft for the frame spectra, plain loops for the regions.  The host tests show that it meets the functional condition on its own;
the GPU tests hold the library to it.  Also the gated-burst source and the synthetic response of that condition."""
import math

import numpy as np

FS, FRAME, HOP, K = 16000, 512, 128, 5
BIN_HZ = FS / FRAME
CENTRES = (125, 250, 500, 1000, 2000, 4000)
BROADBAND = (88.39, 5656.85)
DEFINED, FEW, ABOVE_RATE, SHORT = 1, 2, 4, 8
U32, U64 = 2.0 ** -24, 2.0 ** -53


def frames_of(n):
    return (n - FRAME) // HOP + 1 if n >= FRAME else 0


def window():
    """the interior of a Hann window of 514 points, float64"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(FRAME) + 1.0) / (FRAME + 1.0))


def bands(fs=FS):
    """[(lo bin, hi bin, above)] for an input rate ``fs``; an octave whose upper edge exceeds 0.45 fs is (0, 0, True)"""
    top = 0.45 * fs
    out = []
    for k in range(7):
        if k == 0:
            lo, hi, above = BROADBAND[0], min(BROADBAND[1], top), False
        else:
            lo, hi = CENTRES[k - 1] / math.sqrt(2.0), CENTRES[k - 1] * math.sqrt(2.0)
            above = hi > top
        bins = [b for b in range(FRAME // 2 + 1) if lo <= b * BIN_HZ < hi]
        out.append((0, 0, True) if above else (bins[0], bins[-1] + 1, False))
    return out


def energies(x, fs=FS):
    """x: 1-D samples at 16 kHz (``fs``: the rate they came from, for the band edges) -> (E (7, M) float64, total (M,): the whole frame's spectral
    energy sum_{k < 512} |X[k]|^2, which scales the fp32 transform's error bound)"""
    x = np.asarray(x, dtype=np.float64)
    M = frames_of(len(x))
    if M == 0:
        return np.zeros((7, 0)), np.zeros(0)
    idx = np.arange(M)[:, None] * HOP + np.arange(FRAME)[None, :]
    fr = x[idx] * window()[None, :]
    P = np.abs(np.fft.rfft(fr, axis=1)) ** 2
    E = np.zeros((7, M))
    for i, (lo, hi, _) in enumerate(bands(fs)):
        for k in range(lo, hi):                      # ascending k
            E[i] += P[:, k]
    return E, FRAME * np.sum(fr * fr, axis=1)


def smooth(E):
    """S[m] = (((E[m] + E[m+1]) + E[m+2]) + E[m+3]) + E[m+4], m = 0 .. M - 5"""
    M = len(E)
    if M < K:
        return np.zeros(0)
    n = M - K + 1
    return (((E[0:n] + E[1:n + 1]) + E[2:n + 2]) + E[3:n + 3]) + E[4:n + 4]


def regions(E, q, floor_rel=1e-6, lmin=6):
    """one band's E (M,) -> [(m0, frames, T, cond)] of the kept regions in frame order; ``cond`` is the condition number of the slope's numerator with
    respect to relative errors of its two sums of d, (n |sum j d| + sum j |sum d|) / |n sum j d - sum j sum d|, which scales the test's bound"""
    S = smooth(np.asarray(E, dtype=np.float64))
    Ms = len(S)
    if Ms == 0:
        return []
    floor = floor_rel * float(np.max(S))
    step = [bool(S[m + 1] < S[m] and S[m + 1] > floor) for m in range(Ms - 1)]
    out, m = [], 0
    while m < Ms - 1:
        if not step[m]:
            m += 1
            continue
        m0 = m
        while m < Ms - 1 and step[m]:
            m += 1
        m1 = m
        if m1 - m0 + 1 >= lmin and S[m0] > floor and S[m1] <= S[m0] * q:
            n = sj = sjj = sd = sjd = 0.0
            for j in range(m1 - m0 + 1):             # ascending j
                d = 10.0 * math.log10(S[m0 + j] / S[m0])
                n += 1.0
                sj += float(j)
                sjj += float(j) * float(j)
                sd += d
                sjd += float(j) * d
            num = n * sjd - sj * sd
            slope = num / (n * sjj - sj * sj)
            if slope < 0.0:
                out.append((m0, m1 - m0 + 1, -60.0 / slope * HOP / FS, (n * abs(sjd) + sj * abs(sd)) / abs(num)))
    return out


def select(T):
    """(t60, q1, q3) of a list of decay times: the order statistics of rank (n-1)//2, (n-1)//4, 3(n-1)//4; NaN without any"""
    n = len(T)
    if n == 0:
        return (float("nan"),) * 3
    s = sorted(T)
    return s[(n - 1) // 2], s[(n - 1) // 4], s[3 * (n - 1) // 4]


def flag_word(n, M, above, lmin=6):
    return (DEFINED if n >= 1 else 0) | (FEW if n < 3 else 0) | (ABOVE_RATE if above else 0) | (SHORT if M < K + lmin else 0)


def from_energies(E, drop_db=10.0, floor_db=-60.0, lmin=6, above=None):
    """steps 2-5 on E (NB, M) -> dict of per-band lists: t60, q1, q3, regions, flags, and ``lists``: the region tuples of each band"""
    q, floor_rel = 10.0 ** (-drop_db / 10.0), 10.0 ** (floor_db / 10.0)
    res = {"t60": [], "q1": [], "q3": [], "regions": [], "flags": [], "lists": []}
    for i in range(len(E)):
        r = regions(E[i], q, floor_rel, lmin)
        t = select([v[2] for v in r])
        res["t60"].append(t[0]); res["q1"].append(t[1]); res["q3"].append(t[2])
        res["regions"].append(len(r))
        res["flags"].append(flag_word(len(r), E.shape[1], bool(above[i]) if above is not None else False, lmin))
        res["lists"].append(r)
    return res


def decay_times(x, fs=FS, **kw):
    """steps 1-5 of one row of samples at 16 kHz"""
    E, _ = energies(x, fs)
    return from_energies(E, above=[b[2] for b in bands(fs)], **kw)


def time_bound(n, cond):
    """relative bound on |T_library - T_restatement| of a region of n points, both sides fed the same S.  Each side's d[j] carries one division,
    one log10 (<= 2 ulp in the library, <= 1 ulp here) and one product: <= 5 u relative; its sums of n non-positive terms add (n - 1) u, so each
    of sum d and sum j d is within eta = (n + 5) u of its exact value, relatively.  The numerator n sum j d - sum j sum d then moves by at most
    eta * cond relatively per side (the sums of j are exact integers), and the quotient, -60 / slope and the two scalings add 6 u per side."""
    return 2.0 * ((n + 5) * cond + 6.0) * U64


# ---- the functional condition's signals --------------------------------------------------------------------------------------------------
def burst_source(seed, seconds=8.0, fs=FS):
    """gated bursts of low-passed noise: on 0.12-0.4 s, off 0.15-0.5 s, 5 ms linear ramps, gains 0.3-1"""
    rs = np.random.RandomState(seed)
    n = int(seconds * fs)
    x = np.zeros(n)
    h = np.exp(-np.arange(64) / 8.0)
    ramp = int(0.005 * fs)
    pos = 0
    while pos < n:
        on = int(rs.uniform(0.12, 0.4) * fs)
        off = int(rs.uniform(0.15, 0.5) * fs)
        b = np.convolve(rs.standard_normal(on + 64), h)[64:64 + on]
        r = np.linspace(0.0, 1.0, ramp)
        b[:ramp] *= r
        b[-ramp:] *= r[::-1]
        b *= rs.uniform(0.3, 1.0)
        m = min(on, n - pos)
        x[pos:pos + m] = b[:m]
        pos += on + off
    return x


def response(seed, t60, fs=FS):
    """exponentially decaying noise of decay time ``t60``, tap 0 set to 1"""
    rs = np.random.RandomState(100 + seed)
    n = int(1.5 * t60 * fs)
    h = np.exp(-6.908 * np.arange(n) / fs / t60) * rs.standard_normal(n) * 0.3
    h[0] = 1.0
    return h


def reverberant(seed, t60):
    """the full convolution of the burst source with the response"""
    x, h = burst_source(seed), response(seed, t60)
    n = len(x) + len(h) - 1
    L = 1 << (n - 1).bit_length()
    return np.fft.irfft(np.fft.rfft(x, L) * np.fft.rfft(h, L), L)[:n]


# ---- crafted energies: steps 2-5 on given doubles -----------------------------------------------------------------------------------------
def energies_for(S):
    """E (len(S) + 4,) whose sums of five are exactly the integer-valued S: E[0] = S[0], E[1..4] = 0, E[m + 5] = E[m] + S[m + 1] - S[m].  Every value
    is an integer far below 2^53, so every sum is exact and a tie or a threshold designed into S holds to the bit.  E is not non-negative; only S
    enters steps 3-5"""
    S = np.asarray(S, dtype=np.float64)
    assert np.all(S == np.round(S)) and np.all(np.abs(S) < 2.0 ** 45)
    E = np.zeros(len(S) + K - 1)
    E[0] = S[0]
    for m in range(len(S) - 1):
        E[m + K] = E[m] + (S[m + 1] - S[m])
    assert np.array_equal(smooth(E), S)
    return E


def fall(start, n, db_per_frame):
    """n strictly decreasing integers from ``start``"""
    v = np.round(start * 10.0 ** (-db_per_frame * np.arange(n) / 10.0))
    assert np.all(np.diff(v) < 0)
    return v


def crafted_cases(tile):
    """[(name, E (M,), q, want)]: ``want`` is the list of (m0, frames) the case is built to keep, or None where the case does not pin it"""
    q10, top = 10.0 ** -1.0, 2.0 ** 40
    flat = lambda n, v=top: np.full(n, float(v))
    cat = lambda *p: energies_for(np.concatenate(p))
    cases = []
    # a tie inside a fall ends the run; the next run starts at the tie's second value
    f = fall(top, 20, 3.0)
    cases.append(("tie", cat(flat(3), f[:9], f[8:9], f[9:], flat(4)), q10, [(3, 9), (12, 12)]))
    cases.append(("run to the last frame", cat(flat(7), fall(top, 30, 1.0)[1:]), q10, [(6, 30)]))
    for M in (tile - 1, tile, tile + 1):             # a fall that ends with the row, rows around one tile
        cases.append((f"M = {M}", cat(flat(M - 4 - 25), fall(top, 26, 1.5)[1:]), q10, [(M - 4 - 26, 26)]))
    for m0 in (tile - 9, tile - 2, tile - 1, tile, tile + 1):       # falls that cross the tile boundary, or start next to it
        cases.append((f"fall from frame {m0}", cat(flat(m0 + 1), fall(top, 31, 1.0)[1:], flat(50)), q10, [(m0, 31)]))
    cases.append(("whole row, short", energies_for(fall(top, 36, 1.0)), q10, [(0, 36)]))
    cases.append(("whole row, three tiles", energies_for(fall(top, 3 * tile - 4, 50.0 / (3 * tile))), q10, [(0, 3 * tile - 4)]))
    cases.append(("a long fall from the second tile", cat(flat(tile + 40), fall(top, 2 * tile + 60, 55.0 / (2 * tile + 60))[1:], flat(9)), q10,
                  [(tile + 39, 2 * tile + 60)]))
    for M in (0, 4, 5, 10, 11):
        cases.append((f"M = {M}", np.zeros(M) if M < K else energies_for(fall(top, M - 4, 3.0)), q10, [(0, M - 4)] if M - 4 >= 6 else []))
    cases.append(("all zero", np.zeros(60), q10, []))
    cases.append(("constant", energies_for(flat(60)), q10, []))
    cases.append(("never 10 dB", cat(flat(5), fall(top, 40, 0.2)[1:], flat(5)), q10, []))
    cases.append(("below the floor", cat(flat(3), fall(top, 40, 2.0)[1:], flat(3, 5.0)), q10, [(2, 31)]))       # the run ends where S passes 1e-6 max
    # q = 1/8 is exact: S[m1] = S[m0] / 8 is kept, one more is not
    ramp = np.array([4096.0, 3000.0, 2000.0, 1500.0, 1000.0, 700.0])
    cases.append(("exactly on q", cat(flat(3, 4096), ramp[1:], [512.0], flat(3, 4096)), 0.125, [(2, 7)]))
    cases.append(("one above q", cat(flat(3, 4096), ramp[1:], [513.0], flat(3, 4096)), 0.125, []))
    rates = (3.0, 1.0, 2.0, 1.5)
    for n in (1, 2, 3, 4):                           # n regions of different slopes: the ranks
        parts, want, at = [flat(4)], [], 3
        for r in rates[:n]:
            parts += [fall(top, 16, r)[1:], flat(5)]
            want.append((at, 16))
            at += 20
        cases.append((f"{n} regions", cat(*parts), q10, want))
    return cases
