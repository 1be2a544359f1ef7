"""float64 numpy restatement of the room-acoustic definitions of DESIGN.md section 16 (ISO 3382-1), written from the definitions: the oracle of
tests/test_acoustics_host.py and tests/test_hip_acoustics.py.  Per RIR row h[0..N) at rate fs and per band k (band 0 broadband):

  n0 = first index of max |h|;  w = round(0.0025 fs);  ns = max(n0 - w, 0);  t = (n - ns) / fs
  g_k[n] = sum_j bank[k][j] h[n - j + P],  n in [0, N + P),  P = (Nh - 1) / 2
  E_k[n] = sum_{m >= n} g_k[m]^2;  D_k[n] = 10 log10(E_k[n] / E_k[ns]),  n >= ns
  EDT / T20 / T30 = -60 / s of the least-squares line D ~ a + s t over {n >= ns: lo <= D[n] <= hi}, (0, -10), (-5, -25), (-5, -35) dB
  a fit is valid iff |s| (N + P - 1 - n_hi) / fs >= 10 dB, n_hi the last fitted sample
  C50 = 10 log10(sum_{ns <= n < ns + round(0.05 fs)} g^2 / sum_{n >= ns + round(0.05 fs)} g^2)
  DRR = 10 log10(sum_{ns <= n <= n0 + w} g^2 / sum_{n > n0 + w} g^2);  Ts = sum t g^2 / sum g^2 from ns
"""
import csv
import math

import numpy as np

RANGES = ((-10.0, 0.0), (-25.0, -5.0), (-35.0, -5.0))      # (lo, hi) in dB: EDT, T20, T30
EDT, T20, T30, C50, DRR, TS = range(6)


def half_up(x):
    return int(math.floor(x + 0.5))


def argmax_abs(h):
    """first index of max |h|, compared in the array's own precision"""
    return int(np.argmax(np.abs(h)))


def band_signals(h, bank, fir_dtype=np.float64):
    """(nb, N + P): the zero-phase band signals of one row, accumulated in ``fir_dtype`` (float64: the oracle; float32: how much a single-precision
    FIR moves the results, for the tolerances of the whole-call test)"""
    h = np.asarray(h)
    bank = np.asarray(bank)
    nb, Nh = bank.shape
    P, N = (Nh - 1) // 2, len(h)
    if fir_dtype == np.float64:
        return np.stack([np.convolve(h.astype(np.float64), bank[k].astype(np.float64))[P:P + N + P] for k in range(nb)])
    hp = np.concatenate([np.zeros(P, fir_dtype), h.astype(fir_dtype), np.zeros(2 * P, fir_dtype)])      # hp[i] = h[i - P]
    g = np.zeros((nb, N + P), fir_dtype)
    for k in range(nb):
        for j in range(Nh - 1, -1, -1):                      # ascending input index n - j + P
            wj = fir_dtype(bank[k, j])
            if wj != 0:
                g[k] += wj * hp[2 * P - j:2 * P - j + N + P]
    return g


def schroeder_db(g, ns):
    """D[n] for n >= ns (index 0 of the result is n = ns), float64; -inf where the tail energy is zero, NaN for an all-zero signal"""
    e = np.asarray(g, np.float64)[ns:] ** 2
    E = np.cumsum(e[::-1])[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(E / E[0])


def metrics(g, n0, fs):
    """one band signal g (its full valid length) with the row's direct-path index -> (values (6,), flags, D from ns)"""
    g = np.asarray(g, np.float64)
    L = len(g)
    w, n50 = half_up(0.0025 * fs), half_up(0.05 * fs)
    ns = max(n0 - w, 0)
    val = np.full(6, np.nan)
    flags = 0
    D = schroeder_db(g, ns)
    e = g[ns:] ** 2
    total = e.sum()
    if not total > 0:
        return val, flags, D
    t = np.arange(L - ns, dtype=np.float64) / fs
    for q, (lo, hi) in enumerate(RANGES):
        sel = np.nonzero((D >= lo) & (D <= hi))[0]
        if len(sel) < 2:
            continue
        tc = t[sel] - t[sel].mean()
        s = float((tc * (D[sel] - D[sel].mean())).sum() / (tc * tc).sum())
        if not s < 0:
            continue
        val[q] = -60.0 / s
        flags |= 1 << q
        n_hi = ns + int(sel[-1])
        if abs(s) * (L - 1 - n_hi) / fs >= 10.0:
            flags |= 1 << (6 + q)
    late = e[n50:].sum()
    if late > 0:
        val[C50] = 10.0 * np.log10(e[:n50].sum() / late)
        flags |= 1 << C50
    cut = n0 + w + 1 - ns                                    # direct part: ns <= n <= n0 + w
    rest = e[cut:].sum()
    if rest > 0:
        val[DRR] = 10.0 * np.log10(e[:cut].sum() / rest)
        flags |= 1 << DRR
    val[TS] = float((t * e).sum() / total)
    flags |= 1 << TS
    return val, flags, D


def analyse_bands(g_rows, n0s, fs):
    """band signals given: g_rows[b] (nb, L_b) -> values (B, nb, 6), flags (B, nb), curves [b][k] (D from ns)"""
    B, nb = len(g_rows), len(g_rows[0])
    values, flags, curves = np.full((B, nb, 6), np.nan), np.zeros((B, nb), np.int32), []
    for b in range(B):
        curves.append([])
        for k in range(nb):
            values[b, k], flags[b, k], D = metrics(g_rows[b][k], int(n0s[b]), fs)
            curves[b].append(D)
    return values, flags, curves


def decaying_noise(seed, n, n0, decay_db, pre_db=-50.0):
    """seeded fp32 test signal: white noise falling by ``decay_db`` dB from a unit peak at n0 to the last sample, noise at ``pre_db`` before it"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal(n)
    k = np.arange(n, dtype=np.float64)
    env = np.where(k >= n0, 10.0 ** (-decay_db * np.maximum(k - n0, 0.0) / max(n - 1 - n0, 1) / 20.0), 10.0 ** (pre_db / 20.0))
    x = 0.3 * x * env
    x[n0] = 1.0
    return x.astype(np.float32)


def limit_margin_db(D):
    """smallest distance of a finite D[n] to one of the range limits below 0 dB (at 0 dB nothing can flip: D <= 0 on both sides)"""
    d = D[np.isfinite(D)]
    return min(float(np.abs(d - lim).min()) for lim in (-5.0, -10.0, -25.0, -35.0)) if len(d) else np.inf


def whole_call_rows(fs=16000):
    """the inputs of the whole-call test and of profiles/acoustics_accuracy.txt, fp32: the exponential of the host test (T = 0.5 s, 2.2 T long) and
    two synthetic decaying-noise RIRs (13 824 samples falling by 70 dB behind a peak at 37, 12 000 samples falling by 95 dB behind a peak at 0)"""
    T = 0.5
    a = math.log(1000.0) / (T * fs)
    return [np.exp(-a * np.arange(int(round(2.2 * T * fs)), dtype=np.float64)).astype(np.float32),
            decaying_noise(11, 13824, 37, 70.0), decaying_noise(12, 12000, 0, 95.0)]


def value_differences(a, b):
    """largest difference per value kind over rows and bands between two (B, nb, 6) results: relative for the four times, in dB for C50 and DRR;
    positions undefined in both are skipped, one defined in only one of them is an infinite difference"""
    out = np.zeros(6)
    for q in range(6):
        x, y = a[..., q].ravel(), b[..., q].ravel()
        both = np.isfinite(x) & np.isfinite(y)
        if np.any(np.isfinite(x) != np.isfinite(y)):
            out[q] = np.inf
        elif both.any():
            d = np.abs(x[both] - y[both])
            out[q] = float((d if q in (C50, DRR) else d / np.abs(y[both])).max())
    return out


def analyse(rows, fs, bank, fir_dtype=np.float64):
    """RIR rows (a list of 1-D arrays of their own lengths) -> values (B, nb, 6), flags (B, nb), n0 (B,)"""
    n0s = [argmax_abs(np.asarray(r)) for r in rows]
    g_rows = [band_signals(r, bank, fir_dtype) for r in rows]
    values, flags, _ = analyse_bands(g_rows, n0s, fs)
    return values, flags, np.asarray(n0s, np.int32)


def read_csv(path):
    """the rows of a report as dicts: empty fields -> NaN, ``flags`` / ``exponential`` columns -> int, ``file`` / ``band`` stay text, the rest float"""
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            row = {}
            for k, v in r.items():
                if k in ("file", "band"):
                    row[k] = v
                elif k.endswith("flags") or k == "exponential":
                    row[k] = int(v)
                else:
                    row[k] = float("nan") if v == "" else float(v)
            out.append(row)
    return out
