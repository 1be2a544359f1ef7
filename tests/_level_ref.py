"""Float64 restatement of the active speech level as plain loops over the definition, for tests/test_hip_level.py and
tests/test_level_host.py.  It shares no code with buddy_amd/utils/level.py.  Besides the values it returns the counts with every threshold moved
by +eps and by -eps: a comparison against a threshold is a decision, so the GPU's counts must EQUAL these wherever the two bracketing counts
agree -- and the seeds below are chosen so that they agree in every case (asserted in tests/test_level_host.py).

eps, the bound on |q_gpu - q_here|, is the sum of two derived bounds on the error of q against exact arithmetic (u = 2^-53, V = max(R, max |x - o|),
every p and q is a weighted mean of the v's, so at most V):

  here (sequential):  each step p = g p + a v, q = g q + a p costs at most 3 roundings of values <= V for p and 3 for q.  An error injected into p
    at sample i' reaches q_i multiplied by (i - i') a g^(i - i'), one injected into q by g^(i - i'); both series sum to at most 1 / (1 - g)
    <= tc fs + 1.  That is 6 (tc fs + 1) u V.  g itself carries up to 2 u of relative error (exp, then 1 - g), and |dq / dg| <= V / (1 - g):
    another 2 (tc fs + 1) u V.  Together  eps_seq = 8 (tc fs + 1) u V.
  the kernels (csrc/level.hip):  every sample is run by the same sequential steps with the same g (eps_seq again: the steps before a thread's own
    run are those of the zero-state runs of the threads and tiles in front of it), plus the compositions c = M^n c1 + c2 that carry the state to
    the thread.  One composition is three fused multiply-adds (3 roundings of values <= V) with two host constants of relative error <= 1.01 u
    (formed in extended precision, rounded once) multiplying values <= V and V / e: at most 6 u V, and it reaches q multiplied by at most 1.  The
    state in front of a thread depends on at most 255 compositions of the scan inside its tile, and on the chain over the tiles in front: each
    chain step adds one composition and that tile's 255, and an error injected k tiles back reaches q multiplied by at most g^(k T) (1 + k T a),
    a series that sums to at most 2 / (1 - g^T).  Together  eps_ker = eps_seq + 6 u V (255 + 256 * 2 / (1 - g^T)), times 1.01 for the second order.
"""
import math

import numpy as np

U = 2.0 ** -53
BELOW, ABOVE, EDGE, UNDEFINED = 1, 2, 4, 8


def eps_seq(fs, tc, V):
    return 8.0 * (tc * fs + 1.0) * U * V


def eps_kernel(fs, tc, V, T):
    g = math.exp(-1.0 / (fs * tc))
    return 1.01 * (eps_seq(fs, tc, V) + 6.0 * U * V * (255.0 + 256.0 * 2.0 / (1.0 - g ** T)))


def eps_offset(n, V, T):
    """the row mean o is a fixed-order double sum on the GPU (16 terms per thread, a tree of 8 levels, a tree over the tiles: at most 32 + tiles
    additions deep) and an exact sum here: |o_gpu - o_here| <= (32 + tiles) u mean |x| <= (32 + tiles) u V.  It moves every v = |x - o| and, under
    the peak rule R = max |x| + |o|, every threshold by at most that much."""
    return 2.0 * (32.0 + math.ceil(n / T)) * U * V


def eps_total(fs, tc, V, T, n=0):
    return eps_seq(fs, tc, V) + eps_kernel(fs, tc, V, T) + eps_offset(n, V, T)


def envelope(x, o, fs, tc):
    """q_i of the definition, a plain loop in float64"""
    g = math.exp(-1.0 / (fs * tc))
    a = 1.0 - g
    q_out = np.empty(len(x), dtype=np.float64)
    p = q = 0.0
    xs = np.asarray(x, dtype=np.float64)
    for i in range(len(xs)):
        v = abs(float(xs[i]) - o)
        p = g * p + a * v
        q = g * q + a * p
        q_out[i] = q
    return q_out


def counts_of(q, thresholds, hang):
    """a_j = #{i : some i' in [max(0, i - I), i] has q_i' >= c_j}, per threshold by a running count of the exceedances inside the window"""
    n = len(q)
    out = []
    for c in thresholds:
        over = (q >= c).astype(np.int64)
        cs = np.concatenate([[0], np.cumsum(over)])
        lo = np.maximum(np.arange(n) - hang, 0)
        inside = cs[np.arange(n) + 1] - cs[lo]
        out.append(int(np.count_nonzero(inside > 0)))
    return out


def counts_p56(q, thresholds, hang):
    """a direct transcription of the P.56 hangover-counter loop: one counter per threshold, started at I"""
    a = [0] * len(thresholds)
    h = [hang] * len(thresholds)
    for qi in q:
        for j, c in enumerate(thresholds):
            if qi >= c:
                a[j] += 1
                h[j] = 0
            elif h[j] < hang:
                a[j] += 1
                h[j] += 1
            else:
                break
    return a


def finish(a, sq, n, R, margin):
    nan = float("nan")
    if n < 1 or not np.isfinite(sq) or sq <= 0.0:
        return dict(level_db=nan, activity=nan, rms_db=nan, flags=UNDEFINED, js=None)
    rms_db = 10.0 * np.log10(sq / n)
    A = [10.0 * np.log10(sq / v) if v > 0 else nan for v in a]
    D = [A[j] - 20.0 * np.log10(R * 2.0 ** (j - 15)) if a[j] > 0 else -np.inf for j in range(16)]
    js = None
    for j in range(16):
        if D[j] <= margin:
            js = j
            break
    cond = 0.0                                         # |d level / d (a common shift of every A)| - 1, for the tolerance
    if js is None:
        level, flags = A[15], ABOVE
    elif js == 0:
        if a[0] == 0:
            return dict(level_db=nan, activity=nan, rms_db=rms_db, flags=BELOW | UNDEFINED, js=0)
        level, flags = A[0], BELOW
    elif a[js] == 0:
        level, flags = A[js - 1], EDGE
    else:
        t = (D[js - 1] - margin) / (D[js - 1] - D[js])
        level, flags = A[js - 1] + t * (A[js] - A[js - 1]), 0
        cond = abs(A[js] - A[js - 1]) / (D[js - 1] - D[js])
    scale = max([1.0, abs(margin)] + [abs(v) for v in A + D if np.isfinite(v)])
    return dict(level_db=float(level), activity=float(10.0 ** ((rms_db - level) / 10.0)), rms_db=float(rms_db), flags=flags, js=js, cond=cond, scale=scale)


def level_ref(x, fs, R=None, remove_mean=True, tc=0.03, hang_s=0.2, margin=15.9, T=4096):
    """the whole definition for one row x (its n valid samples).  R None: the peak rule of ``speech_level`` (max |x| + |mean|)."""
    x = np.asarray(x)
    n = len(x)
    hang = int(math.floor(hang_s * fs + 0.5))
    xs = x.astype(np.float64)
    if n == 0 or not np.all(np.isfinite(xs)):
        return dict(n=n, counts=None, flags=UNDEFINED, level_db=float("nan"), activity=float("nan"), rms_db=float("nan"), sq=float("nan"), hang=hang)
    o = math.fsum(xs.tolist()) / n if remove_mean else 0.0
    peak = float(np.max(np.abs(xs))) + abs(o)
    if R is None:
        R = peak
    sq = math.fsum(((xs - o) ** 2).tolist())
    if not R > 0.0 or sq == 0.0:
        return dict(n=n, counts=None, flags=UNDEFINED, level_db=float("nan"), activity=float("nan"), rms_db=float("nan"), sq=sq, hang=hang, o=o, R=R)
    assert float(np.mean(np.abs(xs))) <= 2.0 * math.sqrt(sq / n), "tol_sq_rel assumes mean |x| <= 2 rms(x - o)"
    q = envelope(x, o, fs, tc)
    V = max(R, float(np.max(np.abs(xs - o))))
    eps = eps_total(fs, tc, V, T, n)
    thr = [R * 2.0 ** (j - 15) for j in range(16)]
    res = finish(counts_of(q, thr, hang), sq, n, R, margin)
    res.update(n=n, o=o, R=R, sq=sq, q=q, hang=hang, eps=eps, thresholds=thr, counts=counts_of(q, thr, hang),
               counts_up=counts_of(q, [c + eps for c in thr], hang), counts_down=counts_of(q, [c - eps for c in thr], hang))
    return res


# ---- tolerances, derived ------------------------------------------------------------------------------------------------
def tol_sq_rel(n, T):
    """sq on the GPU: (x - o) rounded, squared (3 u), summed over 16 samples of a thread, a tree of 8 levels over the threads and a chain over the
    row's tiles: a relative error of at most (3 + 16 + 8 + tiles) u on a sum of non-negative terms; the restatement's fsum adds 4 u.  The two
    offsets differ by d <= (32 + tiles) u mean |x| (eps_offset), which moves sq by at most 2 d sum |x - o| <= 2 d n rms(x - o): relatively
    2 d / rms(x - o) <= 4 (32 + tiles) u for rows with mean |x| <= 2 rms(x - o), which ``level_ref`` asserts of every row it is given."""
    tiles = math.ceil(n / T)
    return (31.0 + tiles + 4.0 * (32.0 + tiles)) * U


def tol_level(res, T):
    """|level_db_gpu - level_db_here| with equal counts: every A and D moves by (10 / ln 10) rel(sq) together, which the interpolation passes on
    multiplied by 1 + |A_j* - A_j*-1| / (D_j*-1 - D_j*); each side adds at most 16 roundings of values at most `scale`"""
    return (1.0 + res["cond"]) * (10.0 / math.log(10.0) * tol_sq_rel(res["n"], T) + 32.0 * U * res["scale"])


def tol_activity(res, T):
    """activity = 10^((rms_db - level_db) / 10): its relative error is (ln 10 / 10) times the error of the exponent's numerator, plus 4 roundings"""
    d = tol_level(res, T) + 10.0 / math.log(10.0) * tol_sq_rel(res["n"], T) + 8.0 * U * res["scale"]
    return res["activity"] * (math.log(10.0) / 10.0 * d + 4.0 * U)


# ---- signals -----------------------------------------------------------------------------------------------------------------------------------
def speechlike(seed, n, fs, pause=0.4, amp=0.3):
    """noise bursts of random length and loudness with pauses of low noise between them, fp32"""
    rs = np.random.RandomState(seed)
    x = 1e-3 * amp * rs.standard_normal(n)
    i = 0
    while i < n:
        on = int(fs * rs.uniform(0.05, 0.6))
        off = int(fs * rs.uniform(0.05, 0.6) * pause / max(1.0 - pause, 1e-3))
        lvl = amp * 10.0 ** (rs.uniform(-12.0, 0.0) / 20.0)
        m = min(on, n - i)
        x[i:i + m] += lvl * rs.standard_normal(m) * np.hanning(m + 2)[1:-1] ** 0.25
        i += on + off
    return x.astype(np.float32)


def length_cases(T, Tc, hang):
    return sorted({1, 2, hang, hang + 1, T - 1, T, T + 1, 2 * T + 3, Tc - 1, Tc, Tc + 1})


def gpu_cases(T, Tc):
    """name -> (fs, rows, remove_mean): every seeded case of tests/test_hip_level.py that is compared count for count"""
    cases = {}
    fs = 1000
    cases["lengths_1k"] = (fs, [speechlike(100 + k, n, fs) for k, n in enumerate(length_cases(T, Tc, 200))], False)
    cases["long_8k"] = (8000, [speechlike(7, 40 * T + 17, 8000)], True)
    cases["hang_over_tile_48k"] = (48000, [speechlike(11, 3 * T + 5, 48000), speechlike(12, 9601, 48000), speechlike(13, 9600, 48000)], True)
    cases["batch_2k"] = (2000, [speechlike(21, 2 * T + 3, 2000), speechlike(22, T + 1, 2000, pause=0.7), speechlike(23, 3 * T - 7, 2000, pause=0.2)], True)
    return cases


def half_peak_row(T, Tc):
    """(fs, row): a row of ``batch_2k`` scaled so that its peak is exactly 0.5, for the comparison of full scale 1 with the peak rule"""
    fs, rows, _ = gpu_cases(T, Tc)["batch_2k"]
    x = rows[1].astype(np.float64)
    x = (x * (0.5 / np.abs(x).max())).astype(np.float32)
    x[np.argmax(np.abs(x))] = 0.5
    assert np.abs(x).max() == 0.5
    return fs, x
