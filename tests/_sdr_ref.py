"""Float64 restatement of the projection SDR for the tests of buddy_amd/utils/sdr.py and csrc/sdr.hip.  It reaches the value by
other routes than the kernel, which runs a Levinson recursion: the dense Toeplitz matrix through ``numpy.linalg.solve`` (LU; the reference value),
through a Cholesky factorisation, and through scipy's own ``solve_toeplitz``; and, for small sizes, the time-domain construction of ``bss_eval`` -- the
matrix of zero-padded delayed copies of the clean signal, a least-squares projection, the energy ratio.  The inputs the GPU test uses are made here,
once, and never modified."""
import csv
import functools

import numpy as np
import scipy.linalg
import scipy.signal

LOADING = 1e-9
ROUTES = ("lu", "cholesky", "toeplitz")
FLOOR = 1e-12                                        # the residual is floored at FLOOR * ee


def products(e, x, N, dtype=np.float64):
    """r[k] = sum_t x[t] x[t + k], d[k] = sum_t e[t + k] x[t] for k < N (zero where there is no term), ee = sum e^2: explicit sums in ``dtype``"""
    e, x = np.asarray(e, dtype=dtype), np.asarray(x, dtype=dtype)
    n = len(x)
    r, d = np.zeros(N, dtype=dtype), np.zeros(N, dtype=dtype)
    for k in range(min(N, n)):
        r[k] = np.dot(x[:n - k], x[k:])
        d[k] = np.dot(x[:n - k], e[k:])
    return r, d, np.dot(e, e)


def product_bounds(e, x, N):
    """the written bound of buddy_sdr_products per lag: (n + 4) 2^-53 sum |.||.| -> (bound of r, bound of d, bound of ee)"""
    br, bd, bee = products(np.abs(e), np.abs(x), N, np.longdouble)
    s = (len(x) + 4) * 2.0 ** -53
    return np.asarray(s * br, np.float64), np.asarray(s * bd, np.float64), float(s * bee)


def toeplitz(r, m, loading=LOADING):
    t = np.array(r[:m], dtype=np.float64)
    t[0] *= 1.0 + loading
    return scipy.linalg.toeplitz(t)


def solve(route, r, d, m, loading=LOADING):
    """h_m = R_m^-1 d[:m] by one of ``ROUTES``"""
    rhs = np.asarray(d[:m], dtype=np.float64)
    if route == "lu":
        return np.linalg.solve(toeplitz(r, m, loading), rhs)
    if route == "cholesky":
        return scipy.linalg.cho_solve(scipy.linalg.cho_factor(toeplitz(r, m, loading)), rhs)
    if route == "toeplitz":
        t = np.array(r[:m], dtype=np.float64)
        t[0] *= 1.0 + loading
        return scipy.linalg.solve_toeplitz(t, rhs)
    raise ValueError(route)


def value(p, ee):
    return 10.0 * np.log10(p / max(ee - p, FLOOR * ee))


def sdr(route, r, d, ee, orders, loading=LOADING):
    """-> (SDR_m in dB, p_m) per order as two float64 arrays, and h of the largest order"""
    out, ps, h = [], [], None
    for m in orders:
        h = solve(route, r, d, m, loading)
        p = float(h @ np.asarray(d[:m], dtype=np.float64))
        ps.append(p)
        out.append(value(p, ee))
    return np.array(out), np.array(ps), h


def evaluate(e, x, orders, loading=LOADING, route="lu"):
    """the whole measure of one pair at 16 kHz -> (SDR per order, p per order, h of the largest order)"""
    r, d, ee = products(e, x, max(orders))
    return sdr(route, r, d, float(ee), orders, loading)


def time_domain(e, x, m):
    """bss_eval's construction without loading: A = the (n + m - 1, m) matrix of the zero-padded copies of x delayed by 0..m - 1, s = the least-squares
    projection of the zero-padded e onto its columns; 10 log10(||s||^2 / ||e - s||^2)"""
    e, x = np.asarray(e, dtype=np.float64), np.asarray(x, dtype=np.float64)
    n = len(x)
    A = np.zeros((n + m - 1, m))
    for k in range(m):
        A[k:k + n, k] = x
    ep = np.concatenate([e, np.zeros(m - 1)])
    h = np.linalg.lstsq(A, ep, rcond=None)[0]
    s = A @ h
    return 10.0 * np.log10(np.dot(s, s) / np.dot(ep - s, ep - s)), h


# ---- the inputs of the solve tests: made once, read-only --------------------------------------------------------------------------------------
N_SOLVE = 32000                                      # 2 s at 16 kHz
ORDERS = (1, 2, 63, 64, 65, 512, 2048)


def decaying_response(seed, taps=3000, t60=0.3, fs=16000):
    rs = np.random.RandomState(seed)
    g = rs.standard_normal(taps) * np.exp(-6.908 * np.arange(taps) / (t60 * fs))
    g[0] = 1.0
    return g


def band_noise(seed, n, edge):
    """white noise band-limited to ``edge`` of Nyquist (255-tap Kaiser low-pass, about -100 dB behind the edge) plus white noise 60 dB below it"""
    rs = np.random.RandomState(seed)
    w = scipy.signal.lfilter(scipy.signal.firwin(255, edge, window=("kaiser", 10.0)), 1.0, rs.standard_normal(n + 255))[255:]
    return w / np.std(w) + 1e-3 * rs.standard_normal(n)


@functools.lru_cache(maxsize=None)
def solve_pairs():
    """name -> (estimate, clean) as float32 rows of N_SOLVE samples: white noise, noise band-limited to 0.45 and to 0.25 of Nyquist, and one speech-like
    row of buddy_amd/synth.py, each through a decaying 3000-tap response with white noise 60 dB below the clean signal added"""
    from buddy_amd.synth import synth_clean
    n = N_SOLVE
    clean = {"white": np.random.RandomState(11).standard_normal(n), "band45": band_noise(12, n, 0.45), "band25": band_noise(13, n, 0.25),
             "speech": synth_clean(3, n).astype(np.float64)}
    pairs = {}
    for q, (name, x) in enumerate(clean.items()):
        x = (0.1 * x / np.std(x)).astype(np.float32)
        e = np.convolve(x.astype(np.float64), decaying_response(20 + q))[:n] + 1e-4 * np.random.RandomState(30 + q).standard_normal(n)
        e = e.astype(np.float32)
        x.setflags(write=False)
        e.setflags(write=False)
        pairs[name] = (e, x)
    return pairs


@functools.lru_cache(maxsize=None)
def solve_case(name):
    """of one pair of ``solve_pairs``: r, d, ee (float64, N = 2048) and per route (SDR, p, h at 2048) at ``ORDERS``; ``tol_db`` / ``tol_p`` / ``tol_h``: the
    largest disagreement among the routes in dB over the orders, in p relative to ee, and in h (max-norm)"""
    e, x = solve_pairs()[name]
    r, d, ee = products(e, x, ORDERS[-1])
    ee = float(ee)
    by = {route: sdr(route, r, d, ee, ORDERS) for route in ROUTES}
    pairs = [(a, b) for i, a in enumerate(ROUTES) for b in ROUTES[i + 1:]]
    case = dict(r=r, d=d, ee=ee, routes=by, sdr=by["lu"][0], p=by["lu"][1], h=by["lu"][2],
                tol_db=max(float(np.abs(by[a][0] - by[b][0]).max()) for a, b in pairs),
                tol_p=max(float(np.abs(by[a][1] - by[b][1]).max()) for a, b in pairs) / ee,
                tol_h=max(float(np.abs(by[a][2] - by[b][2]).max()) for a, b in pairs),
                cond=float(np.linalg.cond(toeplitz(r, ORDERS[-1]))))
    for v in (r, d) + tuple(a for t in by.values() for a in t):
        v.setflags(write=False)
    return case


# ---- the inputs of the known-answer tests ---------------------------------------------------------------------------------------------------------
N_KNOWN = 8000
TAPS = (1, 64, 512, 2048)
SHIFT = 5                                            # samples of the delayed and of the advanced copy


@functools.lru_cache(maxsize=None)
def known_pairs():
    """name -> (estimate, clean) float32 rows of N_KNOWN samples over one white clean signal x; ``known_fir()`` is the drawn 40-tap g:
    same: e = x;  fir40: e = g * x;  fir40_noise: e = g * x + w, w white at a drawn level;  delayed: e[t] = x[t - 5];  advanced: e[t] = x[t + 5].
    x ends in 64 zeros, so that g * x and the delayed copy end inside the row: a filtered copy cut off at the row's end is not a filtered copy"""
    rs = np.random.RandomState(41)
    x = (0.1 * rs.standard_normal(N_KNOWN)).astype(np.float32)
    x[-64:] = 0.0
    gx = np.convolve(x.astype(np.float64), known_fir())[:N_KNOWN]
    level = 10.0 ** (rs.uniform(-30.0, -10.0) / 20.0)
    zeros = np.zeros(SHIFT, np.float32)
    pairs = {"same": x.copy(), "fir40": gx.astype(np.float32), "fir40_noise": (gx + level * np.std(gx) * rs.standard_normal(N_KNOWN)).astype(np.float32),
             "delayed": np.concatenate([zeros, x[:-SHIFT]]), "advanced": np.concatenate([x[SHIFT:], zeros])}
    x.setflags(write=False)
    for e in pairs.values():
        e.setflags(write=False)
    return {name: (e, x) for name, e in pairs.items()}


@functools.lru_cache(maxsize=None)
def known_fir():
    g = np.random.RandomState(42).standard_normal(40) * np.exp(-np.arange(40) / 10.0)
    g[0] = 1.0
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def known_case(name):
    """of one pair of ``known_pairs`` at ``TAPS``: per route (SDR, p, h at 2048), and the routes' largest disagreement in dB and in h (max-norm)"""
    e, x = known_pairs()[name]
    by = {route: evaluate(e, x, TAPS, route=route) for route in ROUTES}
    pairs = [(a, b) for i, a in enumerate(ROUTES) for b in ROUTES[i + 1:]]
    return dict(routes=by, sdr=by["lu"][0], h=by["lu"][2], tol_db=max(float(np.abs(by[a][0] - by[b][0]).max()) for a, b in pairs),
                tol_h=max(float(np.abs(by[a][2] - by[b][2]).max()) for a, b in pairs))


def read_csv(path):
    """rows of a report as dicts: '' -> NaN, integers as int, other numbers as float, the file name as it is"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = []
    for r in rows:
        d = {}
        for k, v in r.items():
            if k in ("file", "value"):
                d[k] = v
            elif v == "":
                d[k] = float("nan")
            else:
                try:
                    d[k] = int(v)
                except ValueError:
                    d[k] = float(v)
        out.append(d)
    return out
