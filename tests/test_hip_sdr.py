"""GPU: the projection SDR report (csrc/sdr.hip, buddy_amd/utils/sdr.py) against the float64 restatement tests/_sdr_ref.py: the lag products alone on
ragged rows placed around the kernel's chunk and lag tile, against the same sums in long double and the entry's written bound; the Levinson kernel alone
on the restatement's r, d, ee, held to 16 times the disagreement of three float64 solvers (LU, Cholesky, scipy's solve_toeplitz); known answers through
``evaluate``; batch independence; the refused arguments; the tester writing its CSV files and the stand-alone tool reading them back.

Every comparison prints a ``sdr_accuracy:`` line (measured error, bound, the routes' disagreement): profiles/sdr_accuracy.txt is those lines."""
import functools
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sdr_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_clean, synth_rir  # noqa: E402
from buddy_amd.utils import metrics as M  # noqa: E402
from buddy_amd.utils import resample as RS  # noqa: E402
from buddy_amd.utils import sdr as S  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 12345.0
ERR_ARG = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = _lib.C


@pytest.fixture(scope="module")
def lib():
    return _lib.require_gpu()


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def padded(rows, ld, fill=np.nan):
    """rows of their own lengths -> (B, ld) float32 on the device with ``fill`` behind every row (NaN: a read past the end would show)"""
    out = np.full((len(rows), ld), fill, np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return torch.from_numpy(out).cuda()


def guarded(n, dtype, fill):
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


def split(buf, n, fill):
    """the first n words; asserts the guard words behind them are intact"""
    a = buf.cpu().numpy()
    assert np.all(a[n:] == fill), "guard words overwritten"
    return a[:n]


def ints(v):
    return (C.c_int * len(v))(*v)


def db_tolerance(tol_routes):
    """a row's tolerance in dB: 16 times the largest disagreement among the three float64 routes -- the margin covers the kernel's other summation
    order, which the routes share among themselves -- never below 1e-9 dB; a reference that disagrees with itself by more than 1e-4 dB / 16 fails"""
    tol = max(16.0 * tol_routes, 1e-9)
    assert tol <= 1e-4, f"the float64 routes disagree by {tol_routes:.2e} dB: no reference to hold a kernel to"
    return tol


# ---- 1. the lag products alone -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def product_rows(T, K):
    """rows of n = 1, 2, T - 1, T, T + 1, 3 T + 17 samples with a mean (nothing removes it), their sums in long double up to 2 K + 3 lags and the
    written bound per lag; computed once, never modified"""
    rs = np.random.RandomState(505)
    lens = (1, 2, T - 1, T, T + 1, 3 * T + 17)
    es = tuple((0.3 * rs.standard_normal(n) - 0.05).astype(np.float32) for n in lens)
    xs = tuple((0.2 * rs.standard_normal(n) + 0.1).astype(np.float32) for n in lens)
    want = tuple(R.products(e, x, 2 * K + 3, np.longdouble) for e, x in zip(es, xs))
    bound = tuple(R.product_bounds(e, x, 2 * K + 3) for e, x in zip(es, xs))
    return lens, es, xs, want, bound


@pytest.mark.parametrize("which", range(6))
def test_products_vs_long_double(lib, which):
    """r, d and ee of six ragged rows in one stride, N = 1, 2, K - 1, K, K + 1, 2 K + 3 (n < N for the short rows): every lag within the entry's own
    bound (n + 4) 2^-53 sum |.||.| of the long-double sums; lags >= n exactly 0; NaN behind every row (nothing behind lens[b] is read); guard words"""
    T, K = lib.buddy_sdr_tile(), lib.buddy_sdr_lag_tile()
    N = (1, 2, K - 1, K, K + 1, 2 * K + 3)[which]
    lens, es, xs, want, bound = product_rows(T, K)
    B, ld = len(lens), 3 * T + 40
    r, d, ee = guarded(B * N, torch.float64, SENTINEL), guarded(B * N, torch.float64, SENTINEL), guarded(B, torch.float64, SENTINEL)
    nbytes = lib.buddy_sdr_products_workspace(B, max(lens), N)
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda")
    e_d, x_d, lens_d = padded(es, ld), padded(xs, ld), dev_i32(lens)
    rc = lib.buddy_sdr_products(_lib.ptr(e_d), _lib.ptr(x_d), lens_d.data_ptr(), B, ld, N, r.data_ptr(), d.data_ptr(), ee.data_ptr(), ws.data_ptr(), nbytes,
                                _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    r, d, ee = split(r, B * N, SENTINEL).reshape(B, N), split(d, B * N, SENTINEL).reshape(B, N), split(ee, B, SENTINEL)
    worst = 0.0
    for b, n in enumerate(lens):
        (wr, wd, wee), (br, bd, bee) = want[b], bound[b]
        for got, ref, bnd, what in ((r[b], wr[:N], br[:N], "r"), (d[b], wd[:N], bd[:N], "d"), (ee[b:b + 1], np.array([wee]), np.array([bee]), "ee")):
            err = np.abs(np.asarray(got, np.longdouble) - ref).astype(np.float64)
            assert np.all(np.isfinite(got)) and np.all(err <= bnd), (what, n, N, float((err - bnd).max()))
            live = bnd > 0
            worst = max(worst, float((err[live] / bnd[live]).max()) if live.any() else 0.0)
        assert not r[b, n:].any() and not d[b, n:].any(), (n, N)                          # no term: exactly zero
    print(f"sdr_accuracy: products N {N:5d} rows {list(lens)}: largest |error| / bound {worst:.3e} (bound (n + 4) 2^-53 sum|.||.| per lag; 1 = at the bound)")


# ---- 2. the Levinson kernel alone ----------------------------------------------------------------------------------------------------------------
def run_solve(lib, r, d, ee, lens, orders, want_h=True, loading=S.LOADING):
    B, N, J = r.shape[0], r.shape[1], len(orders)
    sdr, p = guarded(B * J, torch.float64, SENTINEL), guarded(B * J, torch.float64, SENTINEL)
    flags, h = guarded(B, torch.int32, -77), guarded(B * N, torch.float64, SENTINEL)
    rd, dd, ed = (torch.from_numpy(np.array(a, dtype=np.float64)).cuda() for a in (r, d, ee))
    lens_d = dev_i32(lens)
    rc = lib.buddy_sdr_solve(rd.data_ptr(), dd.data_ptr(), ed.data_ptr(), lens_d.data_ptr(), B, N, ints(orders), J, loading, sdr.data_ptr(), p.data_ptr(),
                             flags.data_ptr(), h.data_ptr() if want_h else None, _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    hh = split(h, B * N, SENTINEL).reshape(B, N) if want_h else split(h, 0, SENTINEL)
    return split(sdr, B * J, SENTINEL).reshape(B, J), split(p, B * J, SENTINEL).reshape(B, J), split(flags, B, -77), hh


def test_solve_vs_three_float64_routes(lib):
    """orders (1, 2, 63, 64, 65, 512, 2048) at N = 2048 on the restatement's r, d, ee of four pairs in one batch -- white noise, noise band-limited to 0.45
    and to 0.25 of Nyquist, one speech-like row, each through a decaying 3000-tap response: SDR within the row's tolerance (``db_tolerance``), p within
    the same tolerance as a ratio, h within 16 times the routes' disagreement in h (max-norm)"""
    names = list(R.solve_pairs())
    cases = [R.solve_case(n) for n in names]
    r, d, ee = np.stack([c["r"] for c in cases]), np.stack([c["d"] for c in cases]), np.array([c["ee"] for c in cases])
    sdr, p, flags, h = run_solve(lib, r, d, ee, [R.N_SOLVE] * len(cases), R.ORDERS)
    fails = []
    for b, (name, c) in enumerate(zip(names, cases)):
        tol = db_tolerance(c["tol_db"])
        rel = 10.0 ** (tol / 10.0) - 1.0
        err, errp, errh = np.abs(sdr[b] - c["sdr"]).max(), np.abs(p[b] / c["p"] - 1.0).max(), np.abs(h[b] - c["h"]).max()
        print(f"sdr_accuracy: solve {name:7s} cond {c['cond']:.1e}: SDR error {err:.2e} dB (tolerance {tol:.2e}, routes {c['tol_db']:.2e}); p error {errp:.2e} "
              f"relative (tolerance {rel:.2e}); h error {errh:.2e} (tolerance {16.0 * c['tol_h']:.2e}, routes {c['tol_h']:.2e}); flags {flags[b]}")
        if not (err <= tol and errp <= rel and errh <= 16.0 * c["tol_h"] and flags[b] == 1):
            fails.append(name)
    assert not fails, fails
    # without h, and the smallest system
    sdr1, p1, flags1, _ = run_solve(lib, r[:, :1], d[:, :1], ee, [R.N_SOLVE] * len(cases), (1,), want_h=False)
    assert np.array_equal(sdr1[:, 0], sdr[:, 0]) and np.array_equal(p1[:, 0], p[:, 0]) and flags1.tolist() == [1] * len(cases)


def test_solve_flags(lib):
    """a pivot that is not positive (r is no autocorrelation) leaves the row undefined: NaN, zeros in h, bit 0 clear; a pivot below 2^-26 sets bit 2 and
    the value is reported; the row next to them is what it is alone"""
    c = R.solve_case("white")
    r0, d = c["r"][0], c["d"][:2]
    r = np.array([[r0, c["r"][1]],
                  [r0, 1.5 * r0],                                                         # |eps_f| > 1 at the one step
                  [r0, r0 * (1.0 + S.LOADING) * (1.0 - 2.0 ** -29)]])                     # 1 - eps_f^2 = about 2^-28
    sdr, p, flags, h = run_solve(lib, r, np.stack([d] * 3), np.full(3, c["ee"]), [R.N_SOLVE] * 3, (1, 2))
    alone = run_solve(lib, r[:1], d[None], np.full(1, c["ee"]), [R.N_SOLVE], (1, 2))
    assert flags[0] == 1 and alone[2][0] == 1 and all(np.array_equal(a[0], b[0]) for a, b in zip((sdr, p, h), (alone[0], alone[1], alone[3])))
    assert flags[1] & 1 == 0 and np.isnan(sdr[1]).all() and np.isnan(p[1]).all() and not h[1].any()
    assert flags[2] & 5 == 5 and np.isfinite(sdr[2]).all() and sdr[2, 0] == sdr[0, 0]


# ---- 3. known answers, through evaluate -------------------------------------------------------------------------------------------------------------
def dev_pair(name):
    e, x = R.known_pairs()[name]
    return torch.from_numpy(e.copy())[None].cuda(), torch.from_numpy(x.copy())[None].cuda()


def at_ceiling(v):
    """about -10 log10(lambda) = 90 dB: the residual there is lambda ee, a difference of nearly equal numbers, and moves with their last bits"""
    return bool(np.all(np.abs(np.asarray(v) - 90.0) < 0.5))


def test_identical_pair():
    e, x = dev_pair("same")
    ev = S.evaluate(e, x, 16000, filters=True)
    h = ev.filters[0].numpy()
    print(f"sdr_accuracy: e = x: SDR {ev.values[0].tolist()} dB at {list(ev.taps)} (about 90), |h - delta / (1 + lambda)| {max(abs(h[0] - 1 / (1 + S.LOADING)), np.abs(h[1:]).max()):.2e}")
    assert ev.taps == S.TAPS and at_ceiling(ev.values[0]) and int(ev.flags[0]) == S.DEFINED | S.CEILING and int(ev.samples[0]) == R.N_KNOWN
    assert abs(h[0] - 1.0 / (1.0 + S.LOADING)) < 1e-9 and np.abs(h[1:]).max() < 1e-9 and h.shape == (2048,)


def test_filtered_copy():
    """e = g * x with a drawn 40-tap g: orders >= 64 sit at the ceiling and h[:40] is g -- within 16 times the routes' disagreement of the restatement's
    h, which itself is within 1e-7 ||g|| of g (the loading moves h by about lambda cond(R) ||g||, below 1e-8 ||g|| for a white x; e rounded to fp32 adds
    noise 2^-24 below it, of which 2048 taps over 8000 samples pick up about 2^-24 sqrt(2048 / 8000) ||g||) -- and orders < 40 are strictly lower"""
    e, x = dev_pair("fir40")
    g, c = R.known_fir(), R.known_case("fir40")
    ev = S.evaluate(e, x, 16000, values=(1, 20, 39, 64, 512, 2048), filters=True)
    v, h = ev.values[0].numpy(), ev.filters[0].numpy()
    errh, ref = np.abs(h - c["h"]).max(), np.abs(c["h"][:40] - g).max()
    print(f"sdr_accuracy: e = g * x: SDR {np.round(v, 4).tolist()} dB at {list(ev.taps)}; |h - restatement| {errh:.2e} (tolerance {16 * c['tol_h']:.2e}, routes "
          f"{c['tol_h']:.2e}); |restatement - g| {ref:.2e} (bound {1e-7 * np.linalg.norm(g):.2e})")
    assert at_ceiling(v[3:]) and int(ev.flags[0]) == S.DEFINED | S.CEILING
    assert errh <= 16.0 * c["tol_h"] and ref <= 1e-7 * np.linalg.norm(g) and np.abs(c["h"][40:]).max() <= 1e-7 * np.linalg.norm(g)
    assert v[0] < v[1] < v[2] < v[3] - 10.0


def test_filtered_copy_in_noise():
    e, x = dev_pair("fir40_noise")
    c = R.known_case("fir40_noise")
    ev = S.evaluate(e, x, 16000)
    tol = db_tolerance(c["tol_db"])
    err = np.abs(ev.values[0].numpy() - c["sdr"])
    print(f"sdr_accuracy: e = g * x + w: SDR {ev.values[0].tolist()} dB, error {err.tolist()} dB (tolerance {tol:.2e}, routes {c['tol_db']:.2e})")
    assert err[2] <= tol and np.all(err <= tol) and int(ev.flags[0]) == S.DEFINED and 20.0 < c["sdr"][2] < 40.0


def test_delayed_and_advanced_copies():
    """e[t] = x[t - 5] is inside the span from order 6 on; e[t] = x[t + 5] is not causal: low at every order, and at the ceiling once the pair is aligned"""
    e, x = dev_pair("delayed")
    ev = S.evaluate(e, x, 16000, values=(1, 5, 6, 64))
    v = ev.values[0].numpy()
    assert v[0] < 0.0 and v[1] < 0.0 and at_ceiling(v[2:]) and int(ev.flags[0]) == S.DEFINED | S.CEILING
    e, x = dev_pair("advanced")
    ev = S.evaluate(e, x, 16000)
    al = S.evaluate(e, x, 16000, align=50)
    print(f"sdr_accuracy: delayed copy {np.round(v, 4).tolist()} dB at [1, 5, 6, 64]; advanced copy {np.round(ev.values[0].numpy(), 4).tolist()} dB, aligned "
          f"{al.values[0].tolist()} dB at {list(S.TAPS)}")
    assert np.all(ev.values[0].numpy() < 0.0) and int(ev.flags[0]) == S.DEFINED and ev.alignment is None
    assert at_ceiling(al.values[0]) and int(al.alignment.lag[0]) == -R.SHIFT and int(al.samples[0]) == R.N_KNOWN - R.SHIFT


def test_undefined_rows():
    """an all-zero clean row, an all-zero estimate, a NaN sample in either signal and n = 1: NaN at every order, bit 0 clear, zeros for the filter; the
    defined rows between them are bit for bit what they are alone"""
    e0, x0 = (a.copy() for a in R.known_pairs()["fir40_noise"])
    n = len(x0)
    zero, nan_e, nan_x = np.zeros(n, np.float32), e0.copy(), x0.copy()
    nan_e[n // 2], nan_x[17] = np.nan, np.nan
    es, xs, lens = [e0, e0, zero, nan_e, e0, e0, e0], [x0, zero, x0, x0, nan_x, x0, x0], [n, n, n, n, n, 1, n - 3]
    ev = S.evaluate(torch.from_numpy(np.stack(es)).cuda(), torch.from_numpy(np.stack(xs)).cuda(), 16000, lens=lens, filters=True)
    for b in (1, 2, 3, 4, 5):
        assert int(ev.flags[b]) & S.DEFINED == 0 and torch.isnan(ev.values[b]).all() and not ev.filters[b].any(), b
    for b in (0, 6):
        one = S.evaluate(torch.from_numpy(es[b][None]).cuda(), torch.from_numpy(xs[b][None]).cuda(), 16000, lens=[lens[b]], filters=True)
        assert int(ev.flags[b]) == int(one.flags[0]) == S.DEFINED and torch.equal(ev.values[b], one.values[0]) and torch.equal(ev.filters[b], one.filters[0]), b


def test_order_one_vs_pair_moments(lib):
    """on zero-mean rows, order 1 is the SI-SDR of buddy_pair_moments (a scale, means removed there and absent here) but for the loading: p_1 =
    <e,x>^2 / (r0 (1 + lambda)) moves the value by -(10 / ln 10) lambda (1 + 10^(SI-SDR / 10)) dB to first order.  Allowed: twice that, plus 1e-9 dB
    for the two kernels' rounding and the rows' residual means (below 2^-24 of their rms, squared in the energies)"""
    rows = []
    for e, x in R.solve_pairs().values():
        rows.append(((e - np.float64(e).mean()).astype(np.float32), (x - np.float64(x).mean()).astype(np.float32)))
    e, x = (torch.from_numpy(np.stack([r[k] for r in rows])).cuda() for k in (0, 1))
    B, L = e.shape
    mom, fl, lens_d = torch.empty(B, 4, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"), dev_i32([L] * B)
    _lib.check(lib.buddy_pair_moments(_lib.ptr(e), _lib.ptr(x), lens_d.data_ptr(), B, L, mom.data_ptr(), fl.data_ptr(), _lib.stream_ptr()))
    si = mom[:, 3].cpu().numpy()
    got = S.evaluate(e, x, 16000, values=(1,)).values[:, 0].numpy()
    shift = (10.0 / math.log(10.0)) * S.LOADING * (1.0 + 10.0 ** (si / 10.0))
    print(f"sdr_accuracy: order 1 against SI-SDR {si.tolist()} dB: differs by {(got - si).tolist()} dB (the loading's effect {(-shift).tolist()})")
    assert np.all(np.abs(got - si) <= 2.0 * shift + 1e-9)


def test_rate_48k_is_the_resampled_pair():
    rs = np.random.RandomState(48)
    x = torch.from_numpy((0.1 * rs.standard_normal((2, 9000))).astype(np.float32)).cuda()
    e = (0.8 * x + 0.3 * torch.roll(x, 7, 1)).contiguous()
    a = S.evaluate(e, x, 48000, filters=True)
    b = S.evaluate(RS.resample(e, 48000, 16000), RS.resample(x, 48000, 16000), 16000, filters=True)
    assert torch.equal(a.values, b.values) and torch.equal(a.filters, b.filters) and torch.equal(a.flags, b.flags) and torch.isfinite(a.values).all()
    assert a.samples.tolist() == [9000, 9000] and b.samples.tolist() == [3000, 3000]
    with pytest.raises(ValueError, match="16000"):
        S.evaluate(e, x, 8000)


# ---- 4. batch independence ---------------------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_their_batch(lib):
    T = lib.buddy_sdr_tile()
    rs = np.random.RandomState(77)
    lens = [3 * T + 100, T + 1, 700, 2 * T, 3 * T + 100]
    xs = [(0.1 * rs.standard_normal(n)).astype(np.float32) for n in lens]
    es = [(np.convolve(x, R.decaying_response(60 + b, 300, 0.02))[:len(x)] + 0.01 * rs.standard_normal(len(x))).astype(np.float32) for b, x in enumerate(xs)]
    ld = max(lens) + 9
    ev = S.evaluate(padded(es, ld), padded(xs, ld), 16000, lens=lens, filters=True)
    assert ev.flags.tolist() == [1] * 5 and torch.isfinite(ev.values).all()
    for b, n in enumerate(lens):
        one = S.evaluate(padded(es[b:b + 1], n), padded(xs[b:b + 1], n), 16000, filters=True)
        assert torch.equal(ev.values[b], one.values[0]) and torch.equal(ev.filters[b], one.filters[0]) and int(one.flags[0]) == 1, b


# ---- 5. the refused arguments ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(lib):
    """every BUDDY_ERR_ARG case of the two entries: the message is set and nothing is launched (the outputs keep their sentinel)"""
    B, n, N = 2, 100, 8
    e, x, lens = torch.zeros(B, n, device="cuda"), torch.zeros(B, n, device="cuda"), dev_i32([n, n])
    r, d, ee = (torch.full((k,), SENTINEL, dtype=torch.float64, device="cuda") for k in (B * N, B * N, B))
    nbytes = lib.buddy_sdr_products_workspace(B, n, N)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    st = _lib.stream_ptr()
    good = [_lib.ptr(e), _lib.ptr(x), lens.data_ptr(), B, n, N, r.data_ptr(), d.data_ptr(), ee.data_ptr(), ws.data_ptr(), nbytes, st]
    empty, long, huge = dev_i32([n, 0]), dev_i32([n, n + 1]), dev_i32([n, 2 ** 30 + 1])  # a length outside 1..2^30, or beyond the stride
    bad = [(i, None) for i in (0, 1, 2, 6, 7, 8, 9)] + [(3, 0), (3, 65536), (4, n - 1), (5, 0), (5, 2049), (10, nbytes - 8), (2, empty.data_ptr()),
                                                          (2, long.data_ptr()), (2, huge.data_ptr())]
    for i, v in bad:
        args = list(good)
        args[i] = v
        assert lib.buddy_sdr_products(*args) == ERR_ARG and b"buddy_sdr_products" in lib.buddy_last_error(), (i, v)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (r, d, ee))
    assert lib.buddy_sdr_products(*good) == 0 and lib.buddy_sdr_products_workspace(B, 2 ** 30 + 1, N) == -1

    J = 3
    sdr, p = (torch.full((B * J,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2))
    flags, h = torch.full((B,), -77, dtype=torch.int32, device="cuda"), torch.full((B * N,), SENTINEL, dtype=torch.float64, device="cuda")
    good = [r.data_ptr(), d.data_ptr(), ee.data_ptr(), lens.data_ptr(), B, N, ints([1, 2, 8]), J, 1e-9, sdr.data_ptr(), p.data_ptr(), flags.data_ptr(), h.data_ptr(), st]
    bad = [(i, None) for i in (0, 1, 2, 3, 6, 9, 10, 11)] + [(4, 0), (4, 65536), (5, 0), (5, 2049), (7, 0), (6, ints([1, 2, 9])), (6, ints([0, 2, 8])),
                                                             (6, ints([1, 1, 8])), (6, ints([2, 1, 8])), (8, -1e-9), (8, float("nan")),
                                                             (3, empty.data_ptr()), (3, huge.data_ptr())]
    for i, v in bad:
        args = list(good)
        args[i] = v
        assert lib.buddy_sdr_solve(*args) == ERR_ARG and b"buddy_sdr_solve" in lib.buddy_last_error(), (i, v)
    args = list(good)
    args[6], args[7] = ints(list(range(1, 10))), 9                                        # more than 8 orders
    assert lib.buddy_sdr_solve(*args) == ERR_ARG and b"J must be" in lib.buddy_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (sdr, p, h)) and bool((flags == -77).all())
    args = list(good)
    args[12] = None                                                                       # h may be NULL
    assert lib.buddy_sdr_solve(*args) == 0 and lib.buddy_sdr_solve(*good) == 0
    torch.cuda.synchronize()
    assert flags.tolist() == [0, 0] and bool(torch.isnan(sdr).all())                      # the all-zero rows are not defined
    with pytest.raises(ValueError, match="taps"):
        S.evaluate(e, x, 16000, values=(0, 1))


# ---- 6. the tester and the tool ------------------------------------------------------------------------------------------------------------------
SMALL = ["tester.sampling_params.T=3", "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "network.nf=32", "tester.noise.generator=philox",
         "tester.sub_batches=1", "+gpu=0", "tester.overriden_name=run", "+allow_random_init=true"]
COLUMNS = ["file"] + [f"sdr{m}_{k}" for m in S.TAPS for k in ("in", "out", "delta")] + ["flags_in", "flags_out", "samples"]
LAGS = ["lag_in", "lag_out", "lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out", "align_flags_in", "align_flags_out"]


def _run_tester(tmp, tag, extra):
    """informed mode, the nf = 32 fixture network, two utterances of one second (the fixture of the other reports' tests)"""
    import test as cli
    data = os.path.join(tmp, "data")
    if not os.path.exists(data):
        for u, n_rir in enumerate((3000, 2400)):
            for sub, x in (("clean", synth_clean(u, 16000)), ("rir", np.concatenate([np.zeros(37, np.float32), synth_rir(u, n_rir)]))):
                d = os.path.join(data, sub, "p001")
                os.makedirs(d, exist_ok=True)
                wavfile.write(os.path.join(d, f"p001_{u:03d}.wav"), 16000, x.astype(np.float32))
    out = os.path.join(tmp, tag)
    torch.manual_seed(0)                                      # +allow_random_init draws the network from torch's generator: the same weights in every run
    t = cli.main(["--config-name=conf_VCTK.yaml", "tester=informed_dereverberation_DPS", *SMALL, f"model_dir={out}", f"dset.test.path={data}",
                  "dset.test.num_examples=2", "+batch_size=2", *extra])
    return t, os.path.join(out, "run", "informed_dereverberation", "VCTK_16k_4s_time")


def _files(base):
    return {os.path.relpath(os.path.join(dp, f), base): open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(base) for f in fs
            if f.endswith((".csv", ".wav"))}


def _same(a, b):
    return (isinstance(a, float) and math.isnan(a) and math.isnan(b)) or a == b


def _tool():
    spec = importlib.util.spec_from_file_location("buddy_tools_sdr", os.path.join(ROOT, "tools", "sdr.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tester_sdr_report_and_tool(tmp_path):
    """with tester.sdr.use the run writes sdr.csv and sdr_summary.csv with the documented columns, whose rows equal evaluate on the written wavs; with
    use=false, or with no sdr block at all, neither file exists and every other csv (metrics.csv was asked for) and wav is the same, byte for byte;
    tools/sdr.py on the mode directory gives the tester's rows, on two folders the _out columns alone, and --write-filters the fitted filters"""
    tmp = str(tmp_path)
    t_on, on = _run_tester(tmp, "on", ["tester.metrics.use=true", "tester.sdr.use=true"])
    rows = R.read_csv(os.path.join(on, "sdr.csv"))
    assert list(rows[0]) == COLUMNS == list(t_on.sdr_report[0]) and [r["file"] for r in rows] == [r["file"] for r in t_on.sdr_report] and len(rows) == 2
    names = [r["file"] for r in rows]
    rd = {s: torch.from_numpy(np.stack([wavfile.read(os.path.join(on, s, n + ".wav"))[1] for n in names])).cuda() for s in ("original", "degraded", "reconstructed")}
    inp, out = S.evaluate(rd["degraded"], rd["original"], 16000), S.evaluate(rd["reconstructed"], rd["original"], 16000, filters=True)
    for b, r in enumerate(rows):
        assert r["samples"] == 16000 and r["flags_in"] == int(inp.flags[b]) and r["flags_out"] == int(out.flags[b]) and r["flags_out"] & 1
        for q, m in enumerate(out.names):
            assert _same(r[m + "_in"], float(inp.values[b, q])) and _same(r[m + "_out"], float(out.values[b, q])) and math.isfinite(r[m + "_out"]), (b, m)
            assert _same(r[m + "_delta"], r[m + "_out"] - r[m + "_in"])
        assert r["sdr1_in"] <= r["sdr64_in"] <= r["sdr512_in"] <= r["sdr2048_in"] and r["sdr2048_in"] > r["sdr1_in"] + 3.0      # a reverberant input
    summ = R.read_csv(os.path.join(on, "sdr_summary.csv"))
    assert [s["value"] for s in summ] == COLUMNS[1:13]
    for s in summ:
        v = np.array([r[s["value"]] for r in rows])
        assert s["n"] == 2 and s["mean"] == float(np.mean(v)) and s["median"] == float(np.median(v)) and s["std"] == float(np.std(v)), s
    _, off = _run_tester(tmp, "off", ["tester.metrics.use=true", "tester.sdr.use=false"])
    _, bare = _run_tester(tmp, "bare", ["tester.metrics.use=true", "tester.sdr=null"])
    f_on, f_off, f_bare = _files(on), _files(off), _files(bare)
    assert f_off == f_bare and "metrics.csv" in f_off and not [f for f in f_off if "sdr" in os.path.basename(f)]
    assert sorted(set(f_on) - set(f_off)) == ["sdr.csv", "sdr_summary.csv"]
    assert all(f_on[f] == data for f, data in f_off.items())                             # the other reports and every wav do not depend on this one
    # the tool, in a child process: the mode directory gives the tester's rows
    saved = open(os.path.join(on, "sdr.csv")).read()
    os.remove(os.path.join(on, "sdr.csv"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sdr.py"), on], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "sdr2048_out" in p.stdout
    again = open(os.path.join(on, "sdr.csv")).read()         # the same header and lines, the files in name order
    assert again.splitlines()[0] == saved.splitlines()[0] and sorted(again.splitlines()[1:]) == sorted(saved.splitlines()[1:]) == again.splitlines()[1:]
    # two folders, no input, other taps: the _in and _delta columns stay empty; the fitted filters are written as wavs
    tool = _tool()
    outd, fdir = str(tmp_path / "scored"), str(tmp_path / "filters")
    only = tool.main(["--reference", os.path.join(on, "original"), "--estimate", os.path.join(on, "reconstructed"), "--out", outd, "--taps", "2048", "64",
                      "--write-filters", fdir])
    back = R.read_csv(os.path.join(outd, "sdr.csv"))
    assert list(back[0]) == ["file"] + [f"sdr{m}_{k}" for m in (64, 2048) for k in ("in", "out", "delta")] + ["flags_in", "flags_out", "samples"] and len(only) == 2
    by = {r["file"]: r for r in rows}
    for b, r in enumerate(back):
        assert _same(r["sdr64_out"], by[r["file"]]["sdr64_out"]) and _same(r["sdr2048_out"], by[r["file"]]["sdr2048_out"])
        assert math.isnan(r["sdr64_in"]) and math.isnan(r["sdr2048_delta"]) and r["flags_in"] == 0
        fs, h = wavfile.read(os.path.join(fdir, r["file"] + ".wav"))
        assert fs == 16000 and h.dtype == np.float32 and np.array_equal(h, out.filters[names.index(r["file"])].numpy().astype(np.float32))
    with pytest.raises(SystemExit, match="no wav name"):
        tool.main(["--reference", outd, "--estimate", os.path.join(on, "reconstructed")])


def test_tester_sdr_report_aligned(tmp_path):
    """with tester.metrics.align.use the report scores the trimmed pairs of metrics.csv: the eight lag columns with the same values, rows equal to
    evaluate(..., align=50) on the written wavs, and tools/sdr.py --align reproduces them; the report is also written when it is the only one asked for"""
    t_on, on = _run_tester(str(tmp_path), "on", ["tester.metrics.use=true", "tester.metrics.align.use=true", "tester.sdr.use=true", "tester.sdr.taps=[512,8]"])
    rows, mrows = R.read_csv(os.path.join(on, "sdr.csv")), R.read_csv(os.path.join(on, "metrics.csv"))
    cols = ["file"] + [f"sdr{m}_{k}" for m in (8, 512) for k in ("in", "out", "delta")] + ["flags_in", "flags_out", "samples"] + LAGS
    assert list(rows[0]) == cols == list(t_on.sdr_report[0]) and [r["file"] for r in rows] == [r["file"] for r in mrows]
    for r, m in zip(rows, mrows):
        assert all(_same(r[c], m[c]) for c in LAGS + ["samples"]), (r, m)
    again = _tool().main([on, "--align", "--taps", "8", "512", "--out", str(tmp_path / "scored")])
    by = {r["file"]: r for r in t_on.sdr_report}
    assert len(again) == 2 and all(list(r) == cols and all(_same(r[c], by[r["file"]][c]) for c in r) for r in again)
    t_only, only = _run_tester(str(tmp_path), "only", ["tester.sdr.use=true"])
    assert len(t_only.sdr_report) == 2 and os.path.exists(os.path.join(only, "sdr.csv")) and not os.path.exists(os.path.join(only, "metrics.csv"))
