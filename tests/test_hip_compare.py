"""GPU tests of the paired comparison (csrc/compare.hip, buddy_amd/utils/compare.py) against the float64 restatement
tests/_compare_ref.py, whose sums are ``math.fsum``: exact, so every bound is the kernels' own (EPS = 2^-53).

  bootstrap  the medians are integer work on the sorted column: EQUAL to ``np.median`` of the drawn values, bit for bit.  The mean is a sum of at most n
             products cnt[k] s[k] (cnt an integer: one rounding each), at most n - 1 additions on any path of the fixed order and one division, against
             fsum / n with its two roundings: (n + 4) EPS sum cnt |s| / n (``CR.mean_bound``).  Integers with ties and all-equal data whose multiples
             are exact in double (-2.5: every partial sum is a multiple of 0.5 below 2^53) leave nothing to round: equality is required.
  selection  exact: the bits of ``np.sort(row)[k]``.  np.sort calls -0 and +0 equal and leaves their order open, so the rows are compared with np.sort
             by value at every rank, bit for bit wherever the value is not a zero, and bit for bit with the sort that puts -0 below +0
             (``CR.total_order_sort``), which is the kernel's documented order.
  sign-flip  T is n terms added into one accumulator (n - 1 roundings; the sign is a negation), the restatement rounds once: n EPS sum |d|
             (``CR.sign_flip``'s bound).  The p-value compares two such sums, |T_r| >= |T_obs|, so it lies between the restatement's counts with the
             threshold moved up and down by twice that (``CR.p_range``); where the two counts agree -- every case drawn here, checked with the
             restatement on the CPU -- equality is required.  On integer data every T, and hence p, is exact.
  calibration  400 columns of 20 standard normals, P = 2000: the number of columns with p <= 0.05 is Binomial(400, 0.05) under the null, 20 +- 4
             sqrt(19) = 2.6 .. 37.4, inside the issue's 3 .. 38.  The 95 % interval of the mean covers 0 in 380 +- 4 sqrt(19) columns, 363 .. 397, less the percentile
             interval's undercoverage at n = 20, which the restatement gives for this seed on the CPU: it covers in 357 columns of 400, 23 below the
             nominal 380, so the lower edge is 339.6.  (The restatement rejects in 33 columns for this seed, as does the t-test on the same data.)

Every case prints its largest deviation over its bound (profiles/compare_accuracy.txt holds a run's lines)."""
import functools
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _compare_ref as CR  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import compare, report, rng  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5
SENTINEL = 12345.0
CAP = 8192                                    # buddy_compare_max_pairs(), asserted below
NS = (1, 2, 3, 63, 64, 65, 257, 1000, CAP)
RS = (1, 7, 257, 1000)
TRIPLES = ((1, 64, 257), (65, 2, 1000), (CAP, 63, 3))       # the ragged calls of C = 3: every n once
KINDS = ("normal", "wide", "equal", "ties")
EXACT = ("equal", "ties")
CALIBRATION_REF_COVER = 357                   # columns of 400 whose restated interval holds 0 (seed 0, R = 1000): 23 below the nominal 380


@pytest.fixture(scope="module")
def lib():
    lib = _lib.require_gpu()
    assert lib.buddy_compare_max_pairs() == CAP
    return lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def on(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def key_of(label):
    return rng.stream_key(SEED, label)


def column(kind, n):
    rs = np.random.RandomState(1000 * KINDS.index(kind) + n % 997)
    if kind == "normal":
        return rs.standard_normal(n) + 0.2
    if kind == "wide":                        # magnitudes from 1e-8 to 1e8, both signs
        return np.where(rs.rand(n) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(-8.0, 8.0, n)
    if kind == "equal":
        return np.full(n, -2.5)
    return rs.randint(-3, 4, n).astype(np.float64)


@functools.lru_cache(maxsize=None)
def boot_indices(n):
    return CR.indices_all(key_of(f"n{n}"), n, max(RS))


@functools.lru_cache(maxsize=None)
def boot_ref(kind, n):
    """the restatement of column (kind, n) at the largest R; a smaller R is its first draws"""
    return CR.bootstrap(column(kind, n), key_of(f"n{n}"), max(RS), idx=boot_indices(n))


def run_bootstrap(lib, cols, labels, R, draw0=0, pad=5):
    """the raw entry on sorted columns in a NaN-padded (C, ld) array and a sentinel-framed output: -> (C, 2, R) host array"""
    C, ld = len(cols), max(len(c) for c in cols) + pad
    s = np.full((C, ld), np.nan)
    for i, c in enumerate(cols):
        s[i, :len(c)] = np.sort(c)
    lens = np.array([len(c) for c in cols], dtype=np.int32)
    keys = np.array([key_of(v) for v in labels], dtype=np.uint32)
    frame = 64
    out = torch.full((frame + C * 2 * R + frame,), SENTINEL, dtype=torch.float64, device="cuda")
    st, lt, kt = on(s), on(lens), on(keys.view(np.int32))
    _lib.check(lib.buddy_compare_bootstrap(st.data_ptr(), lt.data_ptr(), kt.data_ptr(), C, ld, R, draw0, out.data_ptr() + 8 * frame, stream()))
    host = out.cpu().numpy()
    assert np.all(host[:frame] == SENTINEL) and np.all(host[-frame:] == SENTINEL), "the frame around the output was written"
    return host[frame:-frame].reshape(C, 2, R)


def over(err, bound):
    """the largest err / bound; where the bound is zero the error must be"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


# ---- bootstrap ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("kind", KINDS)
def test_bootstrap_against_restatement(lib, kind, R):
    worst = 0.0
    got = {}
    for trio in TRIPLES:                      # C = 3, ragged
        res = run_bootstrap(lib, [column(kind, n) for n in trio], [f"n{n}" for n in trio], R)
        for i, n in enumerate(trio):
            got[n] = res[i]
    for n in NS:
        means, meds, bound = (v[:R] for v in boot_ref(kind, n))
        assert np.array_equal(bits(got[n][1]), bits(meds)), (kind, n, R, "median")
        if kind in EXACT:
            assert np.array_equal(bits(got[n][0]), bits(means)), (kind, n, R, "mean of exact data")
        else:
            ratio = over(np.abs(got[n][0] - means), bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (kind, n, R, ratio)
        alone = run_bootstrap(lib, [column(kind, n)], [f"n{n}"], R, pad=0)          # C = 1: the same bits as inside the ragged call
        assert np.array_equal(bits(alone[0]), bits(got[n])), (kind, n, R, "C = 1 against C = 3")
    print(f"compare bootstrap: {kind:6s} R {R:4d} n {NS}: medians equal; means " + ("equal" if kind in EXACT else f"deviation / bound {worst:.3f}"))


def test_bootstrap_draw0_shifts_the_draws(lib):
    d = column("normal", 65)
    a = run_bootstrap(lib, [d], ["n65"], 20, draw0=0)
    b = run_bootstrap(lib, [d], ["n65"], 7, draw0=13)
    assert np.array_equal(bits(a[0, :, 13:]), bits(b[0]))


# ---- selection ----------------------------------------------------------------------------------------------------------------------------------
def select_rows(R):
    rs = np.random.RandomState(R)
    tiny = 5e-324
    pool = np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, -1.0, 1.0 + 2.0 ** -52, 1e300, -1e300, 7.0, 7.0])
    return np.stack([rs.standard_normal(R),                                   # mixed signs
                     rs.choice(pool, R),                                      # duplicates, signed zeros, denormals
                     np.round(rs.standard_normal(R) * 3.0) + 0.0,             # many ties, +0 only
                     -np.abs(rs.standard_normal(R)) * 10.0 ** rs.randint(-300, 300, R),
                     np.full(R, -0.0)])


@pytest.mark.parametrize("R", (2, 255, 256, 257, 10000))
def test_select_is_np_sort(lib, R):
    x = select_rows(R)
    k = R // 40
    ranks = [0, k, R - 1 - k, R - 1]
    got = compare.select(on(x), ranks).cpu().numpy()
    alone = compare.select(on(x[1:2]), ranks).cpu().numpy()
    assert np.array_equal(bits(alone[0]), bits(got[1]))
    for m in range(x.shape[0]):
        want, total = np.sort(x[m])[ranks], CR.total_order_sort(x[m])[ranks]
        assert np.array_equal(got[m], want), (R, m, "values")
        nz = want != 0.0
        assert np.array_equal(bits(got[m])[nz], bits(want)[nz]), (R, m, "bits of np.sort away from the zeros")
        assert np.array_equal(bits(got[m]), bits(total)), (R, m, "bits with -0 below +0")
    print(f"compare select: R {R:5d} ranks {ranks}: 5 rows equal to np.sort")


# ---- sign-flip ----------------------------------------------------------------------------------------------------------------------------------
def run_signflip(lib, cols, labels, P, draw0=0, pad=3):
    """the raw entry with the Python layer's choice of mode: -> T (C, P) host (sentinel where nothing was written), tobs (C,), p (C,), modes"""
    C, ld = len(cols), max(len(c) for c in cols) + pad
    d = np.full((C, ld), np.nan)
    for i, c in enumerate(cols):
        d[i, :len(c)] = c
    lens = np.array([len(c) for c in cols], dtype=np.int32)
    modes = np.array([1 if n <= 30 and 2 ** int(n) <= P else 0 for n in lens], dtype=np.int32)
    patterns = np.where(modes == 1, 2 ** np.minimum(lens, 30).astype(np.int64), P)
    keys = np.array([key_of(v) for v in labels], dtype=np.uint32)
    frame = 64
    buf = torch.full((frame + C * P + frame,), SENTINEL, dtype=torch.float64, device="cuda")
    tobs = torch.full((C + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    dt, lt, mt, kt = on(d), on(lens), on(modes), on(keys.view(np.int32))
    _lib.check(lib.buddy_compare_signflip(dt.data_ptr(), lt.data_ptr(), mt.data_ptr(), kt.data_ptr(), C, ld, P, draw0, buf.data_ptr() + 8 * frame,
                                          tobs.data_ptr() + 8, stream()))
    T = buf[frame:frame + C * P].view(C, P)
    count = compare.count_ge(T, patterns, tobs[1:C + 1].abs().contiguous()).cpu().numpy()
    host, th = buf.cpu().numpy(), tobs.cpu().numpy()
    assert np.all(host[:frame] == SENTINEL) and np.all(host[-frame:] == SENTINEL) and th[0] == SENTINEL and th[-1] == SENTINEL
    p = np.where(modes == 1, count / patterns, (1.0 + count) / (1.0 + patterns))
    return host[frame:-frame].reshape(C, P), th[1:-1], p, modes


def flip_column(n, integer=False):
    rs = np.random.RandomState(77 + n)
    return rs.randint(-4, 6, n).astype(np.float64) if integer else rs.standard_normal(n) + 2.0 / math.sqrt(n + 3.0)


@pytest.mark.parametrize("integer", (False, True))
def test_signflip_exhaustive(lib, integer):
    ns, P = (1, 2, 3, 8, 12), 5000
    cols = [flip_column(n, integer) for n in ns]
    labels = [f"x{n}" for n in ns]
    T, tobs, p, modes = run_signflip(lib, cols, labels, P)
    assert modes.tolist() == [1] * 5
    worst = 0.0
    for i, n in enumerate(ns):
        Tr, to, bound, ex = CR.sign_flip(cols[i], key_of(labels[i]), P)
        assert ex and len(Tr) == 2 ** n
        assert np.all(T[i, 2 ** n:] == SENTINEL), (n, "entries beyond 2^n were written")
        assert bits(T[i, :1])[0] == bits(tobs[i:i + 1])[0], (n, "pattern 0 is T_obs")
        assert np.array_equal(bits(T[i, 2 ** n - 1:2 ** n]), bits(-tobs[i:i + 1])), (n, "the last pattern is -T_obs")
        if integer:
            assert np.array_equal(T[i, :2 ** n], Tr) and tobs[i] == to and p[i] == CR.p_value(Tr, abs(to), True), (n, "integer data are exact")
        else:
            ratio = max(over(np.abs(T[i, :2 ** n] - Tr), np.full(2 ** n, bound)), over(abs(tobs[i] - to), bound))
            worst = max(worst, ratio)
            lo, hi = CR.p_range(Tr, to, bound, True)
            assert ratio <= 1.0 and lo <= p[i] <= hi, (n, ratio, lo, p[i], hi)
            assert lo == hi, (n, "the restatement's p-value is not settled for this column: draw another")
    print(f"compare sign-flip exhaustive: {'integer' if integer else 'normal '} n {ns}: " + ("T and p equal" if integer else f"deviation / bound {worst:.3f}, p equal"))


@pytest.mark.parametrize("n", (31, 32, 33, 64, 65, 1000))
def test_signflip_random(lib, n):
    Ps = (1, 1000, 4097)
    d, label = flip_column(n), f"r{n}"
    Tr, to, bound, ex = CR.sign_flip(d, key_of(label), max(Ps))               # a smaller P is its first patterns
    assert not ex
    worst, settled = 0.0, 0
    for P in Ps:
        T, tobs, p, modes = run_signflip(lib, [d, flip_column(5)], [label, "other"], P)      # beside a column of another length (and mode, from P = 1000 on)
        assert modes[0] == 0
        ratio = max(over(np.abs(T[0] - Tr[:P]), np.full(P, bound)), over(abs(tobs[0] - to), bound))
        worst = max(worst, ratio)
        lo, hi = CR.p_range(Tr[:P], to, bound, False)
        assert ratio <= 1.0 and lo <= p[0] <= hi, (n, P, ratio, lo, p[0], hi)
        assert lo == hi, (n, P, "the restatement's p-value is not settled for this column: draw another")
        settled += lo == hi
    Ti, _, pi, _ = run_signflip(lib, [flip_column(n, True)], [label], 1000)
    Tri, toi, _, _ = CR.sign_flip(flip_column(n, True), key_of(label), 1000)
    assert np.array_equal(Ti[0], Tri) and pi[0] == CR.p_value(Tri, abs(toi), False), (n, "integer data are exact")
    print(f"compare sign-flip random: n {n:4d} P {Ps}: deviation / bound {worst:.3f}; p equal in {settled} of {len(Ps)}; integer data equal")


# ---- independence -------------------------------------------------------------------------------------------------------------------------------
def test_a_column_does_not_depend_on_its_call(lib):
    """alone, among others and at another position: the bits of all three kernels; and a second call repeats the first"""
    ns = (257, 12, 40, 1000)
    cols, labels = [flip_column(n) for n in ns], [f"i{n}" for n in ns]
    R, P = 257, 4097
    boot = run_bootstrap(lib, cols, labels, R)
    T, tobs, p, _ = run_signflip(lib, cols, labels, P)
    sel = compare.select(on(boot.reshape(8, R)), [6, 250]).cpu().numpy()
    order = (2, 0, 3, 1)
    boot2 = run_bootstrap(lib, [cols[i] for i in order], [labels[i] for i in order], R, pad=11)
    T2, tobs2, p2, _ = run_signflip(lib, [cols[i] for i in order], [labels[i] for i in order], P, pad=0)
    sel2 = compare.select(on(boot2.reshape(8, R)), [6, 250]).cpu().numpy()
    for q, i in enumerate(order):
        assert np.array_equal(bits(boot2[q]), bits(boot[i])) and np.array_equal(bits(T2[q]), bits(T[i])) and bits(tobs2[q:q + 1])[0] == bits(tobs[i:i + 1])[0]
        assert p2[q] == p[i] and np.array_equal(bits(sel2[2 * q:2 * q + 2]), bits(sel[2 * i:2 * i + 2]))
        b1 = run_bootstrap(lib, [cols[i]], [labels[i]], R)
        T1, tobs1, p1, _ = run_signflip(lib, [cols[i]], [labels[i]], P)
        assert np.array_equal(bits(b1[0]), bits(boot[i])) and np.array_equal(bits(T1[0]), bits(T[i])) and p1[0] == p[i]
        assert np.array_equal(bits(compare.select(on(b1[0]), [6, 250]).cpu().numpy()), bits(sel[2 * i:2 * i + 2]))
    again = run_bootstrap(lib, cols, labels, R)
    Ta, _, pa, _ = run_signflip(lib, cols, labels, P)
    assert np.array_equal(bits(again), bits(boot)) and np.array_equal(bits(Ta), bits(T)) and np.array_equal(pa, p)
    # the Python layer's wrappers give the entry's bits (the bootstrap sorts on the device)
    C, ld = len(cols), max(ns)
    d = np.zeros((C, ld))
    for i, c in enumerate(cols):
        d[i, :len(c)] = c
    keys = np.array([key_of(v) for v in labels], dtype=np.uint32)
    assert np.array_equal(bits(compare.bootstrap(on(d), np.array(ns), keys, R).cpu().numpy()), bits(boot))
    Tw, tw, patterns, modes = compare.sign_flip(on(d), np.array(ns), keys, P)
    assert modes.tolist() == [0, 1, 0, 0] and patterns.tolist() == [P, 4096, P, P] and np.array_equal(bits(tw.cpu().numpy()), bits(tobs))
    assert np.array_equal(bits(Tw.cpu().numpy()[0]), bits(T[0])) and np.array_equal(bits(Tw.cpu().numpy()[1, :4096]), bits(T[1, :4096]))
    print("compare independence: bootstrap, selection and sign-flip bits do not depend on C, position or padding; a second call repeats the first")


# ---- calibration --------------------------------------------------------------------------------------------------------------------------------
def test_calibration_under_the_null():
    C, n = 400, 20
    data = np.random.RandomState(0).standard_normal((n, C))
    recs = compare.paired(None, data, [f"null{c}" for c in range(C)], seed=0, resamples=1000, permutations=2000, level=0.95)
    assert all(r["patterns"] == 2000 and r["flags"] == 0 and r["n"] == n for r in recs)
    reject = sum(r["p_signflip"] <= 0.05 for r in recs)
    cover = sum(r["mean_lo"] <= 0.0 <= r["mean_hi"] for r in recs)
    sd = math.sqrt(C * 0.05 * 0.95)
    lower = C * 0.95 - 4.0 * sd - max(0, C * 0.95 - CALIBRATION_REF_COVER)
    print(f"compare calibration: 400 null columns of n = 20: p <= 0.05 in {reject} (3 .. 37 allowed); the 95 % interval of the mean holds 0 in {cover} "
          f"({lower:.1f} .. {C * 0.95 + 4.0 * sd:.1f} allowed; restatement {CALIBRATION_REF_COVER})")
    assert C * 0.05 - 4.0 * sd <= reject <= C * 0.05 + 4.0 * sd
    assert lower <= cover <= C * 0.95 + 4.0 * sd
    # a column of the call is the restatement's: edges by order statistics of its bootstrap values, p by its counts
    for c in (0, 123, 399):
        (mlo, mhi), (qlo, qhi), p, ex = CR.paired_column(data[:, c], f"null{c}", 0, 1000, 2000, 0.95)
        r = recs[c]
        tol = 24 * CR.EPS * np.abs(data[:, c]).max()                          # CR.mean_bound's (n + 4) EPS at the largest |s|
        assert not ex and abs(r["mean_lo"] - mlo) <= tol and abs(r["mean_hi"] - mhi) <= tol and (r["median_lo"], r["median_hi"]) == (qlo, qhi)
        assert r["p_signflip"] == p, (c, r["p_signflip"], p)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def metrics_rows(seed, shift):
    rs = np.random.RandomState(seed)
    rows = []
    for i in range(8):
        vi, vo = 3.0 + rs.standard_normal(), 9.0 + shift + rs.standard_normal()
        si, so = 0.6 + 0.05 * rs.standard_normal(), 0.8 + 0.02 * shift + 0.05 * rs.standard_normal()
        rows.append({"file": f"utt{i}", "samples": 16000, "si_sdr_in": vi, "si_sdr_out": vo, "si_sdr_delta": vo - vi, "stoi_in": si,
                     "stoi_out": so if i != 5 else float("nan"), "stoi_delta": so - si if i != 5 else float("nan"), "flags_in": 0, "flags_out": 0})
    return rows


def test_tool_end_to_end(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    report.write_report(str(a / "metrics.csv"), metrics_rows(1, 0.0))
    report.write_report(str(b / "metrics.csv"), metrics_rows(2, 1.0) + [{**metrics_rows(3, 0.0)[0], "file": "extra"}])
    args = [str(a), str(b), "--resamples", "400", "--permutations", "1000"]
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "compare.py")] + args + ["--out", str(tmp_path / "o1")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "1 file(s) in run B only: extra" in run.stderr and "si_sdr_out" in run.stdout and "EXHAUSTIVE|UNPAIRED" in run.stdout
    first = open(tmp_path / "o1" / "comparison_metrics.csv", "rb").read()
    # the file is ``paired`` on the joined arrays
    tab = compare.compare_reports(str(a / "metrics.csv"), str(b / "metrics.csv"))
    assert tab["labels"] == ["si_sdr_in", "si_sdr_out", "si_sdr_delta", "stoi_in", "stoi_out", "stoi_delta"]
    recs = compare.paired(tab["a"], tab["b"], tab["labels"], 0, 400, 1000, 0.95, only_a=0, only_b=1)
    report.write_report(str(tmp_path / "direct.csv"), recs)
    assert open(tmp_path / "direct.csv", "rb").read() == first
    by = {r["column"]: r for r in recs}
    assert by["si_sdr_out"]["n"] == 8 and by["stoi_out"]["n"] == 7 and by["si_sdr_out"]["patterns"] == 256 and by["stoi_out"]["patterns"] == 128
    assert all(r["flags"] == compare.EXHAUSTIVE | compare.UNPAIRED and r["only_b"] == 1 and r["only_a"] == 0 for r in recs)
    assert all(r["mean_lo"] <= r["mean_diff"] <= r["mean_hi"] and r["p_signflip"] >= 2 / r["patterns"] and r["p_holm"] >= r["p_signflip"] for r in recs)
    # a second run gives the same bytes; another seed moves the interval edges and leaves the enumerated p-values alone
    spec = importlib.util.spec_from_file_location("compare_tool", os.path.join(ROOT, "tools", "compare.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(args + ["--out", str(tmp_path / "o2")])
    assert open(tmp_path / "o2" / "comparison_metrics.csv", "rb").read() == first
    other = tool.main(args + ["--out", str(tmp_path / "o3"), "--seed", "1"])["metrics"]
    assert open(tmp_path / "o3" / "comparison_metrics.csv", "rb").read() != first
    assert any((r["mean_lo"], r["mean_hi"]) != (o["mean_lo"], o["mean_hi"]) for r, o in zip(recs, other))
    assert all(r["p_signflip"] == o["p_signflip"] and r["p_sign"] == o["p_sign"] and r["mean_diff"] == o["mean_diff"] for r, o in zip(recs, other))
    # one run: its *_delta columns against zero
    one = tool.main([str(b), "--resamples", "400", "--permutations", "1000", "--out", str(tmp_path / "o4")])["metrics"]
    assert [r["column"] for r in one] == ["si_sdr_delta", "stoi_delta"] and one[0]["n"] == 9 and math.isnan(one[0]["mean_a"])
    assert one[0]["mean_diff"] > 0 and one[0]["mean_lo"] > 0 and one[0]["p_signflip"] == 2 / 512
    print(f"compare end to end: si_sdr_out {by['si_sdr_out']['mean_diff']:+.3f} dB [{by['si_sdr_out']['mean_lo']:+.3f}, {by['si_sdr_out']['mean_hi']:+.3f}] "
          f"p {by['si_sdr_out']['p_signflip']:.4f} over {by['si_sdr_out']['patterns']} patterns; same bytes from a second run")
