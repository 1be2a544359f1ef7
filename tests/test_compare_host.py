"""CPU tests of the paired comparison's host side: the new symbols and purpose numbers, every argument refusal of the C entries
(nothing is launched; the lengths, modes, ranks and counts, which the entries read to check them, are real host arrays) and of the Python layer and
the tool, the float64 restatement (tests/_compare_ref.py) and the host statistics on hand-checked cases, and the CSV join on written-out reports."""
import ctypes as C
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _compare_ref as CR  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import compare, report, rng, rooms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("buddy_compare_max_pairs", "buddy_compare_bootstrap", "buddy_compare_select", "buddy_compare_signflip", "buddy_compare_count_ge")


def tool():
    spec = importlib.util.spec_from_file_location("compare_tool", os.path.join(ROOT, "tools", "compare.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- symbols and refusals -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTED and getattr(lib, name) is not None       # header = signatures = exports: tests/test_abi_host.py
    assert os.path.isfile(os.path.join(ROOT, "buddy_amd", "csrc", "compare.hip"))          # build.sh compiles and links every csrc/*.hip
    assert lib.buddy_compare_max_pairs() >= 8192 and compare.max_pairs() == lib.buddy_compare_max_pairs()


def test_purpose_numbers():
    assert (compare.COMPARE_BOOT, compare.COMPARE_SIGN) == (11, 12) == (CR.BOOT, CR.SIGN)
    assert compare.COMPARE_BOOT == rooms.TAIL + 1


def test_argument_checks_need_no_gpu():
    """every BUDDY_ERR_ARG case of the four entries, with nothing launched: 0x1000 stands in for the data pointers"""
    lib = _lib.load()
    X, cap = 0x1000, lib.buddy_compare_max_pairs()
    ints = lambda *v: C.cast((C.c_int * len(v))(*v), C.c_void_p)
    good = dict(d=X, lens=ints(5, 3), keys=X, C=2, ld=8, R=100, P=1000, draw0=0, out=X, modes=ints(0, 1), T=X, tobs=X, x=X, M=4, ldx=100, ranks=ints(2, 97),
                K=2, counts=ints(1000, 8), thr=X, ldt=1000)
    columns = [(dict(d=None), "null data"), (dict(lens=None), "null lens"), (dict(keys=None), "null keys"), (dict(C=0), "C < 1"), (dict(C=65536), "C above 65535"),
               (dict(lens=ints(0, 3)), "a length of 0"), (dict(lens=ints(5, -1)), "a negative length"), (dict(lens=ints(5, cap + 1), ld=cap + 1), "a length above max_pairs"),
               (dict(ld=4), "ld below a length")]
    boot = [(dict(out=None), "null out"), (dict(R=0), "R < 1"), (dict(R=2 ** 24 + 1), "R above 2^24"), (dict(draw0=2 ** 32 - 99), "draw0 + R above 2^32")]
    flip = [(dict(modes=None), "null modes"), (dict(T=None), "null T"), (dict(tobs=None), "null tobs"), (dict(P=0), "P < 1"), (dict(P=2 ** 30 + 1), "P above 2^30"),
            (dict(draw0=2 ** 32 - 999), "draw0 + P above 2^32"), (dict(modes=ints(0, 2)), "an unknown mode"), (dict(modes=ints(1, 1), lens=ints(5, 10), ld=10), "2^10 above P = 1000"),
            (dict(modes=ints(1, 1), lens=ints(5, 31), ld=31, P=2 ** 30), "2^31 above any P"), (dict(P=7), "2^3 above P = 7")]
    sel = [(dict(x=None), "null x"), (dict(ranks=None), "null ranks"), (dict(out=None), "null out"), (dict(M=0), "M < 1"), (dict(M=65536), "M above 65535"),
           (dict(R=0), "R < 1"), (dict(ldx=99), "ldx < R"), (dict(K=0), "K < 1"), (dict(ranks=ints(2, 100)), "a rank of R"), (dict(ranks=ints(-1, 97)), "a negative rank")]
    cnt = [(dict(T=None), "null T"), (dict(counts=None), "null counts"), (dict(thr=None), "null thr"), (dict(out=None), "null out"), (dict(C=0), "C < 1"),
           (dict(C=65536), "C above 65535"), (dict(counts=ints(1000, 0)), "a count of 0"), (dict(counts=ints(1001, 8)), "a count above ldt")]
    calls = (
        (lambda a: lib.buddy_compare_bootstrap(a["d"], a["lens"], a["keys"], a["C"], a["ld"], a["R"], a["draw0"], a["out"], None), "buddy_compare_bootstrap: ",
         columns + boot),
        (lambda a: lib.buddy_compare_signflip(a["d"], a["lens"], a["modes"], a["keys"], a["C"], a["ld"], a["P"], a["draw0"], a["T"], a["tobs"], None),
         "buddy_compare_signflip: ", columns + flip),
        (lambda a: lib.buddy_compare_select(a["x"], a["M"], a["R"], a["ldx"], a["ranks"], a["K"], a["out"], None), "buddy_compare_select: ", sel),
        (lambda a: lib.buddy_compare_count_ge(a["T"], a["counts"], a["thr"], a["C"], a["ldt"], a["out"], None), "buddy_compare_count_ge: ", cnt))
    for call, who, cases in calls:
        for change, why in cases:
            assert call(dict(good, **change)) == 2, (who, why)
            assert lib.buddy_last_error().decode().startswith(who), (who, why)


def test_python_refusals_and_cpu_tensors():
    cap = compare.max_pairs()
    d = torch.zeros(2, 8, dtype=torch.float64)
    keys = np.array([rng.stream_key(0, "a"), rng.stream_key(0, "b")], dtype=np.uint32)
    lens = np.array([5, 3])
    for fn, extra in ((compare.bootstrap, 100), (compare.sign_flip, 100)):
        for bad, why in ((dict(d=d.float()), "float64"), (dict(d=d[0]), "float64"), (dict(lens=np.array([5])), "lens"), (dict(lens=np.array([5.0, 3.0])), "lens"),
                         (dict(keys=keys[:1]), "keys"), (dict(keys=keys.astype(np.int64)), "keys"), (dict(lens=np.array([5, 0])), "empty"),
                         (dict(lens=np.array([5, 9])), "stride"), (dict(n=0), "must be in"), (dict(draw0=2 ** 32 - 50), "2\\^32"), (dict(draw0=-1), "2\\^32")):
            a = dict(dict(d=d, lens=lens, keys=keys, n=extra, draw0=0), **bad)
            with pytest.raises(ValueError, match=why):
                fn(a["d"], a["lens"], a["keys"], a["n"], a["draw0"])
        # too long a column: both numbers are named, before anything is launched
        big = torch.zeros(1, cap + 1, dtype=torch.float64)
        with pytest.raises(ValueError, match=f"{cap + 1} pairs.*{cap}"):
            fn(big, np.array([cap + 1]), keys[:1], extra)
        with pytest.raises(_lib.BuddyHipError):                                 # CPU tensors
            fn(d, lens, keys, extra)
    x = torch.zeros(3, 50, dtype=torch.float64)
    for bad, why in ((dict(x=x.float()), "float64"), (dict(ranks=[]), "ranks"), (dict(ranks=[0.5]), "ranks"), (dict(ranks=[50]), "rank is outside"),
                     (dict(ranks=[-1]), "rank is outside")):
        a = dict(dict(x=x, ranks=[1, 48]), **bad)
        with pytest.raises(ValueError, match=why):
            compare.select(a["x"], a["ranks"])
    with pytest.raises(_lib.BuddyHipError):
        compare.select(x, [1, 48])
    T, thr = torch.zeros(2, 10, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    for bad, why in ((dict(T=T.float()), "float64"), (dict(thr=thr[:1]), "float64"), (dict(patterns=np.array([10, 11])), "patterns"),
                     (dict(patterns=np.array([0, 10])), "patterns"), (dict(patterns=np.array([10])), "patterns")):
        a = dict(dict(T=T, patterns=np.array([10, 8]), thr=thr), **bad)
        with pytest.raises(ValueError, match=why):
            compare.count_ge(a["T"], a["patterns"], a["thr"])
    with pytest.raises(_lib.BuddyHipError):
        compare.count_ge(T, np.array([10, 8]), thr)
    # paired: shapes, labels, the interval's ranks, the caps -- all before the GPU is asked for
    a, b = np.zeros((4, 2)), np.ones((4, 2))
    for kw, why in ((dict(a=np.zeros((3, 2))), "one shape"), (dict(labels=["x"]), "label"), (dict(labels=["x", "x"]), "label"), (dict(resamples=39), "resamples"),
                    (dict(level=1.0), "level"), (dict(level=0.0), "level"), (dict(permutations=0), "permutations"), (dict(resamples=2 ** 24 + 1), "resamples")):
        k = dict(dict(a=a, b=b, labels=["x", "y"], resamples=1000, permutations=1000, level=0.95), **kw)
        with pytest.raises(ValueError, match=why):
            compare.paired(k["a"], k["b"], k["labels"], 0, k["resamples"], k["permutations"], k["level"])
    with pytest.raises(ValueError, match=f"{cap + 1} pairs.*{cap}"):
        compare.paired(None, np.ones((cap + 1, 1)), ["x"])
    with pytest.raises(_lib.BuddyHipError):                                     # a CPU device: no fallback
        compare.paired(a, b + np.arange(4)[:, None], ["x", "y"], device="cpu")
    # columns with fewer than two pairs never reach the GPU: the whole record is host work
    recs = compare.paired(np.array([[1.0, np.nan], [np.nan, np.nan]]), np.array([[3.0, 1.0], [2.0, np.nan]]), ["one", "none"], only_a=2)
    one, none = recs
    assert one["n"] == 1 and one["flags"] == compare.FEW | compare.DEGENERATE | compare.UNPAIRED and one["only_a"] == 2
    assert (one["mean_diff"], one["mean_lo"], one["mean_hi"], one["median_lo"], one["median_hi"], one["mean_a"], one["mean_b"]) == (2.0, 2.0, 2.0, 2.0, 2.0, 1.0, 3.0)
    assert all(math.isnan(one[k]) for k in ("std_diff", "dz", "p_sign", "p_signflip", "p_holm")) and one["patterns"] == 0
    assert none["n"] == 0 and none["flags"] == compare.FEW | compare.UNPAIRED and math.isnan(none["mean_diff"]) and math.isnan(none["mean_lo"])
    assert tuple(one.keys()) == compare.COLUMNS


# ---- the restatement and the host statistics by hand --------------------------------------------------------------------------------------------
def test_indices_are_the_scaled_words():
    key = rng.stream_key(3, "col")
    for n, draw in ((1, 0), (7, 5), (1000, 2)):
        w = rng.words(key, 11, draw, n)
        want = [(int(v) * n) >> 32 for v in w]
        assert CR.indices(key, n, draw).tolist() == want and 0 <= min(want) and max(want) < n
    # a resample's mean and median are those of the drawn values
    d = np.array([4.0, -1.0, 2.5, 0.5, 9.0])
    means, meds, bound = CR.bootstrap(d, key, 3, draw0=7)
    v = np.sort(d)[CR.indices(key, 5, 8)]
    assert means[1] == math.fsum(v) / 5 and meds[1] == np.median(v) and bound[1] == 9 * CR.EPS * np.abs(v).sum() / 5


def test_sign_flip_by_hand():
    """d = (1, 2, 4): T_obs = 7, and of the 8 patterns only + + + and - - - reach |T| >= 7: p = 2 / 8.
    d = (1, 1, -1): T_obs = 1; the sums s1 + s2 - s3 over the 8 patterns are 1, -1, -1, -3, 3, 1, 1, -1 (r = 0..7, bit j of r flips d[j]):
    every |T| >= 1, so p = 8 / 8 = 1 -- the smallest observed |T| there is cannot be significant."""
    key = rng.stream_key(0, "x")
    T, tobs, bound, ex = CR.sign_flip([1.0, 2.0, 4.0], key, 8)
    assert ex and tobs == 7.0 and T.tolist() == [7.0, 5.0, 3.0, 1.0, -1.0, -3.0, -5.0, -7.0] and CR.p_value(T, abs(tobs), ex) == 2 / 8
    assert bound == 3 * 2.0 ** -53 * 7.0
    T, tobs, _, ex = CR.sign_flip([1.0, 1.0, -1.0], key, 100)
    assert ex and tobs == 1.0 and T.tolist() == [1.0, -1.0, -1.0, -3.0, 3.0, 1.0, 1.0, -1.0] and CR.p_value(T, abs(tobs), ex) == 1.0
    # P = 7 < 2^3: random patterns from purpose 12, bit j & 31 of word j >> 5 of draw r; p = (1 + count) / (1 + P)
    T, tobs, _, ex = CR.sign_flip([1.0, 2.0, 4.0], key, 7)
    assert not ex and len(T) == 7
    for r in range(7):
        w = int(rng.words(key, 12, r, 1)[0])
        assert T[r] == sum(-v if (w >> j) & 1 else v for j, v in enumerate((1.0, 2.0, 4.0)))
    assert CR.p_value(T, 7.0, False) == (1 + int(np.sum(np.abs(T) >= 7.0))) / 8
    # bit 32 of a pattern is bit 0 of the draw's second word
    sg = CR.signs(key, 40, 2, draw0=3)
    w = rng.words(key, 12, 4, 2)
    assert sg.shape == (2, 40) and sg[1, 32] == (-1.0 if int(w[1]) & 1 else 1.0) and sg[1, 31] == (-1.0 if int(w[0]) >> 31 else 1.0)


def test_sign_test_holm_and_ranks_by_hand():
    # 7 wins to 1 loss: 2 (C(8,0) + C(8,1)) / 2^8 = 18 / 256
    assert compare.sign_test(7, 1) == CR.sign_test(7, 1) == 18 / 256 and compare.sign_test(1, 7) == 18 / 256
    assert compare.sign_test(0, 0) == 1.0 and compare.sign_test(4, 4) == 1.0 and compare.sign_test(5, 0) == 2 / 32
    for w, l in ((3, 9), (40, 61), (300, 240)):                                # the running binomial is math.comb's sum
        assert compare.sign_test(w, l) == CR.sign_test(w, l) and 0.0 < compare.sign_test(w, l) <= 1.0
    assert 0.03 < compare.sign_test(4000, 4192) < 0.04                         # no overflow at 8192 pairs; z = 2.12 (normal approximation: 0.034)
    # Holm: p = (0.01, 0.04, 0.03, 0.005), m = 4.  Sorted 0.005, 0.01, 0.03, 0.04 take the factors 4, 3, 2, 1: 0.02, 0.03, 0.06, 0.04, and the
    # running maximum makes the last 0.06
    got = compare.holm([0.01, 0.04, 0.03, 0.005])
    assert np.allclose(got, [0.03, 0.06, 0.06, 0.02], rtol=0, atol=1e-17) and np.allclose(CR.holm([0.01, 0.04, 0.03, 0.005]), got, rtol=0, atol=1e-17)
    got = compare.holm([0.5, float("nan"), 0.4])                               # NaN takes no part: m = 2; 0.8, then max(0.8, 0.5)
    assert got[0] == 0.8 and math.isnan(got[1]) and got[2] == 0.8
    assert compare.holm([0.9, 0.8]).tolist() == [1.0, 1.0]
    # the interval's ranks
    assert compare.interval_ranks(1000, 0.95) == (25, 974) and compare.interval_ranks(10000, 0.95) == (250, 9749)
    assert compare.interval_ranks(1000, 0.9) == (50, 949) and compare.interval_ranks(40, 0.95) == (1, 38)
    with pytest.raises(ValueError, match="at least 40"):
        compare.interval_ranks(39, 0.95)
    assert CR.interval(np.arange(1000.0)[::-1].copy(), 25) == (25.0, 974.0)
    assert compare.flag_names(0) == "-" and compare.flag_names(5) == "FEW|EXHAUSTIVE"


def test_total_order_sort_is_np_sort_with_signed_zeros_ordered():
    row = np.array([0.0, -0.0, 3.0, -3.0, 5e-324, -5e-324, 0.0, -0.0, 3.0])
    got = CR.total_order_sort(row)
    assert np.array_equal(got, np.sort(row)) and np.signbit(got).tolist() == [True, True, True, True, False, False, False, False, False]


# ---- the CSV join -------------------------------------------------------------------------------------------------------------------------------
def rows_of(names, base, mode="m"):
    nan = float("nan")
    out = []
    for i, name in enumerate(names):
        vi, vo = base + i, base + 2.0 * i + 0.5
        out.append({"file": name, "samples": 16000 + i, "si_sdr_in": vi, "si_sdr_out": vo if name != "f2" else nan, "si_sdr_delta": vo - vi if name != "f2" else nan,
                    "lag_in": i, "lag_out": -i, "lag_ms_in": i / 16.0, "lag_ms_out": -i / 16.0, "flags_in": 0, "flags_out": 4, "align_flags_in": 1, "mode": mode,
                    "frames_out": 10 + i, "level_db": -26.0 - 0.25 * i})
    return out


def test_csv_join(tmp_path):
    pa, pb = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    report.write_report(pa, rows_of(["f0", "f1", "f2", "f3", "onlya"], 1.0))
    report.write_report(pb, rows_of(["f3", "f2", "f1", "f0", "onlyb", "onlyb2"], 2.0))
    tab = compare.compare_reports(pa, pb)
    assert tab["files"] == ["f0", "f1", "f2", "f3"] and tab["only_a"] == ["onlya"] and tab["only_b"] == ["onlyb", "onlyb2"]
    # scores: the in / out / delta columns that are no flag word and no integer lag, and the plain float column; never samples, frames, flags, lags, mode
    assert tab["labels"] == ["si_sdr_in", "si_sdr_out", "si_sdr_delta", "lag_ms_in", "lag_ms_out", "level_db"]
    assert tab["a"].shape == tab["b"].shape == (4, 6)
    assert tab["a"][:, 0].tolist() == [1.0, 2.0, 3.0, 4.0] and tab["b"][:, 0].tolist() == [5.0, 4.0, 3.0, 2.0]       # B in A's file order: f0 is B's fourth row
    assert math.isnan(tab["a"][2, 1]) and tab["a"][3, 1] == 7.5 and math.isnan(tab["b"][2, 1]) and tab["b"][0, 1] == 8.5
    assert tab["b"][:, 5].tolist() == [-26.75, -26.5, -26.25, -26.0]
    # asked columns: a subset in the asked order; a non-numeric or integer or unknown column is refused
    assert compare.compare_reports(pa, pb, ["level_db", "si_sdr_out"])["labels"] == ["level_db", "si_sdr_out"]
    for bad in ("mode", "samples", "flags_out", "lag_in", "nothing", "file"):
        with pytest.raises(ValueError, match="not a numeric score column"):
            compare.compare_reports(pa, pb, [bad])
    # one run: its *_delta columns against zero
    one = compare.compare_reports(pb)
    assert one["a"] is None and one["labels"] == ["si_sdr_delta"] and one["only_a"] == one["only_b"] == []
    assert one["files"] == ["f3", "f2", "f1", "f0", "onlyb", "onlyb2"] and math.isnan(one["b"][1, 0])
    assert np.delete(one["b"][:, 0], 1).tolist() == [0.5, 2.5, 3.5, 4.5, 5.5]
    # no common file, no file column, a file twice
    pc = str(tmp_path / "c.csv")
    report.write_report(pc, rows_of(["g0", "g1"], 0.0))
    with pytest.raises(ValueError, match="no file is common"):
        compare.compare_reports(pa, pc)
    report.write_report(pc, [{"name": "f0", "x_out": 1.0}])
    with pytest.raises(ValueError, match="no 'file' column"):
        compare.compare_reports(pa, pc)
    report.write_report(pc, [{"file": "f0", "x_out": 1.0}, {"file": "f0", "x_out": 2.0}])
    with pytest.raises(ValueError, match="twice"):
        compare.compare_reports(pc, pa)
    report.write_report(pc, [{"file": "f0", "samples": 3}, {"file": "f1", "samples": 4}])
    with pytest.raises(ValueError, match="no score column"):
        compare.compare_reports(pc, pc)


def test_tool_refusals(tmp_path):
    T = tool()
    a, b, e = tmp_path / "a", tmp_path / "b", tmp_path / "empty"
    for d in (a, b, e):
        d.mkdir()
    report.write_report(str(a / "metrics.csv"), rows_of(["f0", "f1", "f2"], 1.0))
    report.write_report(str(b / "metrics.csv"), rows_of(["g0", "g1", "g2"], 1.0))
    report.write_report(str(a / "levels.csv"), [{"file": "f0", "samples": 3}, {"file": "f1", "samples": 4}])
    cases = (([str(a), str(tmp_path / "missing")], "does not exist"), ([str(a), str(e)], "no report"), ([str(a), str(b), "--report", "srmr"], "srmr.csv is not in"),
             ([str(a), str(b), "--report", "scores"], "--report takes"), ([str(a), str(a / "metrics.csv")], "not one of each"),
             ([str(a), str(b), "--resamples", "39"], "--resamples"), ([str(a), str(b), "--resamples", "0"], "--resamples"),
             ([str(a), str(b), "--level", "1.5"], "--level"), ([str(a), str(b), "--permutations", "0"], "--permutations"),
             ([str(a), str(b)], "no file is common"), ([str(a), str(a), "--columns", "mode"], "not a numeric score column"),
             ([str(a / "metrics.csv"), str(b / "metrics.csv"), "--report", "srmr"], "does not name"), ([str(a), "--report", "levels"], "no score column"))
    for argv, why in cases:
        with pytest.raises(SystemExit) as x:
            T.main(argv)
        assert why in str(x.value), (argv, str(x.value))
    # the no-common-file refusal names both folders
    with pytest.raises(SystemExit) as x:
        T.main([str(a), str(b)])
    assert str(a) in str(x.value) and str(b) in str(x.value)
