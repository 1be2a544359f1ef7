"""CPU: the host side of the time alignment (buddy_amd/utils/metrics.py align) and its float64 restatement tests/_align_ref.py:
the tester's options parser, the report's columns with and without an alignment, the restatement's own properties (a shifted copy, a constructed
tie, the trimmed pair), the library's symbols, and the refusal of CPU tensors."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _align_ref as A  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import metrics as M  # noqa: E402

BASE = ["file", "samples"] + [f"{m}_{k}" for m in M.VALUES for k in ("in", "out", "delta")] + ["flags_in", "flags_out", "kept_frames", "frames"]
EXTRA = ["lag_in", "lag_out", "lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out", "align_flags_in", "align_flags_out"]


def test_align_options():
    from buddy_amd.config import compose
    from buddy_amd.testing.tester import align_options, metrics_options
    assert align_options({}) == (False, 50.0)                                             # a config written before the block existed
    assert align_options({"metrics": {"use": True}}) == (False, 50.0)
    assert align_options({"metrics": {"align": {"use": True}}}) == (True, 50.0)
    assert align_options({"metrics": {"align": {"use": True, "max_lag_ms": 12.5}}}) == (True, 12.5)
    for name in ("blind_dereverberation_BUDDy", "informed_dereverberation_DPS"):
        t = compose(tester=name).tester
        assert align_options(t) == (False, 50.0) and metrics_options(t) == (False, M.VALUES)
        assert t.metrics.align == {"use": False, "max_lag_ms": 50}
    t = compose(overrides=["tester.metrics.use=true", "tester.metrics.align.use=true", "tester.metrics.align.max_lag_ms=20"]).tester
    assert align_options(t) == (True, 20.0) and metrics_options(t) == (True, M.VALUES)
    assert align_options(compose(tester="real_dereverberation_BUDDy").tester) == (False, 50.0)
    assert M.MAX_LAG_MS == 50.0 and M.ALIGN_FLAGS == ("defined", "edge", "inverted")


def _ev(vals, alignment=None):
    args = (torch.tensor(vals, dtype=torch.float64), torch.tensor([15, 15], dtype=torch.int32), torch.tensor([40, 7], dtype=torch.int32),
            torch.tensor([45, 9], dtype=torch.int32), torch.tensor([6000, 1300], dtype=torch.int32), M.VALUES)
    return M.Evaluation(*args) if alignment is None else M.Evaluation(*args, alignment)


def _al(lags, rho, flags, fs=16000):
    return M.Alignment(torch.tensor(lags, dtype=torch.int32), torch.tensor(rho, dtype=torch.float64), torch.zeros(2, dtype=torch.float64),
                       torch.tensor(flags, dtype=torch.int32), None, None, torch.tensor([6000, 1300], dtype=torch.int32), 800, fs)


def test_report_columns_with_and_without_alignment(tmp_path):
    v = [[1.0, 0.5, 0.25, 9.0], [2.0, 0.75, 0.5, 3.0]]
    plain = M.report_rows(["a", "b"], _ev(v), _ev(v))
    assert list(plain[0]) == BASE and _ev(v).alignment is None                            # six positional arguments still build an Evaluation
    assert [s["value"] for s in M.summary_rows(plain)] == [f"{m}_{k}" for m in M.VALUES for k in ("in", "out", "delta")]
    rows = M.report_rows(["a", "b"], _ev(v, _al([0, -3], [0.5, -0.25], [1, 5])), _ev(v, _al([8, 800], [0.875, math.nan], [1, 3])))
    assert list(rows[0]) == BASE + EXTRA and [rows[0][c] for c in BASE] == [plain[0][c] for c in BASE]
    assert [rows[1][c] for c in EXTRA] == [-3, 800, -0.1875, 50.0, -0.25, rows[1]["xcorr_out"], 5, 3] and math.isnan(rows[1]["xcorr_out"])
    assert [rows[0][c] for c in EXTRA] == [0, 8, 0.0, 0.5, 0.5, 0.875, 1, 1]
    summ = M.summary_rows(rows)
    assert [s["value"] for s in summ] == [f"{m}_{k}" for m in M.VALUES for k in ("in", "out", "delta")] + ["lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out"]
    by = {s["value"]: s for s in summ}
    assert by["lag_ms_out"]["mean"] == 25.25 and by["xcorr_out"]["n"] == 1 and by["xcorr_out"]["mean"] == 0.875
    half = M.report_rows(["a", "b"], _ev(v), _ev(v, _al([8, 800], [0.875, 0.5], [1, 3])))  # the tool without --input: no alignment on the input side
    assert list(half[0]) == BASE + EXTRA and math.isnan(half[0]["lag_in"]) and math.isnan(half[0]["xcorr_in"]) and half[0]["align_flags_in"] == 0
    p = str(tmp_path / "metrics.csv")
    M.write_report(p, rows)
    assert open(p).read().splitlines()[0].split(",") == BASE + EXTRA


def test_reference_finds_the_shift_of_a_copy():
    rs = np.random.RandomState(3)
    x = rs.standard_normal(300).astype(np.float32)
    for d in (0, 1, -1, 7, -7, 12, -12):
        e = (A.shift(x, d) + 0.1 * rs.standard_normal(300)).astype(np.float32)
        got, rho, frac, flags, r = A.lag(e, x, 12)
        assert got == d and flags == (3 if abs(d) == 12 else 1) and 0.9 < rho < 1.0 and abs(frac) < 0.5, d
        got, rho, _, flags, _ = A.lag(-e, x, 12)
        assert got == d and flags == (7 if abs(d) == 12 else 5) and -1.0 < rho < -0.9, d
        et, xt = A.trim(e, x, d)
        assert len(et) == len(xt) == 300 - abs(d) and abs(np.corrcoef(et, xt)[0, 1]) > 0.9
    r, et, xt = A.xcorr(x[:40], x[:40] * 2 + 1, 45)                                       # against the definition written as two loops; K >= n
    for k in range(-45, 46):
        s = sum(et[m + k] * xt[m] for m in range(40) if 0 <= m + k < 40)
        assert abs(r[k + 45] - s) <= 1e-12 * max(1.0, abs(s))
    assert np.all(r[:6] == 0.0) and np.all(r[-6:] == 0.0) and A.peak(r, 45) == 0
    assert np.all(A.bound(x[:40], x[:40], 45)[6:-6] > 0.0) and A.bound(x[:40], x[:40], 45)[0] == 0.0


def test_reference_tie_rule_and_undefined_rows():
    assert A.peak(np.array([3.0, 1.0, 0.0, 2.0, 3.0]), 2) == 2                            # |k| equal: k >= 0
    assert A.peak(np.array([3.0, -3.0, 1.0, 0.0, 3.0]), 2) == -1                          # the smallest |k| among the largest |r|
    assert A.peak(np.array([0.0, 2.0, -2.0, 2.0, 0.0]), 2) == 0
    assert A.peak(np.zeros(5), 2) == 0
    # a constructed tie in the signals themselves: x = +1 -1 (mean 0), e = the same pulse pair at both distance 2 before and behind
    x = np.array([0, 0, 0, 0, 1, -1, 0, 0, 0, 0], np.float32)
    e = A.shift(x, 2) + A.shift(x, -2)
    d, rho, frac, flags, r = A.lag(e, x, 3)
    assert r[3 + 2] == r[3 - 2] == np.max(np.abs(r)) and d == 2 and flags == 1
    for e, x in ((np.zeros(8), np.arange(8.0)), (np.arange(8.0), np.full(8, 0.25)), ([1.0], [2.0]), ([1.0, math.inf, 0.0], [1.0, 2.0, 4.0])):
        d, rho, frac, flags, _ = A.lag(e, x, 2)
        assert (d, frac, flags) == (0, 0.0, 0) and math.isnan(rho)


def test_library_has_the_alignment_entries():
    lib = _lib.load()
    for name in ("buddy_xcorr_lag", "buddy_xcorr_lag_workspace", "buddy_align_pair", "buddy_align_tile", "buddy_align_lag_tile"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    T, Lt = lib.buddy_align_tile(), lib.buddy_align_lag_tile()
    assert T >= 64 and Lt >= 8
    one = lib.buddy_xcorr_lag_workspace(1, T, 0)
    assert one > 0 and lib.buddy_xcorr_lag_workspace(3, T, 0) == 3 * one and lib.buddy_xcorr_lag_workspace(1, T + 1, Lt) > lib.buddy_xcorr_lag_workspace(1, T, Lt)
    for bad in ((0, 100, 1), (1, 0, 1), (1, 100, -1), (1, 100, 65536), (1, 2 ** 30 + 1, 1)):
        assert lib.buddy_xcorr_lag_workspace(*bad) == -1, bad


def test_align_has_no_cpu_form():
    x = torch.zeros(1, 4096)
    with pytest.raises(_lib.BuddyHipError):
        M.align(x, x, 16000)
    with pytest.raises(_lib.BuddyHipError):
        M.evaluate(x, x, 16000, align=50)
