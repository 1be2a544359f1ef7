"""CPU: the host side of the evaluation report (buddy_amd/utils/metrics.py) and its float64 oracle tests/_metrics_ref.py: the
third-octave table, the oracle's own invariants, frame removal on an exact-zero gap, the short-signal rule, the CSV round trip, the tester's
options parser, and the refusal of CPU tensors (there is no CPU form)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _metrics_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_clean  # noqa: E402
from buddy_amd.utils import metrics as M  # noqa: E402


def test_third_octave_table():
    assert M.third_octave_bands() == R.BANDS == ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
                                                 (87, 109), (109, 138), (138, 174), (174, 219))
    assert M.third_octave_bands() is M.third_octave_bands()          # cached
    assert M.VALUES == ("si_sdr", "stoi", "estoi", "lsd") and (M.FRAME, M.HOP, M.NFFT, M.SEGMENT) == (R.FRAME, R.HOP, R.NFFT, R.SEG)
    assert [M.frames_of(n) for n in (255, 256, 383, 384)] == [R.frames_of(n) for n in (255, 256, 383, 384)] == [0, 1, 1, 2]


def test_oracle_identity_scores_one():
    x = synth_clean(0, 12000)
    s, es, fl, K, F = R.stoi(x, x, 10000)
    assert fl == 1 and abs(s - 1.0) < 1e-12 and abs(es - 1.0) < 1e-12 and K == F == R.frames_of(12000)
    v, fl = R.lsd(x, x)
    assert fl == 1 and v == 0.0


def test_oracle_si_sdr_invariances_and_product_formula():
    rs = np.random.RandomState(0)
    x = synth_clean(1, 4000)
    e = (x + 0.3 * x.std() * rs.standard_normal(4000)).astype(np.float32)
    base = R.moments(e, x)[3]
    assert abs(R.moments(2.5 * e.astype(np.float64) + 0.1, x)[3] - base) < 1e-9           # a gain and an offset on the estimate change nothing
    assert abs(base - float(M.si_sdr(torch.from_numpy(e), torch.from_numpy(x)))) < 1e-9
    ee, xx, ex, s, fl = R.moments(np.ones(5, np.float32), np.zeros(5, np.float32))      # a silent clean signal: the clamped formula, flag clear
    assert fl == 0 and xx == 0.0 and s == float(M.si_sdr(torch.ones(5), torch.zeros(5))) == -math.inf
    assert R.moments([1.0], [2.0])[4] == 0                                                # a single sample has no zero-mean content


@pytest.mark.parametrize("f0,f1", [(0, 3), (10, 14), (40, 44)])
def test_exact_zero_gap_loses_exactly_its_frames(f0, f1):
    """frames f0..f1 lie wholly inside a run of exact zeros (leading, interior, trailing: 45 frames in all); exactly they are removed"""
    L = 256 + 128 * 44
    x = synth_clean(2, L).astype(np.float64)
    x[f0 * 128:f1 * 128 + 256] = 0.0
    src = R.kept_frames(x)
    assert sorted(set(range(45)) - set(src.tolist())) == list(range(f0, f1 + 1))
    assert len(R.rebuild(x, src)) == (len(src) - 1) * 128 + 256


def test_short_signal_is_undefined():
    n = 29 * 128 + 256                                       # 30 frames at 10 kHz: the shortest signal with a segment
    x = synth_clean(3, n)
    assert R.stoi(x, x, 10000)[2] == 1
    s, es, fl, K, F = R.stoi(x[:n - 1], x[:n - 1], 10000)
    assert math.isnan(s) and math.isnan(es) and fl == 0 and K == F == 29
    assert R.evaluate(x[:200], x[:200], 10000)[1] == 0b0001 and math.isnan(R.lsd(x[:255], x[:255])[0])      # no full frame: only SI-SDR is defined


def test_csv_round_trip(tmp_path):
    nan = float("nan")

    def ev(vals, flags):
        return M.Evaluation(torch.tensor(vals, dtype=torch.float64), torch.tensor(flags, dtype=torch.int32), torch.tensor([40, 7], dtype=torch.int32),
                            torch.tensor([45, 9], dtype=torch.int32), torch.tensor([6000, 1300], dtype=torch.int32), M.VALUES)
    inp = ev([[-3.25, 0.5, 0.25, 9.0], [1.0 / 3.0, nan, nan, 2.0]], [15, 9])
    out = ev([[4.5, 0.75, 0.5, 5.0], [2.0 / 3.0, nan, nan, nan]], [15, 1])
    rows = M.report_rows(["a", "b"], inp, out)
    assert list(rows[0]) == ["file", "samples"] + [f"{m}_{k}" for m in M.VALUES for k in ("in", "out", "delta")] + ["flags_in", "flags_out", "kept_frames",
                                                                                                                    "frames"]
    assert rows[0]["si_sdr_delta"] == 7.75 and rows[0]["lsd_delta"] == -4.0 and math.isnan(rows[1]["stoi_delta"]) and math.isnan(rows[1]["lsd_delta"])
    p = str(tmp_path / "metrics.csv")
    M.write_report(p, rows)
    assert ",,," in open(p).read().splitlines()[2]           # NaN is an empty field
    back = R.read_csv(p)
    assert len(back) == 2
    for a, b in zip(rows, back):
        assert list(a) == list(b)
        for k in a:
            assert (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k], k      # repr(float) reads back exactly
    summ = M.summary_rows(rows)
    assert [s["value"] for s in summ] == [f"{m}_{k}" for m in M.VALUES for k in ("in", "out", "delta")]
    by = {s["value"]: s for s in summ}
    assert by["si_sdr_out"]["n"] == 2 and by["si_sdr_out"]["mean"] == np.mean([4.5, 2.0 / 3.0]) and by["si_sdr_out"]["std"] == np.std([4.5, 2.0 / 3.0])
    assert by["stoi_in"]["n"] == 1 and by["stoi_in"]["median"] == 0.5 and by["stoi_in"]["std"] == 0.0
    q = str(tmp_path / "metrics_summary.csv")
    M.write_report(q, summ)
    assert [r["n"] for r in R.read_csv(q)] == [s["n"] for s in summ]
    none = M.summary_rows(M.report_rows(["b"], ev([[nan] * 4] * 2, [0, 0]), ev([[nan] * 4] * 2, [0, 0])))
    assert none[0]["n"] == 0 and math.isnan(none[0]["mean"])
    assert M.summary_rows([]) == []


def test_metrics_options_default_off():
    from buddy_amd.config import compose
    from buddy_amd.testing.tester import metrics_options
    assert metrics_options({}) == (False, M.VALUES)                                       # a config written before the block existed
    assert metrics_options({"metrics": {"use": True, "values": ["stoi", "lsd"]}}) == (True, ("stoi", "lsd"))
    for name in ("blind_dereverberation_BUDDy", "informed_dereverberation_DPS"):
        assert metrics_options(compose(tester=name).tester) == (False, M.VALUES)
    assert metrics_options(compose(overrides=["tester.metrics.use=true", "tester.metrics.values=[stoi]"]).tester) == (True, ("stoi",))
    assert metrics_options(compose(tester="real_dereverberation_BUDDy").tester) == (False, M.VALUES)


def test_evaluate_has_no_cpu_form():
    x = torch.zeros(1, 4096)
    with pytest.raises(_lib.BuddyHipError):
        M.evaluate(x, x, 16000)
    lib = _lib.load()
    assert lib.buddy_metrics_tile() >= 64
    assert lib.buddy_stoi_select_workspace(2, 256 + 128 * 9) == 8 * 2 * 10 and lib.buddy_stoi_scores_workspace(3, 31) == 16 * 3 * 2
    assert lib.buddy_lsd_workspace(1, 255) == 8 and lib.buddy_stoi_select_workspace(0, 100) == -1
