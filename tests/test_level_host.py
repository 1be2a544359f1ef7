"""Host side of the active speech level (buddy_amd/utils/level.py); no GPU.  The float64 restatement of tests/_level_ref.py
against a direct transcription of the P.56 hangover-counter loop; the bracket condition on every seed the GPU tests compare count for count; the
interpolation and every flag branch of ``finish`` on hand-made counts; the scaling rule; the report's columns and summary; the argument checks."""
import csv
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _level_ref as R  # noqa: E402
from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import level as lv  # noqa: E402


def _tiles():
    lib = _lib.load()
    return int(lib.buddy_level_tile()), int(lib.buddy_level_counts_tile())


def test_restatement_equals_the_p56_counter_loop():
    """the sliding-window form of the hangover (section 23) and the standard's counter per threshold, started at I, count the same samples"""
    rs = np.random.RandomState(0)
    for trial in range(12):
        fs = [1000, 2000, 8000][trial % 3]
        n = int(rs.randint(1, 3000))
        x = R.speechlike(300 + trial, n, fs, pause=float(rs.uniform(0.1, 0.8)))
        hang = int(math.floor(0.2 * fs + 0.5)) if trial % 4 else int(rs.randint(0, 5))
        q = R.envelope(x, 0.0, fs, 0.03)
        thr = [float(np.max(np.abs(x))) * 2.0 ** (j - 15) for j in range(16)]
        assert R.counts_of(q, thr, hang) == R.counts_p56(q, thr, hang)


def test_brackets_agree_on_every_gpu_seed():
    """the cap of the count comparison: with thresholds moved by +eps and -eps the restatement counts the same, so the GPU counts must be EQUAL"""
    T, Tc = _tiles()
    worst = 0.0
    for name, (fs, rows, remove_mean) in R.gpu_cases(T, Tc).items():
        for b, x in enumerate(rows):
            res = R.level_ref(x, fs, remove_mean=remove_mean, T=T)
            assert res["counts"] is not None, (name, b)
            assert res["counts_up"] == res["counts"] == res["counts_down"], (name, b, len(x))
            worst = max(worst, res["eps"] / res["thresholds"][0])
    fs, x = R.half_peak_row(T, Tc)
    for full in (1.0, 0.5):
        res = R.level_ref(x, fs, R=full, remove_mean=False, T=T)
        assert res["counts_up"] == res["counts"] == res["counts_down"] and res["flags"] == 0 and res["js"] >= 2
    print(f"largest eps / lowest threshold over the cases: {worst:.3e}")
    assert worst < 1e-6


def _counts(active):
    """non-increasing counts from a list"""
    return list(active) + [0] * (16 - len(active))


def test_finish_interpolates_and_flags():
    n, ref, M = 10000, 1.0, 15.9
    sq = 0.01 * n                                      # rms -20 dB
    # every threshold up to j = 9 sees all samples, above that none would be natural; make the counts fall slowly instead
    a = [n] * 8 + [9000, 8000, 6000, 3000, 1000, 100, 10, 1]
    level, act, rms_db, flags = lv.finish(a, sq, n, ref, M)
    A = [10 * math.log10(sq / v) for v in a]
    D = [A[j] - 20 * math.log10(2.0 ** (j - 15)) for j in range(16)]
    js = next(j for j in range(16) if D[j] <= M)
    assert js >= 1 and D[js - 1] > M
    t = (D[js - 1] - M) / (D[js - 1] - D[js])
    assert flags == 0 and level == pytest.approx(A[js - 1] + t * (A[js] - A[js - 1]), abs=1e-12)
    assert A[js - 1] <= level <= A[js]
    assert rms_db == pytest.approx(-20.0, abs=1e-12) and act == pytest.approx(10 ** ((rms_db - level) / 10), rel=1e-14)
    mine = R.finish(a, sq, n, ref, M)
    assert mine["flags"] == 0 and mine["level_db"] == pytest.approx(level, abs=1e-12)
    # BELOW: the lowest threshold is already within the margin (a huge full scale)
    level, act, _, flags = lv.finish([n] + [0] * 15, sq, n, 1e4, M)
    assert flags == lv.BELOW and level == pytest.approx(-20.0, abs=1e-12) and act == pytest.approx(1.0, rel=1e-12)
    # BELOW and UNDEFINED: not even the lowest threshold is reached
    level, act, rms_db, flags = lv.finish([0] * 16, sq, n, 1e6, M)
    assert flags == lv.BELOW | lv.UNDEFINED and math.isnan(level) and math.isnan(act) and rms_db == pytest.approx(-20.0, abs=1e-12)
    # ABOVE: no threshold within the margin (a tiny full scale)
    level, _, _, flags = lv.finish([n] * 15 + [n // 2], sq, n, 1e-3, M)
    assert flags == lv.ABOVE and level == pytest.approx(10 * math.log10(sq / (n // 2)), abs=1e-12)
    # EDGE: the level is far above threshold j* - 1 and threshold j* has no active sample (a signal of high crest factor)
    a = _counts([n] * 10)
    level, _, _, flags = lv.finish(a, sq, n, 1.0, M)
    assert -20.0 - 20 * math.log10(2.0 ** (9 - 15)) > M
    assert flags == lv.EDGE and level == pytest.approx(-20.0, abs=1e-12)
    # UNDEFINED: no sample, no energy, a sum that is not finite
    for args in ((a, sq, 0, 1.0), (a, 0.0, n, 1.0), (a, float("nan"), n, 1.0), (a, float("inf"), n, 1.0), (a, sq, n, float("nan"))):
        level, act, rms_db, flags = lv.finish(*args, M)
        assert flags == lv.UNDEFINED and math.isnan(level) and math.isnan(act) and math.isnan(rms_db)
    for f, text in ((0, ""), (lv.EDGE, "EDGE"), (lv.BELOW | lv.UNDEFINED, "BELOW|UNDEFINED"), (lv.ABOVE, "ABOVE")):
        assert lv.flag_text(f) == text


def test_active_gain_is_the_std_rule_at_the_reference_activity():
    """active_rms^2 = (sq / n) / activity, so at activity == reference_activity the rule divides by the row's rms: the std rule's scale for a
    zero-mean row, up to torch's unbiased sqrt(n / (n - 1))"""
    rs = np.random.RandomState(3)
    n = 20000
    y = rs.standard_normal(n) * 0.1
    y -= y.mean()
    sq = float(np.sum(y * y))
    for activity in (0.3, 0.62, 1.0):
        level_db = 10 * math.log10(sq / n) - 10 * math.log10(activity)
        g = lv.active_gain(1.5, 0.05, 10.0 ** (level_db / 20.0), activity)
        assert g == pytest.approx(1.5 * 0.05 / math.sqrt(sq / n), rel=1e-13)
        std = float(torch.from_numpy(y).std())
        assert g == pytest.approx(1.5 * 0.05 / std * math.sqrt(n / (n - 1.0)), rel=1e-12)
    # a row with half the reference's activity at the same active level gets the same g: its std is lower by sqrt(2), its scale is not
    assert lv.active_gain(1.0, 0.05, 0.1, 0.5) == pytest.approx(0.05 / (0.1 * math.sqrt(0.5)), rel=1e-15)


def test_level_options():
    assert lv.level_options({}) == ("std", None)
    assert lv.level_options({"level": "std", "reference_activity": None}) == ("std", None)
    assert lv.level_options({"level": "active", "reference_activity": 0.6}) == ("active", 0.6)
    with pytest.raises(ValueError, match=r"tools/speech_level\.py --segment-seconds"):
        lv.level_options({"level": "active", "reference_activity": None})
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="reference_activity"):
            lv.level_options({"level": "active", "reference_activity": bad})
    with pytest.raises(ValueError, match="'std' or 'active'"):
        lv.level_options({"level": "loud"})


def test_config_ships_std_and_no_reference_activity():
    from buddy_amd.config import compose
    rr = compose(tester="real_dereverberation_BUDDy").tester.real_recordings
    assert rr.level == "std" and rr.reference_activity is None
    assert lv.level_options(rr) == ("std", None)


def test_argument_checks():
    with pytest.raises(_lib.BuddyHipError, match="MI355X only"):
        lv.speech_level(torch.zeros(1, 100), 16000)
    ok = dict(fs=16000, full_scale="peak", margin_db=15.9, time_constant=0.03, hangover=0.2, rows=2)
    fs, ref, hang = lv.check_arguments(**ok)
    assert (fs, ref, hang) == (16000.0, None, 3200)
    assert lv.hangover_samples(0.2, 48000) == 9600 and lv.hangover_samples(0.2, 1000) == 200 and lv.hangover_samples(0.0, 8000) == 0
    assert lv.hangover_samples(0.00025, 2000) == 1      # floor(0.5 + 0.5)
    assert lv.check_arguments(**dict(ok, full_scale=1.0))[1].tolist() == [1.0, 1.0]
    assert lv.check_arguments(**dict(ok, full_scale=torch.tensor([0.5, 2.0])))[1].tolist() == [0.5, 2.0]
    for key, bad in (("fs", 0), ("fs", float("nan")), ("fs", -8000), ("margin_db", float("inf")), ("time_constant", 0.0), ("time_constant", -1.0),
                     ("hangover", -0.1), ("hangover", float("nan")), ("full_scale", "rms"), ("full_scale", 0.0), ("full_scale", -1.0),
                     ("full_scale", float("nan")), ("full_scale", [1.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            lv.check_arguments(**dict(ok, **{key: bad}))


def _fake(level, activity, rms, peak, flags):
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)      # noqa: E731
    return lv.SpeechLevel(f64(level), f64(activity), 10.0 ** (f64(level) / 20.0), f64(rms), f64(peak), torch.zeros(len(level), 16, dtype=torch.int64),
                          torch.tensor(flags, dtype=torch.int32), torch.tensor([100] * len(level), dtype=torch.int32))


def test_report_columns_and_summary(tmp_path):
    nan = float("nan")
    res = _fake([-20.0, -26.0, nan, -23.0], [0.5, 0.7, nan, 0.6], [-23.0, -27.5, nan, -25.2], [0.9, 0.4, 1.0, 0.5], [0, 0, lv.UNDEFINED, lv.EDGE])
    rows = lv.report_rows(["a", "b", "c", "d"], res, [{"rule": "active", "g": 0.5}] * 4)
    assert list(rows[0]) == ["file", "samples", "level_db", "activity", "rms_db", "peak", "flags", "rule", "g"]
    assert rows[2]["flags"] == "UNDEFINED" and rows[3]["flags"] == "EDGE" and rows[0]["flags"] == ""
    summary = lv.summary_rows(rows)
    assert [s["value"] for s in summary] == ["level_db", "activity", "rms_db-level_db"]
    assert [s["n"] for s in summary] == [3, 3, 3]
    assert summary[1]["median"] == 0.6 and summary[0]["mean"] == pytest.approx(-23.0) and summary[0]["std"] == pytest.approx(np.std([-20.0, -26.0, -23.0]))
    assert summary[2]["median"] == pytest.approx(-2.2)
    assert len(lv.format_summary(summary).splitlines()) == 3
    p = tmp_path / "levels.csv"
    lv.write_report(str(p), rows)
    with open(p, newline="") as f:
        got = list(csv.reader(f))
    assert got[0] == ["file", "samples", "level_db", "activity", "rms_db", "peak", "flags", "rule", "g"] and len(got) == 5
    assert got[3][2] == "" and got[1][2] == repr(-20.0)      # NaN is an empty field
    assert lv.summary_rows([])[0]["n"] == 0


def test_tool_reads_files_folders_and_segments(tmp_path):
    import importlib.util
    import os
    from scipy.io import wavfile
    spec = importlib.util.spec_from_file_location("speech_level_tool", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "speech_level.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rs = np.random.RandomState(0)
    d = tmp_path / "wavs" / "sub"
    d.mkdir(parents=True)
    wavfile.write(d / "b.wav", 8000, (rs.standard_normal((2500, 2)) * 3000).astype(np.int16))      # two channels, int16
    wavfile.write(tmp_path / "wavs" / "a.wav", 8000, (0.1 * rs.standard_normal(1999)).astype(np.float32))
    paths = tool.wav_paths([str(tmp_path / "wavs")])
    assert [os.path.basename(p) for p in paths] == ["a.wav", "b.wav"]
    rows = tool.read_rows(paths, None, None, "cpu")
    assert [(r[0], r[1].numel(), r[2]) for r in rows] == [("a", 1999, 8000), ("b", 2500, 8000)]
    assert rows[1][1].dim() == 1 and float(rows[1][1].abs().max()) <= 1.0      # mixed down, scaled by the format's full scale
    rows = tool.read_rows(paths, 0.1, None, "cpu")                              # full segments of 800 samples, the rest dropped
    assert [r[0] for r in rows] == ["a#0", "a#1", "b#0", "b#1", "b#2"] and all(r[1].numel() == 800 for r in rows)
    (tmp_path / "empty").mkdir()
    with pytest.raises(SystemExit):
        tool.wav_paths([str(tmp_path / "empty")])
