"""Host: the float64 restatement of the blind decay time (tests/_decay_ref.py) meets the functional condition on its own --
before the GPU tests lean on it -- and the host pieces of buddy_amd/utils/decay.py: bin ranges, flags, report rows, option parsing for old configs."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _decay_ref as R  # noqa: E402
from _srmr_ref import read_csv  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import decay as D  # noqa: E402

NOMINAL = (0.2, 0.3, 0.5, 0.7, 1.0)


@pytest.mark.parametrize("seed", range(6))
def test_restatement_meets_the_functional_condition(seed):
    """gated bursts through an exponentially decaying response: the broadband decay time within 15 % of the nominal one from at least 6 regions, at
    0.2 .. 1.0 s; the dry source reads below 0.2 s"""
    for t60 in NOMINAL:
        r = R.decay_times(R.reverberant(seed, t60))
        print(f"seed {seed} T60 {t60}: {r['t60'][0]:.4f} s from {r['regions'][0]} regions, flags {r['flags'][0]}")
        assert abs(r["t60"][0] / t60 - 1.0) <= 0.15 and r["regions"][0] >= 6 and r["flags"][0] == R.DEFINED, (seed, t60, r["t60"][0], r["regions"][0])
        assert r["q1"][0] <= r["t60"][0] <= r["q3"][0]
    dry = R.decay_times(R.burst_source(seed))
    print(f"seed {seed} dry: {dry['t60'][0]:.4f} s from {dry['regions'][0]} regions")
    assert dry["t60"][0] < 0.2 and dry["regions"][0] >= 1


def test_bin_ranges_and_flags():
    lo, hi, above = D.bin_ranges(16000)
    assert (lo, hi) == ([3, 3, 6, 12, 23, 46, 91], [182, 6, 12, 23, 46, 91, 182]) and not any(above)
    assert [(a, b) for a, b, _ in R.bands(16000)] == list(zip(lo, hi))                   # the restatement lists the bins one by one
    assert lo[1:] + [hi[-1]] == [lo[1]] + hi[1:] and lo[0] == lo[1] and hi[0] == hi[-1]  # the octaves tile the broadband range
    for fs in (8000, 11025, 12571, 12572, 22050, 48000):
        lo, hi, above = D.bin_ranges(fs)
        assert [(a, b, c) for a, b, c in R.bands(fs)] == list(zip(lo, hi, above)), fs
        assert above == [False] * 6 + [fs * 0.45 < 4000 * math.sqrt(2.0)], fs
    lo, hi, above = D.bin_ranges(8000)
    assert (lo[0], hi[0]) == (3, 116) and (lo[6], hi[6]) == (0, 0) and 115 * 31.25 < 3600.0 <= 116 * 31.25
    assert D.band_edges(8000)[0][1] == 3600.0 and D.band_edges(48000)[0][1] == 5656.85
    assert D.flag_word(0, 100, False, 6) == D.FEW and D.flag_word(1, 100, False, 6) == D.DEFINED | D.FEW and D.flag_word(3, 100, False, 6) == D.DEFINED
    assert D.flag_word(0, 10, True, 6) == D.FEW | D.ABOVE_RATE | D.SHORT and D.flag_word(0, 11, False, 6) == D.FEW
    assert [D.frames_of(n) for n in (511, 512, 639, 640)] == [0, 1, 1, 2] == [R.frames_of(n) for n in (511, 512, 639, 640)]


def test_restatement_regions_on_crafted_energies():
    """the crafted cases of the GPU test keep the regions they are built to keep: ties, runs to the last frame and across the tile, the whole row,
    the shortest rows, the floor, a drop exactly on S[m0] q, 1 to 4 regions"""
    cases = R.crafted_cases(256)
    assert len(cases) >= 25
    for name, E, q, want in cases:
        r = R.regions(E, q)
        assert [(v[0], v[1]) for v in r] == want, name
        assert all(v[2] > 0.0 and v[3] >= 1.0 for v in r), name
    e = 10.0 ** (-0.5 * np.arange(60.0) / 10.0)                                          # an exact exponential, 0.5 dB per frame: its decay time to 1e-12
    (m0, n, T, cond), = R.regions(e, 0.1)
    assert (m0, n) == (0, 56) and abs(T / (60.0 / 0.5 * 128 / 16000) - 1.0) < 1e-12
    assert all(math.isnan(v) for v in R.select([]))
    assert R.select([3.0]) == (3.0, 3.0, 3.0) and R.select([2.0, 1.0]) == (1.0, 1.0, 1.0)
    assert R.select([3.0, 1.0, 2.0]) == (2.0, 1.0, 2.0) and R.select([4.0, 3.0, 1.0, 2.0]) == (2.0, 1.0, 3.0)
    assert R.select([5.0, 4.0, 3.0, 1.0, 2.0]) == (3.0, 2.0, 4.0)


def test_restatement_short_and_silent_rows():
    for n, M in ((511, 0), (512, 1), (1024, 5), (1663, 9), (1664, 10), (1792, 11)):
        r = R.decay_times(np.random.RandomState(n).standard_normal(n))
        assert R.frames_of(n) == M and [bool(f & R.SHORT) for f in r["flags"]] == [M < 11] * 7, n
        assert M >= 11 or (r["regions"] == [0] * 7 and all(math.isnan(v) for v in r["t60"])), n
    z = R.decay_times(np.zeros(16000))
    assert z["regions"] == [0] * 7 and all(math.isnan(v) for v in z["t60"]) and z["flags"] == [R.FEW] * 7
    r8 = R.decay_times(R.reverberant(0, 0.5), fs=8000)
    assert r8["flags"][6] == R.FEW | R.ABOVE_RATE and r8["regions"][6] == 0 and r8["flags"][0] & R.DEFINED


def _scored(t, n, frames=100, samples=16000, flags=1):
    return {"t60": [t + 0.01 * k for k in range(7)], "q1": [t - 0.05] * 7, "q3": [t + 0.125] * 7, "regions": [n] * 7, "flags": [flags] * 7, "frames": frames,
            "samples": samples}


def test_csv_round_trip(tmp_path):
    nan = float("nan")
    none = {"t60": [nan] * 7, "q1": [nan] * 7, "q3": [nan] * 7, "regions": [0] * 7, "flags": [D.FEW | D.SHORT] * 7, "frames": 3, "samples": 900}
    inp, out = [_scored(0.71, 12), none], [_scored(0.24, 9, frames=371, samples=48000), none]
    rows = D.report_rows(["a", "b"], inp, out)
    bands = ["", "_125", "_250", "_500", "_1000", "_2000", "_4000"]
    cols = (["file", "samples_in", "samples_out", "frames_in", "frames_out"] + [f"t60{b}_{s}" for b in bands for s in ("in", "out", "delta")]
            + [f"{c}{b}_{s}" for c in ("regions", "spread", "flags") for b in bands for s in ("in", "out")])
    assert list(rows[0]) == cols
    assert rows[0]["t60_in"] == 0.71 and rows[0]["t60_out"] == 0.24 and rows[0]["t60_delta"] == 0.24 - 0.71 and rows[0]["t60_4000_out"] == 0.24 + 0.06
    assert rows[0]["spread_in"] == (0.71 + 0.125) - (0.71 - 0.05) and rows[0]["regions_500_out"] == 9 and math.isnan(rows[1]["t60_delta"])
    paired = D.report_rows(["a", "b"], inp, out, clean=out)
    assert list(paired[0]) == cols + [f"t60{b}_clean" for b in bands] + [f"regions{b}_clean" for b in bands] and paired[0]["t60_250_clean"] == 0.24 + 0.02
    alone = D.report_rows(["a"], None, out[:1])                                          # no input signal: those columns stay empty
    assert math.isnan(alone[0]["t60_in"]) and math.isnan(alone[0]["t60_delta"]) and alone[0]["t60_out"] == 0.24 and alone[0]["flags_in"] == 0
    p = str(tmp_path / "decay.csv")
    D.write_report(p, rows)
    assert open(p).read().splitlines()[2].startswith("b,900,900,3,3,,,,")                # NaN is an empty field
    back = read_csv(p)
    assert len(back) == 2
    for a, b in zip(rows, back):
        assert list(a) == list(b)
        for k in a:
            assert (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k], k      # repr(float) reads back exactly
    summ = D.summary_rows(paired)
    assert [s["value"] for s in summ] == [c for c in paired[0] if c.startswith("t60")]
    by = {s["value"]: s for s in summ}
    assert by["t60_out"]["n"] == 1 and by["t60_out"]["mean"] == by["t60_out"]["median"] == 0.24 and by["t60_out"]["std"] == 0.0
    assert D.summary_rows([]) == [] and "t60_in" in D.format_summary(summ)
    # tools/compare.py reads the report: the decay times and the spreads are score columns, the counts and the flag words are not
    from buddy_amd.utils import compare
    both = D.report_rows(["a", "c"], [inp[0]] * 2, [out[0], _scored(0.3, 7)])
    D.write_report(p, both)
    labels = compare.compare_reports(p, p)["labels"]
    assert "t60_out" in labels and "t60_1000_delta" in labels and "spread_out" in labels
    assert not [c for c in labels if c.startswith(("regions", "flags", "frames", "samples"))]
    import importlib.util
    spec = importlib.util.spec_from_file_location("buddy_tools_compare", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "compare.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert "decay" in tool.REPORTS


def test_decay_options_default_off():
    from buddy_amd.config import compose
    from buddy_amd.testing.tester import decay_options
    assert decay_options({}) is False                                                    # a config written before the block existed
    assert decay_options({"decay": {"use": True}}) is True and decay_options({"decay": {}}) is False
    conf = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conf", "tester")
    shipped = sorted(f[:-5] for f in os.listdir(conf) if f.endswith(".yaml"))
    assert len(shipped) >= 4
    for name in shipped:
        assert decay_options(compose(tester=name).tester) is False, name
    for name in ("real_dereverberation_BUDDy", "blind_dereverberation_BUDDy", "informed_dereverberation_DPS"):
        assert decay_options(compose(tester=name, overrides=["tester.decay.use=true"]).tester) is True


def test_decay_has_no_cpu_form():
    with pytest.raises(_lib.BuddyHipError):
        D.decay_times(torch.zeros(1, 8192), 16000)
    lib = _lib.load()
    assert lib.buddy_decay_regions_tile() >= 64 and lib.buddy_decay_regions_tile() % 64 == 0
    assert (D.FRAME, D.HOP, D.K_SMOOTH) == (R.FRAME, R.HOP, R.K)
