"""CPU: the host side of the SRMR report (buddy_amd/utils/srmr.py) and its float64 restatement tests/_srmr_ref.py: the two
banks, the restatement's own invariants (gain, reverberation ordering, the band limit, the frame edges), the score rule on given energies, the CSV
round trip, the tester's options parser, and the refusal of CPU tensors (there is no CPU form)."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy import signal

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _srmr_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_rir  # noqa: E402
from buddy_amd.utils import srmr as S  # noqa: E402

LENGTHS = [57, 65, 75, 86, 98, 112, 129, 148, 169, 194, 222, 255, 292, 335, 384, 440, 504, 578, 663, 760, 872, 999, 1146]


def test_gammatone_bank():
    bank = S.gammatone_bank()
    assert bank is S.gammatone_bank()                                                    # cached
    assert bank.centres.shape == (23,) and abs(bank.centres[0] - 6947.845) < 1e-3 and abs(bank.centres[-1] - 125.0) < 1e-9
    assert np.all(np.diff(bank.centres) < 0)
    assert list(bank.lengths) == LENGTHS and sum(bank.lengths) == 8583
    n_all = np.arange(max(LENGTHS))
    for cf, g in zip(bank.centres, bank.taps):
        assert g.dtype == np.complex128 and g[0] == 0.0
        assert abs(abs(np.sum(g * np.exp(-2j * np.pi * cf * n_all[:len(g)] / 16000.0))) - 1.0) < 1e-12      # unit gain at the centre
    # the restatement designs the same bank on its own
    assert np.abs(bank.centres - R.centres()).max() < 1e-9
    assert [len(g) for g in R.taps()] == LENGTHS
    assert max(np.abs(a - b).max() for a, b in zip(bank.taps, R.taps())) < 1e-14
    assert np.allclose(S.erb(bank.centres), R.erb(R.centres()), rtol=1e-14) and abs(float(S.erb(125.0)) - 38.19) < 5e-3


def test_modulation_bank():
    mod = S.modulation_bank()
    assert mod is S.modulation_bank()
    assert np.allclose(mod.centres, [4, 6.5627, 10.7672, 17.6654, 28.9832, 47.5518, 78.0169, 128], atol=5e-5)
    assert np.allclose(mod.lower_edges, [3.1231, 5.1240, 8.4068, 13.7928, 22.6294, 37.1273, 60.9137, 99.9394], atol=5e-5)
    assert mod.coef.shape == (8, 6) and np.all(mod.coef[:, 3] == 1.0) and np.all(mod.coef[:, 1] == 0.0) and np.all(mod.coef[:, 0] == -mod.coef[:, 2])
    for k, (b, a) in enumerate(R.modulation_filters()):
        assert np.abs(mod.coef[k, :3] - b).max() < 1e-18 and np.abs(mod.coef[k, 3:] - a).max() < 1e-15
        w, h = signal.freqz(b, a, worN=[2 * np.pi * mod.centres[k] / 16000.0])
        assert abs(abs(h[0]) - 1.0) < 1e-9                                               # a band-pass with unit gain at its centre
    assert (S.WINDOW, S.HOP) == (R.W, R.H) == (4096, 1024)
    assert [S.frames_of(n) for n in (4095, 4096, 5119, 5120)] == [R.frames_of(n) for n in (4095, 4096, 5119, 5120)] == [0, 1, 1, 2]
    h = R.window()
    assert np.allclose(h, np.hamming(4098)[1:-1], atol=1e-15)                            # the interior of a 4098-point Hamming window


def test_restatement_gain_invariance():
    x = R.speechlike(0, 64000)
    s = R.srmr(x)["srmr"]
    assert abs(s - 4.49) < 5e-3
    rel = abs(R.srmr(3.7 * x)["srmr"] / s - 1.0)
    print(f"gain 3.7: relative change {rel:.2e}")
    assert rel < 1e-12


@pytest.mark.parametrize("u,want", [(0, (4.49, 4.28, 3.12, 1.81, 1.04)), (1, (4.39, 3.71, 2.68, 1.71, 1.11))])
def test_restatement_falls_with_reverberation(u, want):
    L = 64000
    x = R.speechlike(u, L)
    got = [R.srmr(x)["srmr"]]
    for t60 in (0.2, 0.4, 0.8, 1.6):
        y = signal.fftconvolve(x, synth_rir(u, taps=int(1.2 * t60 * 16000) + 1000, t60=t60).astype(np.float64))[:L]
        got.append(R.srmr(y)["srmr"])
    print(f"u {u}: dry, t60 0.2 0.4 0.8 1.6 -> " + " ".join(f"{v:.4f}" for v in got))
    assert all(a > b for a, b in zip(got, got[1:]))                                      # strictly falling
    assert np.allclose(got, want, atol=6e-3)


@pytest.mark.parametrize("fc,kstar,bw", [(300, 6, 57.6), (500, 7, 75.7), (3000, 8, 172.0)])
def test_restatement_band_limit(fc, kstar, bw):
    b, a = signal.butter(8, fc / 8000.0)
    r = R.srmr(signal.lfilter(b, a, R.speechlike(0, 24000)))
    assert r["flag"] == 1 and r["kstar"] == kstar and abs(r["bw"] - bw) < 0.05


def test_restatement_frame_edges():
    x = R.speechlike(0, 24000)
    r = {L: R.srmr(x[:L]) for L in (4095, 4096, 5119, 5120)}
    assert r[4095]["frames"] == 0 and math.isnan(r[4095]["srmr"]) and r[4095]["flag"] == 0
    assert r[4096]["frames"] == r[5119]["frames"] == 1 and r[5120]["frames"] == 2
    assert abs(r[5119]["srmr"] / r[4096]["srmr"] - 1.0) < 1e-12                          # samples behind the last full frame change nothing
    assert r[5120]["srmr"] != r[4096]["srmr"] and r[5120]["flag"] == 1


def test_score_rule_on_given_energies():
    """every branch of K* through a chosen erb / lower-edge table, the strict > 0.9 on an exact tie, and the undefined cases"""
    low = np.array([3.0, 5.0, 8.0, 14.0, 23.0, 37.0, 61.0, 100.0])
    erbs = np.array([30.0, 50.0, 80.0, 120.0])                                           # ascending channels: K* 5, 6, 7, 8 when they close the 90 %
    for j, ks in enumerate((5, 6, 7, 8)):
        ebar = np.full((4, 8), 1e-3)
        ebar[j] = 1.0                                                                    # channel j holds nearly all the energy
        s, k, bw, fl = R.scores(ebar, 3, erbs, low)
        assert (k, bw, fl) == (ks, erbs[j], 1)
        assert abs(s - ebar[:, :4].sum() / ebar[:, 4:ks].sum()) < 1e-12 * s
    tie = np.zeros((4, 8))
    tie[0, 0], tie[1, 4] = 9.0, 1.0                                                      # running sum 9 = 0.9 * 10 exactly: not strictly above
    assert 0.9 * 10.0 == 9.0
    assert R.scores(tie, 1, erbs, low)[1:3] == (6.0, 50.0)
    tie[0, 0] = 9.0000001
    assert R.scores(tie, 1, erbs, low)[1:3] == (5.0, 30.0)
    lowonly = np.zeros((4, 8))
    lowonly[:, :4] = 1.0                                                                 # no energy in bands 4..K* - 1: a zero denominator
    s, k, bw, fl = R.scores(lowonly, 2, erbs, low)
    assert math.isnan(s) and fl == 0 and (k, bw) == (8.0, 120.0)
    assert R.scores(np.zeros((4, 8)), 2, erbs, low)[3] == 0 and math.isnan(R.scores(np.zeros((4, 8)), 2, erbs, low)[1])
    assert R.scores(np.ones((4, 8)), 0, erbs, low)[3] == 0
    # with the real bank erb(125 Hz) is above the lower edge of band 5: K* is never 5 on a signal
    assert float(R.erb(125.0)) > R.modulation_lower_edges()[5]


def test_csv_round_trip(tmp_path):
    nan = float("nan")
    inp = [dict(srmr=1.0 / 3.0, kstar=6, bw=57.25, flags=1, frames=12, samples=16000), dict(srmr=nan, kstar=0, bw=nan, flags=0, frames=0, samples=900)]
    out = [dict(srmr=2.0 / 3.0, kstar=8, bw=172.5, flags=1, frames=56, samples=48000), dict(srmr=nan, kstar=0, bw=nan, flags=0, frames=0, samples=2700)]
    rows = S.report_rows(["a", "b"], inp, out)
    cols = ["file", "samples_in", "samples_out", "srmr_in", "srmr_out", "srmr_delta", "kstar_in", "kstar_out", "bw_in", "bw_out", "flags_in", "flags_out",
            "frames_in", "frames_out"]
    assert list(rows[0]) == cols
    assert rows[0]["srmr_delta"] == 2.0 / 3.0 - 1.0 / 3.0 and math.isnan(rows[1]["srmr_delta"])
    paired = S.report_rows(["a", "b"], inp, out, clean=out)
    assert list(paired[0]) == cols + ["srmr_clean", "kstar_clean", "bw_clean"] and paired[0]["srmr_clean"] == 2.0 / 3.0
    alone = S.report_rows(["a"], None, out[:1])                                          # no input signal: those columns stay empty
    assert math.isnan(alone[0]["srmr_in"]) and math.isnan(alone[0]["srmr_delta"]) and alone[0]["srmr_out"] == 2.0 / 3.0
    p = str(tmp_path / "srmr.csv")
    S.write_report(p, rows)
    assert open(p).read().splitlines()[2] == "b,900,2700,,,,0,0,,,0,0,0,0"                 # NaN is an empty field
    back = R.read_csv(p)
    assert len(back) == 2
    for a, b in zip(rows, back):
        assert list(a) == list(b)
        for k in a:
            assert (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k], k      # repr(float) reads back exactly
    summ = S.summary_rows(paired)
    assert [s["value"] for s in summ] == ["srmr_in", "srmr_out", "srmr_delta", "srmr_clean"]
    by = {s["value"]: s for s in summ}
    assert by["srmr_out"]["n"] == 1 and by["srmr_out"]["mean"] == by["srmr_out"]["median"] == 2.0 / 3.0 and by["srmr_out"]["std"] == 0.0
    both = S.summary_rows(S.report_rows(["a", "c"], inp[:1] * 2, [out[0], dict(out[0], srmr=1.5)]))
    assert both[1]["n"] == 2 and both[1]["mean"] == float(np.mean([2.0 / 3.0, 1.5])) and both[1]["std"] == float(np.std([2.0 / 3.0, 1.5]))
    q = str(tmp_path / "srmr_summary.csv")
    S.write_report(q, summ)
    assert [r["n"] for r in R.read_csv(q)] == [s["n"] for s in summ]
    none = S.summary_rows(S.report_rows(["b"], inp[1:], out[1:]))
    assert none[0]["n"] == 0 and math.isnan(none[0]["mean"])
    assert S.summary_rows([]) == []


def test_srmr_options_default_off():
    from buddy_amd.config import compose
    from buddy_amd.testing.tester import srmr_options
    assert srmr_options({}) is False                                                     # a config written before the block existed
    assert srmr_options({"srmr": {"use": True}}) is True and srmr_options({"srmr": {}}) is False
    conf = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conf", "tester")
    shipped = sorted(f[:-5] for f in os.listdir(conf) if f.endswith(".yaml"))
    assert len(shipped) >= 4
    for name in shipped:
        assert srmr_options(compose(tester=name).tester) is False, name
    assert srmr_options(compose(tester="real_dereverberation_BUDDy", overrides=["tester.srmr.use=true"]).tester) is True


def test_srmr_has_no_cpu_form():
    x = torch.zeros(1, 8192)
    with pytest.raises(_lib.BuddyHipError):
        S.srmr(x, 16000)
    lib = _lib.load()
    assert lib.buddy_srmr_tile() >= 64 and lib.buddy_srmr_tile() % 4 == 0
    assert S.HOP % lib.buddy_modulation_chunk() == 0
