"""CPU: the host side of the spectral distortion report (buddy_amd/utils/spectral.py): the mel table, the frame rule, the invariants
of the float64 restatement tests/_spectral_ref.py, the CSV writers and the options parser."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spectral_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import spectral as S  # noqa: E402

PEAK_BINS = [3, 5, 8, 12, 15, 20, 24, 30, 35, 42, 49, 57, 65, 75, 86, 98, 111, 126, 142, 161, 181, 203, 228]


def test_mel_bands():
    M = S.mel_bands()
    assert M.shape == (23, 257) and M.dtype == np.float64 and not M.flags.writeable and S.mel_bands() is M      # designed once
    assert np.all(M >= 0.0) and np.all(M <= 1.0) and np.all(M.sum(axis=1) > 0.0)
    assert M.argmax(axis=1).tolist() == PEAK_BINS
    f = np.arange(257) * 31.25
    # the centre of a triangle is where its two flanks meet: recovered from the two bins either side of the peak, which lie on one flank each
    top = 2595.0 * math.log10(1.0 + 8000.0 / 700.0)
    centre = lambda j: 700.0 * (10.0 ** ((j + 1) * top / 24.0 / 2595.0) - 1.0)
    assert abs(centre(0) - 77.4973614726905) < 1e-9 and abs(centre(22) - 7132.824009157633) < 1e-8
    for j in (0, 22):
        lo, c, hi = (centre(j - 1) if j else 0.0), centre(j), (centre(j + 1) if j < 22 else 8000.0)
        want = np.maximum(0.0, np.minimum((f - lo) / (c - lo), (hi - f) / (hi - c)))
        assert np.abs(M[j] - want).max() < 1e-12, j
    assert M[0, 0] == 0.0 and abs(M[22, 256]) < 1e-12                                     # the outer feet sit on 0 Hz and 8 kHz
    assert np.abs(M - R.mel_bands()).max() < 1e-12                                        # the oracle designs its own
    # neighbouring triangles share their feet: between the first and the last centre the rows sum to one
    inside = (f >= centre(0)) & (f <= centre(22))
    assert np.abs(M.sum(axis=0)[inside] - 1.0).max() < 1e-12


def test_frames_of():
    assert [S.frames_of(n) for n in (1, 399, 400, 559, 560, 719, 720, 12000, 7777)] == [0, 0, 1, 1, 2, 2, 3, 73, 47]
    assert all(S.frames_of(n) == R.frames_of(n) for n in range(1, 2000, 7))
    assert (S.FS, S.FRAME, S.HOP, S.NFFT, S.BINS, S.LPC_ORDER, S.VALUES) == (16000, 400, 160, 512, 257, 12, ("cd", "llr", "fwsegsnr"))
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, 401) / 401.0)                        # the interior of a 402-point Hann window
    assert np.array_equal(w, np.hanning(402)[1:-1]) or np.abs(w - np.hanning(402)[1:-1]).max() < 1e-15
    assert abs(S._window_energy() - float(np.sum(w * w))) < 1e-12 and np.abs(R.WINDOW - w).max() < 1e-15


def test_restatement_identical_and_scaled():
    x = R.ar_noise(1, 6000)
    v, fl, F, nl, ns = R.evaluate(x, x, 16000)
    assert fl == 7 and F == 36 and abs(v[0]) <= 1e-12 and abs(v[1]) <= 1e-12 and abs(v[2] - 35.0) <= 1e-12
    es, xs = R.pairs()
    for e, x in zip(es[:2], xs[:2]):
        a, b = R.evaluate(e.astype(np.float64), x, 16000), R.evaluate(3.0 * e.astype(np.float64), x, 16000)
        assert np.abs(a[0] - b[0]).max() <= 1e-10 and a[1:] == b[1:], (a, b)
        assert a[0][0] > 0.5 and a[0][1] > 1e-3 and a[0][2] < 30.0                       # the pairs are distorted: the invariance is not vacuous


def test_restatement_gap_and_short_rows():
    es, xs = R.pairs()
    lo, hi = R.GAP
    zero = [f for f in range(R.frames_of(12000)) if f * R.HOP >= lo and f * R.HOP + R.FRAME <= hi]
    assert zero == [19, 20, 21, 22]
    for e, x, n in zip(es[:2], xs[:2], (73, 47)):
        assert not x[lo:hi].any() and not e[lo:hi].any() and x[lo - 1] != 0.0 and x[hi] != 0.0
        v, fl, F, nl, ns = R.evaluate(e, x, 16000)
        assert fl == 7 and F == n and nl == ns == n - len(zero)
    x = xs[0].copy()
    x[lo:hi] = xs[1][lo:hi] + 1e-3                                                        # without the gap every frame counts
    assert R.evaluate(x, x, 16000)[2:] == (73, 73, 73)
    x = R.ar_noise(2, 400)
    v, fl, F, nl, ns = R.evaluate(x[:399], x[:399], 16000)
    assert fl == 0 and (F, nl, ns) == (0, 0, 0) and np.isnan(v).all()
    v, fl, F, nl, ns = R.evaluate(x, x, 16000)
    assert fl == 7 and (F, nl, ns) == (1, 1, 1) and abs(v[2] - 35.0) <= 1e-12
    v, fl, F, nl, ns = R.evaluate(x, np.zeros(400), 16000)                                # a clean signal without power: nothing is defined
    assert fl == 0 and (F, nl, ns) == (1, 0, 0)


def test_restatement_levinson():
    """the recursion against the normal equations solved directly, and the quadratic form a R a = the prediction error"""
    x = R.framed(R.ar_noise(3, 400))[0]
    r = R.autocorr(x)
    a, err = R.levinson(r)
    i = np.arange(R.ORDER + 1)
    T = r[np.abs(i[:, None] - i[None, :])]
    want = np.concatenate([[1.0], np.linalg.solve(T[1:, 1:], -r[1:])])
    assert np.abs(a - want).max() < 1e-9 and abs(a @ T @ a - err) < 1e-9 * r[0] and 0.01 < err / r[0] < 0.5


def _evaluation(vals, flags, frames, nl, ns, samples, names=S.VALUES, alignment=None):
    t = lambda v, dt: torch.as_tensor(v, dtype=dt)
    i32 = torch.int32
    return S.SpectralEvaluation(t(vals, torch.float64), t(flags, i32), t(frames, i32), t(nl, i32), t(ns, i32), t(samples, i32), names, alignment)


def test_csv_round_trip(tmp_path):
    from buddy_amd.utils.metrics import Alignment
    nan = float("nan")
    inp = _evaluation([[4.0 / 3.0, 0.5, 2.5], [nan, nan, nan]], [7, 0], [98, 0], [90, 0], [91, 0], [16000, 300])
    out = _evaluation([[2.0 / 3.0, 0.25, 7.5], [nan, nan, nan]], [7, 0], [98, 0], [92, 0], [93, 0], [16000, 300])
    rows = S.report_rows(["a", "b"], inp, out)
    cols = ["file", "samples", "cd_in", "cd_out", "cd_delta", "llr_in", "llr_out", "llr_delta", "fwsegsnr_in", "fwsegsnr_out", "fwsegsnr_delta", "flags_in",
            "flags_out", "frames", "llr_frames_in", "llr_frames_out", "fwsegsnr_frames_in", "fwsegsnr_frames_out"]
    assert list(rows[0]) == cols
    assert rows[0]["cd_delta"] == 2.0 / 3.0 - 4.0 / 3.0 and rows[0]["fwsegsnr_delta"] == 5.0 and math.isnan(rows[1]["llr_delta"])
    p = str(tmp_path / "spectral.csv")
    S.write_report(p, rows)
    assert open(p).read().splitlines()[2] == "b,300,,,,,,,,,,0,0,0,0,0,0,0"                # NaN is an empty field
    back = R.read_csv(p)
    assert len(back) == 2
    for a, b in zip(rows, back):
        assert list(a) == list(b)
        for k in a:
            assert (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k], k      # repr(float) reads back exactly
    summ = S.summary_rows(rows)
    assert [s["value"] for s in summ] == [f"{m}_{k}" for m in S.VALUES for k in ("in", "out", "delta")]
    by = {s["value"]: s for s in summ}
    assert by["cd_out"]["n"] == 1 and by["cd_out"]["mean"] == by["cd_out"]["median"] == 2.0 / 3.0 and by["cd_out"]["std"] == 0.0
    assert "cd_out" in S.format_summary(summ) and S.summary_rows([]) == []
    part = S.report_rows(["a", "b"], inp, _evaluation(out.values, out.flags, out.frames, out.llr_frames, out.fwsegsnr_frames, out.samples, names=("llr",)))
    assert list(part[0]) == [c for c in cols if not c.startswith(("cd_", "fwsegsnr_in", "fwsegsnr_out", "fwsegsnr_delta"))]
    al = Alignment(torch.tensor([3, 0], dtype=torch.int32), torch.tensor([0.75, nan], dtype=torch.float64), torch.tensor([0.125, 0.0], dtype=torch.float64),
                   torch.tensor([1, 0], dtype=torch.int32), None, None, torch.tensor([15997, 300], dtype=torch.int32), 800, 16000)
    out.alignment = al
    lagged = S.report_rows(["a", "b"], inp, out)
    assert list(lagged[0]) == cols + ["lag_in", "lag_out", "lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out", "align_flags_in", "align_flags_out"]
    assert lagged[0]["lag_out"] == 3 and lagged[0]["lag_ms_out"] == 0.1875 and math.isnan(lagged[0]["lag_in"]) and lagged[0]["align_flags_in"] == 0
    assert [s["value"] for s in S.summary_rows(lagged)][9:] == ["lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out"]
    q = str(tmp_path / "lagged.csv")
    S.write_report(q, lagged)
    assert R.read_csv(q)[0]["lag_out"] == 3


def test_spectral_options_default_off():
    from buddy_amd.config import compose
    from buddy_amd.testing.tester import spectral_options
    assert spectral_options({}) == (False, S.VALUES)                                      # a config written before the block existed
    assert spectral_options({"spectral": {"use": True}}) == (True, S.VALUES) and spectral_options({"spectral": {}}) == (False, S.VALUES)
    assert spectral_options({"spectral": {"use": True, "values": ["llr"]}}) == (True, ("llr",))
    conf = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conf", "tester")
    shipped = sorted(f[:-5] for f in os.listdir(conf) if f.endswith(".yaml"))
    assert len(shipped) >= 4
    for name in shipped:
        assert spectral_options(compose(tester=name).tester) == (False, S.VALUES), name
    assert spectral_options(compose(tester="blind_dereverberation_BUDDy", overrides=["tester.spectral.use=true"]).tester) == (True, S.VALUES)


def test_spectral_has_no_cpu_form():
    x = torch.zeros(1, 8000)
    with pytest.raises(_lib.BuddyHipError):
        S.evaluate(x, x, 16000)
    lib = _lib.load()
    assert lib.buddy_cepstral_distance_workspace(3, 73) == 8 * 3 * 73 * 50 and lib.buddy_cepstral_distance_workspace(3, 0) == 8 * 3 * 50
    assert lib.buddy_fwsegsnr_workspace(3, 73) == 16 * 3 * 73 and lib.buddy_fwsegsnr_workspace(0, 73) == -1
    assert lib.buddy_llr_workspace(3, 12000, 400, 160) == 16 * 3 * 73 and lib.buddy_llr_workspace(3, 399, 400, 160) == 16 * 3
    assert lib.buddy_llr_workspace(3, 12000, 513, 160) == -1 and lib.buddy_llr_workspace(3, 12000, 400, 0) == -1
