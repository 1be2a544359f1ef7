"""CPU tests of the room-acoustics report's host side: the float64 oracle (tests/_acoustics_ref.py) on closed forms, the octave bank's measured
response, the validity rule of a decay fit, the CSV writers, the tester yaml, and every argument check of the three C entries (no GPU needed:
nothing is launched and no data pointer is dereferenced)."""
import ctypes as C
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acoustics_ref as R  # noqa: E402

from buddy_amd.utils import acoustics as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000


def exponential(T, seconds, fs=FS):
    """h[n] = exp(-a n) with a 60 dB energy decay in T seconds, cut after ``seconds``"""
    a = math.log(1000.0) / (T * fs)
    return np.exp(-a * np.arange(int(round(seconds * fs)), dtype=np.float64)), a


def test_oracle_on_closed_forms():
    """a sampled exponential has an exactly linear Schroeder curve up to its truncation term, 4.34 exp(-2a (N - n_hi)) dB < 1e-7 dB at 2.2 T, so the
    three decay times equal T; the energy ratios and the centre time are geometric series"""
    T = 0.5
    h, a = exponential(T, 2.2 * T)
    N = len(h)
    val, flags, D = R.metrics(h, R.argmax_abs(h), FS)
    assert flags == 0b111111111
    for q in (R.EDT, R.T20, R.T30):
        assert abs(val[q] / T - 1.0) < 1e-6, (q, val[q])
    q = math.exp(-2.0 * a)
    n50, w = 800, 40
    assert abs(val[R.C50] - 10.0 * math.log10((1.0 - q ** n50) / (q ** n50 - q ** N))) < 1e-9
    assert abs(val[R.DRR] - 10.0 * math.log10((1.0 - q ** (w + 1)) / (q ** (w + 1) - q ** N))) < 1e-9          # n0 = ns = 0: direct part n <= w
    first_moment = q * (1.0 - N * q ** (N - 1) + (N - 1) * q ** N) / (1.0 - q) ** 2                              # sum_{n < N} n q^n
    ts = first_moment / ((1.0 - q ** N) / (1.0 - q)) / FS
    assert abs(val[R.TS] / ts - 1.0) < 1e-9
    assert D[0] == 0.0 and np.all(np.diff(D) < 0)


def test_oracle_direct_path_offset_and_degenerate_rows():
    """a delayed exponential: the analysis starts w samples before the peak and the values do not move; an all-zero row gives NaN and no flag"""
    T = 0.3
    h, _ = exponential(T, 2.5 * T)
    ref, fl_ref, _ = R.metrics(h, 0, FS)
    d = np.concatenate([np.zeros(100), h])
    assert R.argmax_abs(d) == 100
    val, fl, D = R.metrics(d, 100, FS)
    assert fl == fl_ref == 0b111111111 and len(D) == len(d) - 60
    for q in (R.T20, R.T30):
        assert abs(val[q] / ref[q] - 1.0) < 1e-9
    assert abs(val[R.TS] - (ref[R.TS] + 40.0 / FS)) < 1e-12                  # the peak sits 40 samples after the analysis start
    val, fl, _ = R.metrics(np.zeros(500), 0, FS)
    assert fl == 0 and np.isnan(val).all()
    val, fl, _ = R.metrics(np.array([0.0, 1.0]), 1, FS)                      # the peak in the last sample: no late and no reverberant part
    assert np.isnan(val[[R.EDT, R.T20, R.T30, R.C50, R.DRR]]).all() and fl == 1 << R.TS


def response_db(taps, f, fs):
    n = np.arange(len(taps)) - (len(taps) - 1) // 2
    return 20.0 * math.log10(abs(float((taps * np.cos(2.0 * np.pi * f * n / fs)).sum())))


@pytest.mark.parametrize("fs,centres", [(16000, A.OCTAVES), (48000, A.OCTAVES + (8000,))])
def test_bank_figures(fs, centres):
    """measured in float64 at both rates: +0.0014 .. +0.0030 dB at the centre, -6.019 .. -6.021 dB at the edges, -59.00 .. -60.5 dB at the centre of
    the octave below, -75.17 .. -88.7 dB at the centre of the octave above"""
    bank = A.octave_bank(fs, centres)
    assert bank.shape == (len(centres), math.ceil(8 * fs / 125) | 1) and bank.dtype == np.float64
    assert A.octave_bank(16000).shape[1] == 1025
    for k, fc in enumerate(centres):
        taps = bank[k]
        n_taps = math.ceil(8 * fs / fc) | 1
        pad = (bank.shape[1] - n_taps) // 2
        assert np.all(taps[:pad] == 0) and np.all(taps[bank.shape[1] - pad:] == 0) and taps[pad] != 0      # centred, zero-padded
        assert np.array_equal(taps, taps[::-1])                                                              # zero phase
        assert 0.0 <= response_db(taps, fc, fs) <= 0.005
        for edge in (fc / math.sqrt(2.0), fc * math.sqrt(2.0)):
            assert abs(response_db(taps, edge, fs) + 6.02) < 0.01
        assert response_db(taps, fc / 2.0, fs) <= -58.9
        assert response_db(taps, fc * 2.0, fs) <= -75.0
    ab = A.analysis_bank(fs, centres)
    P = (ab.shape[1] - 1) // 2
    assert ab.shape[0] == len(centres) + 1 and ab[0, P] == 1.0 and np.count_nonzero(ab[0]) == 1 and np.array_equal(ab[1:], bank)


def test_bank_refuses_a_centre_above_the_band_limit():
    with pytest.raises(ValueError, match="0.45 fs"):
        A.octave_bank(16000, (4000, 8000))                  # upper edge 11 314 Hz > 7200 Hz
    assert A.octave_bank(16000, (5000,)).shape == (1, 27)   # 7071 Hz: allowed
    with pytest.raises(ValueError):
        A.octave_bank(16000, (5100,))                       # 7212 Hz


def test_validity_rule():
    """the same exponential (T = 0.5 s) cut to 0.3 s and to 1.1 s: the -35 dB point lies at 0.29 s, so the first row has about 1 dB of decay left
    after its last fitted sample and its T30 is not valid; the second has 97 dB left"""
    rows = [exponential(0.5, 0.3)[0], exponential(0.5, 1.1)[0]]
    values, flags, n0 = R.analyse(rows, FS, np.ones((1, 1)))
    assert list(n0) == [0, 0]
    t30_valid = (flags[:, 0] >> (6 + R.T30)) & 1
    assert list(t30_valid) == [0, 1]
    assert ((flags[:, 0] >> R.T30) & 1).all() and np.isfinite(values[:, 0, R.T30]).all()       # the value is returned either way
    assert abs(values[1, 0, R.T30] / 0.5 - 1.0) < 1e-6
    assert values[0, 0, R.T30] < 0.5 * (1.0 - 1e-3)                                              # bent down by the truncation


def test_csv_writers_round_trip(tmp_path):
    nan = float("nan")
    est = A.RirAcoustics((0.0, 125.0), torch.tensor([[[0.5, 0.25, nan, 3.0, -11.5, 0.036], [nan] * 6]], dtype=torch.float64),
                         torch.tensor([[0b011111011, 0]], dtype=torch.int32), torch.tensor([7], dtype=torch.int32))
    true = A.RirAcoustics((0.0, 125.0), torch.tensor([[[0.4, 0.2, 0.3, 2.0, -10.0, 0.03], [0.1, nan, nan, 1.0, 2.0, 0.01]]], dtype=torch.float64),
                          torch.tensor([[511, 0b111001]], dtype=torch.int32), torch.tensor([0], dtype=torch.int32))
    rows = A.report_rows(["a b,c"], est, true)
    p = str(tmp_path / "acoustics.csv")
    A.write_report(p, rows)
    text = open(p).read().splitlines()
    assert text[0] == "file,band,EDT,T20,T30,C50,DRR,Ts,flags,true_EDT,true_T20,true_T30,true_C50,true_DRR,true_Ts,true_flags,err_EDT,err_T20,err_T30,err_C50,err_DRR"
    assert text[2] == '"a b,c",125,,,,,,,0,0.1,,,1.0,2.0,0.01,57,,,,,'              # NaN -> empty field, flags -> integer
    back = R.read_csv(p)
    assert len(back) == 2 and back[0]["file"] == "a b,c" and back[0]["band"] == "broadband" and back[1]["band"] == "125"
    for r, b in zip(rows, back):
        for k, v in r.items():
            if isinstance(v, float):
                assert (math.isnan(v) and math.isnan(b[k])) or v == b[k], (k, v, b[k])            # repr() of a double reads back bit for bit
            else:
                assert v == b[k]
    assert back[0]["err_EDT"] == 0.5 - 0.4 and math.isnan(back[0]["err_T30"]) and back[0]["flags"] == 0b011111011
    # without the true RIRs: no true_* / err_* columns
    A.write_report(p, A.report_rows(["x"], est))
    assert open(p).read().splitlines()[0] == "file,band,EDT,T20,T30,C50,DRR,Ts,flags"
    # the operator's parameters
    params = {"freqs": [125.0, 250.0], "T60": torch.tensor([[[0.1, 0.2]], [[0.3, nan]]], dtype=torch.float64),
              "weights": torch.tensor([[[2.0, 1.0]], [[0.5, 0.25]]], dtype=torch.float64)}
    q = str(tmp_path / "parameters.csv")
    A.write_parameters(q, A.parameter_rows(["u0", "u1"], params))
    back = R.read_csv(q)
    assert [(r["file"], r["exponential"], r["freq_hz"]) for r in back] == [("u0", 0, 125.0), ("u0", 0, 250.0), ("u1", 0, 125.0), ("u1", 0, 250.0)]
    assert back[0]["T60"] == 0.1 and back[2]["weight"] == 0.5 and math.isnan(back[3]["T60"]) and back[3]["weight"] == 0.25
    A.write_report(p, [])
    assert open(p).read() == ""


def test_rir_report_is_off_in_every_shipped_yaml():
    """`use: false` with the octave centres in the tester yaml files that have a blind mode, absent (or off) in every other yaml"""
    blind = []
    for f in sorted(glob.glob(os.path.join(ROOT, "conf", "**", "*.yaml"), recursive=True)):
        cfg = yaml.safe_load(open(f)) or {}
        modes = cfg.get("modes", []) if isinstance(cfg, dict) else []
        block = cfg.get("rir_report", None) if isinstance(cfg, dict) else None
        if any("blind" in str(m) for m in modes):
            blind.append(os.path.basename(f))
            assert block == {"use": False, "centres": [125, 250, 500, 1000, 2000, 4000]}, f
        else:
            assert block is None or block.get("use", False) is False, f
    assert blind == ["blind_dereverberation_BUDDy.yaml", "real_dereverberation_BUDDy.yaml"]
    from buddy_amd.testing.tester import rir_report_options
    assert rir_report_options({}) == (False, A.OCTAVES)                                  # a config written before the key existed
    assert rir_report_options({"rir_report": {"use": True, "centres": [250, 500]}}) == (True, (250.0, 500.0))
    assert rir_report_options({"rir_report": {"use": True}}) == (True, A.OCTAVES)


def test_cpu_tensor_is_refused():
    with pytest.raises(A._lib.BuddyHipError):
        A.rir_acoustics(torch.zeros(1, 100), 16000)


def test_argument_checks_need_no_gpu():
    """every BUDDY_ERR_ARG case of the three entries, with nothing launched: data pointers are never dereferenced (0x1000 stands in for them); the
    length arrays are real int32 arrays, read on the host where no device exists"""
    from buddy_amd import _lib
    lib = _lib.load()
    X = 0x1000
    ints = lambda *v: C.addressof(keep.setdefault(v, (C.c_int * len(v))(*v)))
    keep = {}
    ok_lens = ints(100, 90)
    cases = {
        "buddy_row_argmax_abs": [      # (h, lens, B, ldh, n0)
            ((None, ok_lens, 2, 100, X), "null h"), ((X, None, 2, 100, X), "null lens"), ((X, ok_lens, 2, 100, None), "null n0"),
            ((X, ok_lens, 0, 100, X), "B < 1"), ((X, ints(100, 0), 2, 100, X), "a zero length"), ((X, ints(-3, 5), 2, 100, X), "a negative length"),
            ((X, ok_lens, 2, 99, X), "stride below the longest row"), ((X, ok_lens, 2, 0, X), "stride < 1"),
        ],
        "buddy_fir_bank": [            # (h, lens, B, ldh, bank, nb, Nh, g, ldg)
            ((None, ok_lens, 2, 100, X, 3, 9, X, 104), "null h"), ((X, None, 2, 100, X, 3, 9, X, 104), "null lens"),
            ((X, ok_lens, 2, 100, None, 3, 9, X, 104), "null bank"), ((X, ok_lens, 2, 100, X, 3, 9, None, 104), "null g"),
            ((X, ok_lens, 0, 100, X, 3, 9, X, 104), "B < 1"), ((X, ok_lens, 2, 100, X, 0, 9, X, 104), "nb < 1"),
            ((X, ok_lens, 2, 100, X, 3, 8, X, 104), "even Nh"), ((X, ok_lens, 2, 100, X, 3, 0, X, 104), "Nh < 1"),
            ((X, ok_lens, 2, 100000, X, 3, 65539, X, 200000), "Nh above 65 537"),
            ((X, ints(0, 90), 2, 100, X, 3, 9, X, 104), "a zero length"), ((X, ok_lens, 2, 99, X, 3, 9, X, 104), "ldh below the longest row"),
            ((X, ok_lens, 2, 100, X, 3, 9, X, 103), "ldg below the longest row plus P"),
        ],
        "buddy_decay_metrics": [       # (g, lens_g, n0, B, nb, ldg, fs, out, flags, edc_db)
            ((None, ok_lens, X, 2, 3, 100, 16000, X, X, None), "null g"), ((X, None, X, 2, 3, 100, 16000, X, X, None), "null lens_g"),
            ((X, ok_lens, None, 2, 3, 100, 16000, X, X, None), "null n0"), ((X, ok_lens, X, 2, 3, 100, 16000, None, X, None), "null out"),
            ((X, ok_lens, X, 2, 3, 100, 16000, X, None, None), "null flags"), ((X, ok_lens, X, 0, 3, 100, 16000, X, X, None), "B < 1"),
            ((X, ok_lens, X, 2, 0, 100, 16000, X, X, None), "nb < 1"), ((X, ok_lens, X, 2, 3, 100, 0, X, X, None), "fs < 1"),
            ((X, ints(100, 0), X, 2, 3, 100, 16000, X, X, None), "a zero length"), ((X, ok_lens, X, 2, 3, 99, 16000, X, X, X), "ldg below the longest row"),
        ],
    }
    for name, rows in cases.items():
        for args, why in rows:
            assert getattr(lib, name)(*args, None) == 2, (name, why)
            assert lib.buddy_last_error().decode().startswith(name + ": "), (name, why)
    assert lib.buddy_decay_tile() >= 64 and lib.buddy_decay_tile() % 64 == 0
