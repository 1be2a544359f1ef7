"""CPU tests of the noise tracker and post-filter's host side: the new symbols, every argument check of the C entries (nothing
is launched and no data pointer is dereferenced), the options parser on every shipped tester config, the frame rule, the refusals of the Python
layer and of the tool, and the properties of the float64 restatement (tests/_denoise_ref.py) that make it worth comparing the kernels against."""
import ctypes as C
import functools
import glob
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy.special import exp1

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _denoise_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.config import load_yaml  # noqa: E402
from buddy_amd.testing.tester import denoise_options  # noqa: E402
from buddy_amd.utils import denoise as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("buddy_denoise_frames", "buddy_denoise_spectra", "buddy_denoise_gains", "buddy_denoise_synthesis_workspace", "buddy_denoise_synthesis",
           "buddy_denoise_stats")
RULES = ("wiener", "lsa")


# ---- symbols, the frame rule, refusals --------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.EXPORTED and getattr(lib, name) is not None       # header = signatures = exports: tests/test_abi_host.py
    assert os.path.isfile(os.path.join(ROOT, "buddy_amd", "csrc", "denoise.hip"))          # build.sh compiles and links every csrc/*.hip
    assert (D.N, D.HOP, D.PAD, D.BINS) == (R.N, R.H, R.P, R.BINS) == (512, 128, 384, 257)
    assert (D.ZERO, D.SHORT, D.NO_SPEECH) == (R.ZERO, R.SHORT, R.NO_SPEECH) and D.ROW_FLOOR == R.FLOOR and D.GAINS == RULES


def test_frame_rule():
    lib = _lib.load()
    assert tuple(D.frames(L) for L in R.EDGE_LENGTHS) == (4, 4, 4, 5, 7, 7, 8, 9) == tuple(R.frames(L) for L in R.EDGE_LENGTHS)
    assert tuple(lib.buddy_denoise_frames(L) for L in R.EDGE_LENGTHS) == (4, 4, 4, 5, 7, 7, 8, 9)
    assert lib.buddy_denoise_frames(0) == -1 and lib.buddy_denoise_frames((1 << 30) + 1) == -1 and lib.buddy_denoise_frames(1 << 30) == R.frames(1 << 30)
    for L in (1, 127, 128, 129, 700, 12345):                                             # every sample lies in exactly four frames
        T = R.frames(L)
        cover = np.zeros(L, int)
        for t in range(T):
            lo, hi = max(t * R.H - R.P, 0), min(t * R.H - R.P + R.N, L)
            assert hi > lo, (L, t)                                                         # and no frame is empty
            cover[lo:hi] += 1
        assert np.all(cover == 4), L
    with pytest.raises(ValueError):
        D.frames(0)
    assert R.window().min() > 0.0


def test_argument_checks_need_no_gpu():
    """every BUDDY_ERR_ARG case of the four entries, with nothing launched: 0x1000 stands in for the data pointers; the lengths and the row floors,
    which the entries read to check them, are real host arrays"""
    lib = _lib.load()
    X, L = 0x1000, 1000
    T = R.frames(L)
    ints = lambda *v: C.cast((C.c_int * len(v))(*v), C.c_void_p)
    dbls = lambda *v: C.cast((C.c_double * len(v))(*v), C.c_void_p)
    inf, nan = float("inf"), float("nan")
    keep = []                                                                              # the host arrays outlive the calls

    def run(entry, good, order, cases):
        for change, why in cases:
            a = dict(good, **change)
            keep.append(a)
            rc = getattr(lib, entry)(*[a[k] for k in order], None)
            assert rc == 2, (entry, why)
            assert lib.buddy_last_error().decode().startswith(entry + ": "), (entry, why)

    rows = [(dict(B=0), "B < 1"), (dict(B=65536), "B above 65535"), (dict(lens=ints(0, L)), "a length of 0"), (dict(lens=ints(L, (1 << 30) + 1)), "a length above 2^30"),
            (dict(lens=ints(L, -5)), "a negative length"), (dict(ldt=T - 1), "ldt < T")]
    strides = rows + [(dict(ld=L - 1), "ld < L")]
    run("buddy_denoise_spectra", dict(x=X, lens=ints(L, 700), B=2, ld=L, Y=X, ldt=T), ("x", "lens", "B", "ld", "Y", "ldt"),
        [(dict(x=None), "null x"), (dict(lens=None), "null lens"), (dict(Y=None), "null Y")] + strides)
    run("buddy_denoise_gains", dict(Y=X, lens=ints(L, 700), phi=dbls(1e-9, 0.0), B=2, ldt=T, rule=1, g_min=0.1778, G=X, S=X),
        ("Y", "lens", "phi", "B", "ldt", "rule", "g_min", "G", "S"),
        [(dict(Y=None), "null Y"), (dict(lens=None), "null lens"), (dict(phi=None), "null phi"), (dict(G=None), "null G"), (dict(S=None), "null sigma2"),
         (dict(rule=2), "unknown rule"), (dict(rule=-1), "unknown rule"), (dict(g_min=0.0), "g_min = 0"), (dict(g_min=-0.5), "g_min < 0"),
         (dict(g_min=1.0001), "g_min > 1"), (dict(g_min=nan), "g_min NaN"), (dict(phi=dbls(nan, 1.0)), "phi NaN"), (dict(phi=dbls(1.0, inf)), "phi inf"),
         (dict(phi=dbls(-1e-12, 1.0)), "phi < 0")] + rows)
    ws = lib.buddy_denoise_synthesis_workspace(2, T)
    assert ws == 4 * 2 * T * 512 and lib.buddy_denoise_synthesis_workspace(0, T) == -1 and lib.buddy_denoise_synthesis_workspace(2, 0) == -1
    run("buddy_denoise_synthesis", dict(Y=X, G=X, lens=ints(L, 700), B=2, ldt=T, out=X, ld=L, ws=X, ws_bytes=ws),
        ("Y", "G", "lens", "B", "ldt", "out", "ld", "ws", "ws_bytes"),
        [(dict(Y=None), "null Y"), (dict(G=None), "null G"), (dict(lens=None), "null lens"), (dict(out=None), "null out"), (dict(ws=None), "null ws"),
         (dict(ws_bytes=ws - 1), "workspace too small")] + strides)
    run("buddy_denoise_stats", dict(x=X, out=X, lens=ints(L, 700), B=2, ld=L, Y=X, S=X, ldt=T, stats=X), ("x", "out", "lens", "B", "ld", "Y", "S", "ldt", "stats"),
        [(dict(x=None), "null x"), (dict(out=None), "null out"), (dict(lens=None), "null lens"), (dict(Y=None), "null Y"), (dict(S=None), "null sigma2"),
         (dict(stats=None), "null stats")] + strides)


def test_options_parser_on_every_shipped_config():
    paths = sorted(glob.glob(os.path.join(ROOT, "conf", "tester", "*.yaml")))
    assert len(paths) >= 4
    with_block = 0
    for p in paths:
        rr = load_yaml(p).get("real_recordings", None) or {}
        assert denoise_options(rr) == (False, "lsa", -15.0), p                             # everything ships off
        with_block += "denoise" in rr
    assert with_block == 1                                                                 # the real-recordings config carries the block
    assert denoise_options({}) == denoise_options({"denoise": None}) == (False, "lsa", -15.0)
    assert denoise_options({"denoise": {"use": True, "gain": "wiener", "floor_db": -20}}) == (True, "wiener", -20.0)
    for bad in ({"gain": "mmse"}, {"floor_db": 3}, {"floor_db": -200}, {"floor_db": float("nan")}):
        with pytest.raises(AssertionError, match="real_recordings.denoise"):
            denoise_options({"denoise": dict({"use": True}, **bad)})


def test_python_refusals():
    x = torch.zeros(2, 1000)
    for call in (lambda: D.denoise(x), lambda: D.spectra_hip(x), lambda: D.gains_hip(torch.zeros(2, 11, 257, 2), [1000, 1000], [1.0, 1.0]),
                 lambda: D.synthesis_hip(torch.zeros(2, 11, 257, 2), torch.zeros(2, 11, 257), [1000, 1000])):
        with pytest.raises(_lib.BuddyHipError):                                            # a CPU tensor: there is no CPU form
            call()
    with pytest.raises(ValueError, match="gain"):
        D.denoise(x, gain="mmse")
    with pytest.raises(ValueError, match="floor_db"):
        D.denoise(x, floor_db=1.0)
    with pytest.raises(ValueError, match="floor_db"):
        D.gains_hip(torch.zeros(2, 11, 257, 2), [1000, 1000], [1.0, 1.0], floor_db=float("nan"))
    with pytest.raises(ValueError):
        D.denoise(np.zeros((2, 1000), np.float32))                                         # not a tensor
    assert D.flag_text(0) == "" and D.flag_text(D.ZERO | D.NO_SPEECH) == "ZERO|NO_SPEECH"


def test_tool_argument_refusals(tmp_path):
    spec = importlib.util.spec_from_file_location("denoise_tool", os.path.join(ROOT, "tools", "denoise.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = [str(tmp_path), "--out", str(tmp_path / "out")]
    for extra, why in ((["--gain", "mmse"], "--gain"), (["--floor-db", "6"], "--floor-db"), (["--floor-db", "-300"], "--floor-db"), (["--fs", "10"], "--fs"),
                       ([], "no wav")):
        with pytest.raises(SystemExit) as e:
            tool.main(base + extra)
        assert why in str(e.value), (extra, str(e.value))
    with pytest.raises(SystemExit):
        tool.main([str(tmp_path)])                                                         # --out is required
    assert not os.path.exists(tmp_path / "out")


# ---- the restatement's own properties -----------------------------------------------------------------------------------------------------------------
def test_exponential_integral():
    """both branches against scipy, in float64; the longdouble run agrees with it to float64's precision"""
    x = np.concatenate([np.logspace(-9, 0, 400)[:-1], np.logspace(0, 3, 400)])
    want = exp1(x)
    live = want > 1e-300
    assert (np.abs(R.expint_e1(x) - want)[live] / want[live]).max() < 2e-14
    assert (np.abs(R.expint_e1(x.astype(np.longdouble)).astype(np.float64) - want)[live] / want[live]).max() < 2e-14


def test_unit_gain_reconstructs():
    for L in R.EDGE_LENGTHS:
        x = np.random.RandomState(L).standard_normal(L)
        Y = R.spectra(x)
        assert Y.shape == (R.frames(L), R.BINS)
        assert np.abs(R.synthesis(Y, np.ones(Y.shape), L) - x).max() <= 1e-12, L


@functools.lru_cache(maxsize=None)
def _white(seed, rule):
    x = R.white(48000, 0.05, seed)
    return x, R.denoise(x, rule)


@pytest.mark.parametrize("rule", RULES)
def test_white_noise_alone(rule):
    """the tracked noise power sits within 2 dB of the true one (the tracker's known bias is about -1.1 dB), and the filter takes stationary noise
    down to nearly its floor of 15 dB"""
    w2 = float(np.sum(R.window() ** 2))
    for seed in (0, 1):
        x, r = _white(seed, rule)
        T = r["frames"]
        bias = 10.0 * math.log10(r["sigma2"][T // 3:].mean() / (0.05 ** 2 * w2))
        att = 10.0 * math.log10(np.sum(x[16000:].astype(np.float64) ** 2) / np.sum(r["out"][16000:] ** 2))
        print(f"{rule} seed {seed}: noise power bias {bias:.2f} dB, attenuation after 1 s {att:.2f} dB, snr_est {r['snr_est_db']:.2f} dB")
        assert abs(bias) <= 2.0 and 13.0 <= att <= 15.5 and r["flags"] == 0


@functools.lru_cache(maxsize=None)
def _bursts(snr, seed, rule):
    y, clean, noise, mask = R.noisy_bursts(snr, seed=seed)
    return y, clean, mask, R.denoise(y, rule)


@pytest.mark.parametrize("rule", RULES)
def test_bursts_plus_noise(rule):
    for seed in (0, 1):
        for snr, gain_db, snr_tol in ((20.0, None, 1.0), (10.0, 2.0, 1.0), (0.0, 4.0, 2.5)):
            y, clean, mask, r = _bursts(snr, seed, rule)
            assert abs(np.mean(clean * clean) - 1.0) < 1e-12
            gained = R.si_sdr(r["out"], clean) - R.si_sdr(y, clean)
            gaps = R.gap_mask(mask)
            att = 10.0 * math.log10(np.sum(y[gaps].astype(np.float64) ** 2) / np.sum(r["out"][gaps] ** 2))
            print(f"{rule} seed {seed} {snr:4.0f} dB: SI-SDR gain {gained:.2f} dB, attenuation in the gaps {att:.2f} dB, snr_est {r['snr_est_db']:.2f} dB")
            assert gain_db is None or gained >= gain_db
            assert att >= 13.0 and abs(r["snr_est_db"] - snr) <= snr_tol
            if rule == "lsa":
                assert r["seen"]["ag_min"] < 0.1 and r["seen"]["ag_max"] > 10.0            # both branches of E1


@pytest.mark.parametrize("rule", RULES)
def test_scaling_and_leading_silence(rule):
    y, _, _, r = _bursts(10.0, 0, rule)
    big = R.denoise(y.astype(np.float64) * 4096.0, rule)
    assert np.abs(big["G"] - r["G"]).max() <= 1e-12
    x = R.silence_led(2000, 12000)
    s = R.denoise(x, rule)
    assert all(np.isfinite(s[k]).all() for k in ("out", "G", "sigma2")) and not s["out"][:1500].any()
    assert math.isfinite(s["snr_est_db"]) and math.isfinite(s["noise_db"]) and s["seen"]["floored"] > 0 and s["flags"] == 0
    z = R.denoise(np.zeros(700, np.float32), rule)
    assert z["flags"] == R.ZERO and not z["out"].any() and np.all(z["G"] == 1.0) and math.isnan(z["snr_est_db"])
    assert R.denoise(R.white(300, 0.1, 9), rule)["flags"] == R.SHORT
