"""CPU tests of the noise field's host side: the new symbols, every argument check of the C entry (nothing is launched and no
data pointer is dereferenced), the refusals of the Python layer and of the tool, the coherence of the two lattices against the closed forms, the
statistics of the float64 restatement (tests/_noise_ref.py) on the project's own Philox normals, the shaping filter, and ``mix_at_snr``'s host form."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy.special import j0

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _level_ref as LR  # noqa: E402
import _noise_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import level as LV  # noqa: E402
from buddy_amd.utils import noise as NZ  # noqa: E402
from buddy_amd.utils import rng  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 343.0


def ring(D, radius=0.1, angle=0.0):
    phi = angle + 2.0 * np.pi * np.arange(D) / D
    return np.stack([radius * np.cos(phi), radius * np.sin(phi), np.zeros(D)], axis=1)


# ---- symbols and refusals -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("buddy_noise_bank", "buddy_noise_tile", "buddy_noise_max_taps"):
        assert name in _lib.EXPORTED and getattr(lib, name) is not None       # header = signatures = exports: tests/test_abi_host.py
    assert lib.buddy_noise_tile() >= 64 and lib.buddy_noise_tile() % 64 == 0
    assert lib.buddy_noise_max_taps() >= NZ.TAPS == 2 * NZ.HW and NZ.HW == lib.buddy_ism_half_width() and NZ.PAD == NZ.HW + NZ.MAX_DELAY
    assert (NZ.NOISE_DRAWS, NZ.NOISE_FIELD, NZ.NOISE_SENSOR) == (7, 8, 9)


def test_argument_checks_need_no_gpu():
    """every BUDDY_ERR_ARG case of buddy_noise_bank, with nothing launched: 0x1000 stands in for the device pointers"""
    lib = _lib.load()
    X, W, inf, nan = 0x1000, lib.buddy_noise_max_taps(), float("inf"), float("nan")
    good = dict(taps=X, first=X, keys=X, purpose=8, draw0=0, out=X, B=2, D=4, N=16, W=W, P=104, L=1000, scale=0.25)
    cases = [(dict(taps=None), "null taps"), (dict(first=None), "null first"), (dict(keys=None), "null keys"), (dict(out=None), "null out"),
             (dict(D=0), "D < 1"), (dict(D=9), "D above 8"), (dict(N=0), "N < 1"), (dict(N=4097), "N above 4096"), (dict(W=0), "W < 1"),
             (dict(W=W + 1), "W above max_taps"), (dict(P=-1), "P < 0"), (dict(P=4097), "P above 4096"), (dict(B=0), "B < 1"), (dict(L=0), "L < 1"),
             (dict(scale=inf), "infinite scale"), (dict(scale=nan), "NaN scale")]
    for change, why in cases:
        a = dict(good, **change)
        rc = lib.buddy_noise_bank(a["taps"], a["first"], a["keys"], a["purpose"], a["draw0"], a["out"], a["B"], a["D"], a["N"], a["W"], a["P"], a["L"],
                                  a["scale"], None)
        assert rc == 2, why
        assert lib.buddy_last_error().decode().startswith("buddy_noise_bank: "), why


def test_python_refusals():
    dirs = NZ.sphere_directions(8)
    taps, first = NZ.delay_taps(ring(3), dirs, 16000)
    keys = np.array([rng.stream_key(0, "a")], dtype=np.uint32)
    assert taps.shape == (8, 3, NZ.TAPS) and first.shape == (8, 3) and first.dtype == np.int32
    with pytest.raises(_lib.BuddyHipError):                                  # CPU tensors
        NZ.noise_bank_hip(torch.from_numpy(taps[None]), torch.from_numpy(first[None]), keys, 100)
    with pytest.raises(_lib.BuddyHipError):
        NZ.mix_at_snr(torch.zeros(1, 2, 10), torch.zeros(1, 2, 10), None, 10.0, None, 16000)
    with pytest.raises(ValueError, match="exceeds M"):                       # tau beyond M: 64 samples are 1.372 m at 16 kHz
        NZ.delay_taps(np.array([[1.4, 0.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]), 16000)
    NZ.delay_taps(np.array([[1.37, 0.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]), 16000)
    with pytest.raises(ValueError, match="float64"):
        NZ.noise_bank_hip(taps[None].astype(np.float32), first[None], keys, 100)
    with pytest.raises(ValueError, match="int32"):
        NZ.noise_bank_hip(taps[None], first[None].astype(np.int64), keys, 100)
    with pytest.raises(ValueError, match="keys"):
        NZ.noise_bank_hip(taps[None], first[None], np.zeros((2, 2), dtype=np.uint32), 100)
    with pytest.raises(ValueError, match="L in"):
        NZ.noise_bank_hip(taps[None], first[None], keys, 0)
    bad = first[None].copy()
    bad[0, 3, 1] = NZ.PAD - NZ.TAPS + 2
    with pytest.raises(ValueError, match="first lag"):
        NZ.noise_bank_hip(taps[None], bad, keys, 100)
    with pytest.raises(ValueError, match="spherical"):
        NZ.directions("planar", 8)


def test_tool_flag_refusals(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_paired_set as T
    base = ["--clean", str(tmp_path), "--out", str(tmp_path / "out")]
    for extra, why in ((["--snr", "10", "20"], "needs --reverberant"), (["--sensor-snr", "30"], "needs --reverberant"),
                       (["--reverberant", "--snr", "10", "20", "--bands"], "--bands"), (["--reverberant", "--snr", "20", "10"], "LO <= HI"),
                       (["--reverberant", "--noise-waves", "0", "--snr", "10", "20"], "--noise-waves"),
                       (["--reverberant", "--snr", "10", "20", "--sensor-snr", "15"], "above")):
        with pytest.raises(SystemExit) as e:
            T.main(base + extra)
        assert why in str(e.value), (extra, str(e.value))


# ---- the lattices are diffuse -------------------------------------------------------------------------------------------------------------------
SPACINGS = (0.0765, 0.1414, 0.2)                     # the pair spacings of the 8-microphone array of radius 0.1 m
FREQS = np.arange(0.0, 8000.5, 25.0)


def _unit_vectors():
    v = np.random.RandomState(0).standard_normal((20, 3))
    return np.concatenate([np.eye(3), v / np.linalg.norm(v, axis=1, keepdims=True)])


def _worst(dirs, vectors, closed_form):
    worst = 0.0
    for d in SPACINGS:
        for u in vectors:
            g = NZ.field_coherence(dirs, np.stack([np.zeros(3), d * u]), FREQS, C)
            assert np.abs(g[0, 0] - 1.0).max() < 1e-15 and np.abs(g[1, 0] - np.conj(g[0, 1])).max() < 1e-15
            worst = max(worst, float(np.abs(g[0, 1] - closed_form(d)).max()))
    return worst


def test_fibonacci_lattice_is_diffuse():
    """measured here: 0.0107 at N = 512 (the three axes and these 20 vectors), 0.122 at N = 256 -- which is why 512 is the default"""
    sinc = lambda d: np.sinc(2.0 * FREQS * d / C)
    dirs = NZ.sphere_directions(512)
    assert np.abs(np.linalg.norm(dirs, axis=1) - 1.0).max() < 1e-15 and abs(dirs[:, 2].sum()) < 1e-12
    assert _worst(dirs, _unit_vectors(), sinc) < 0.02
    assert _worst(NZ.sphere_directions(256), _unit_vectors(), sinc) > 0.02


def test_circle_is_cylindrically_diffuse():
    """horizontal pairs (the field has no vertical component to decorrelate a vertical pair); measured here: 2e-15"""
    v = _unit_vectors()[:, :2]
    v = v[np.linalg.norm(v, axis=1) > 0]
    vectors = np.concatenate([v / np.linalg.norm(v, axis=1, keepdims=True), np.zeros((len(v), 1))], axis=1)
    assert _worst(NZ.circle_directions(512), vectors, lambda d: j0(2.0 * np.pi * FREQS * d / C)) < 0.02


def test_delay_taps_are_the_simulator_kernel():
    taps, first = NZ.delay_taps(np.array([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [64 * C / 16000, 0.0, 0.0]]), np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]), 16000, C)
    delta = np.zeros(NZ.TAPS)
    delta[NZ.HW - 1] = 1.0
    assert np.array_equal(taps[0, 0], delta) and first[0, 0] == 1 - NZ.HW            # tau = 0: a delta at lag 0
    tau = 16000 * 0.05 / C
    lags = first[0, 1] + np.arange(NZ.TAPS)
    x = lags - tau
    assert np.all(np.abs(x) < NZ.HW) and np.abs(taps[0, 1] - np.sinc(x) * 0.5 * (1 + np.cos(np.pi * x / NZ.HW))).max() < 1e-16
    assert np.array_equal(first[1], -first[0] - NZ.TAPS + 1 + np.array([1, 0, 1])) and np.abs(taps[1, 1] - taps[0, 1][::-1]).max() < 1e-13
    assert abs(taps[0, 1].sum() - 1.0) < 1e-3
    assert abs(abs(first[0, 2] + NZ.HW - 1) - 64) <= 1 and first.min() >= -NZ.PAD and first.max() <= NZ.PAD - NZ.TAPS + 1      # tau = +-M stays inside


# ---- restatement statistics ---------------------------------------------------------------------------------------------------------------------
def test_restatement_has_the_lattice_coherence():
    """N = 512, D = 4 on a circle of 0.1 m, the project's Philox normals.  L = 2^16, half of the issue's 2^17 (the restatement takes about 5 s
    here; at 2^17 twice that), so K = 256 segments and the bound 4 / sqrt(K) keeps its form: per component the estimate's error has a standard
    deviation of at most 1 / sqrt(2 K).  Measured here: the worst of the 6 pairs x 113 bins is 2.68 / sqrt(K), variances 0.979 .. 0.995 (the windowed sinc loses
    a little of the top octave)."""
    L, N, D, fs = 2 ** 16, 512, 4, 16000
    pos = ring(D)
    x = R.diffuse(pos, rng.stream_key(3, "p1/a"), L, fs, N)
    assert x.shape == (D, L)
    coh, K = R.coherence(x, 256)
    assert K == L // 256
    fb = np.arange(129) * fs / 256.0
    keep = fb <= 7000.0
    want = NZ.field_coherence(NZ.sphere_directions(N), pos, fb, C)
    err = np.abs(coh - want)[:, :, keep]
    var = x.var(axis=1)
    print(f"worst |coh - Gamma_N| sqrt(K) = {err.max() * math.sqrt(K):.3f}, variances {var.min():.4f} .. {var.max():.4f}")
    assert err.max() <= 4.0 / math.sqrt(K)
    assert np.abs(var - 1.0).max() <= 0.03


# ---- shaping ------------------------------------------------------------------------------------------------------------------------------------
def test_shaping_fir():
    fs = 16000
    white = NZ.shaping_fir(fs, 0.0)
    assert len(white) == 513 and abs(white[256] - 1.0) < 1e-12 and np.abs(np.delete(white, 256)).max() < 1e-12
    h = NZ.shaping_fir(fs, -3.0)
    assert np.abs(h - h[::-1]).max() < 1e-15                                 # linear phase
    H2 = np.abs(np.fft.rfft(h, 1024)) ** 2
    f = np.arange(513) * fs / 1024.0
    at = lambda hz: 10.0 * math.log10(H2[int(round(hz * 1024 / fs))])
    assert abs(at(1000.0)) < 0.05 and abs(at(4000.0) + 6.0) < 0.05 and abs(at(250.0) - 6.0) < 0.3
    x = rng.normals(rng.stream_key(1, "shape"), 0, 0, 2 ** 17 + 512)
    y = R.fir(x, h)[0, 512:]
    S, K = R.welch_cross(y[None], 1024)
    p = np.real(S[0, 0])
    # the estimate's expectation is |H|^2 smoothed by the Hann window's four-bin main lobe: narrow against an octave of 23 bins or more
    octave = lambda fc: (f >= fc / math.sqrt(2.0)) & (f < fc * math.sqrt(2.0))
    got = 10.0 * math.log10(p[octave(500.0)].sum() / p[octave(2000.0)].sum())
    want = 10.0 * math.log10(H2[octave(500.0)].sum() / H2[octave(2000.0)].sum())
    print(f"500 Hz over 2 kHz octave: estimated {got:.3f} dB, designed {want:.3f} dB")
    assert abs(got - want) < 0.5 and abs(want) < 3.0                         # pink: equal power per octave, up to the bin count of the bands


# ---- mix_at_snr on the restatement --------------------------------------------------------------------------------------------------------------
def _speech_and_noise(L=8000, D=3, fs=16000):
    key = rng.stream_key(5, "mix")
    diffuse = R.diffuse(ring(D), key, L, fs, 16).astype(np.float32)
    sensor = np.stack([rng.normals(key, NZ.NOISE_SENSOR, d, L) for d in range(D)]).astype(np.float32)
    env = 0.1 * (1.0 + np.sin(2.0 * np.pi * 3.0 * np.arange(L) / fs))
    speech = np.stack([env * rng.normals(key, 0, 7 + d, L) for d in range(D)]).astype(np.float32)
    return speech[None], diffuse[None], sensor[None]


def _snr_of(mix, speech):
    """recomputed in double from the arrays alone"""
    s = mix.mixed.astype(np.float64) - mix.noise.astype(np.float64)
    assert np.abs(s - speech).max() <= 2.0 ** -23 * np.abs(mix.mixed).max()
    return 10.0 * np.log10(np.sum(s[:, 0] ** 2, axis=1) / np.sum(mix.noise[:, 0].astype(np.float64) ** 2, axis=1))


def test_mix_at_snr_meets_the_request():
    y, dn, sn = _speech_and_noise()
    for snr, ssnr, d, s in ((20.0, 30.0, dn, sn), (5.0, None, dn, None), (None, 25.0, None, sn), (0.0, 40.0, dn, sn)):
        m = NZ.mix_at_snr(y, d, s, snr, ssnr, 16000)
        want = snr if d is not None else ssnr
        assert m.mixed.dtype == np.float32 and m.noise.shape == y.shape and m.reference == ["rms"] and m.flags == [""]
        assert abs(float(m.snr_measured_db[0]) - want) < 1e-3 and abs(float(_snr_of(m, y)[0]) - want) < 1e-3
        assert math.isnan(m.gain_diffuse[0]) == (d is None) and math.isnan(m.gain_sensor[0]) == (s is None)
        if d is not None and s is not None:          # one gain per kind for all channels, and the sensor noise alone sits at its own SNR
            assert np.abs(m.noise - (np.float32(m.gain_diffuse[0]) * d + np.float32(m.gain_sensor[0]) * s)).max() <= 2.0 ** -23 * np.abs(m.noise).max()
            ps, pn = np.sum(y[0, 0].astype(np.float64) ** 2), np.sum((m.gain_sensor[0] * sn[0, 0].astype(np.float64)) ** 2)
            assert abs(10.0 * math.log10(ps / pn) - ssnr) < 1e-3
    with pytest.raises(ValueError, match="above snr_db"):
        NZ.mix_at_snr(y, dn, sn, 20.0, 15.0, 16000)
    with pytest.raises(ValueError, match="no noise"):
        NZ.mix_at_snr(y, None, None, 20.0, None, 16000)


def _meter(forced_flags=None):
    """the level tool's float64 restatement behind the interface of utils.level.speech_level"""
    def level(x, fs):
        res = [LR.level_ref(r, fs, remove_mean=False) for r in np.asarray(x)]
        _meter.last = res
        return LV.SpeechLevel(np.array([r["level_db"] for r in res]), np.array([r["activity"] for r in res]), None, np.array([r["rms_db"] for r in res]),
                              None, None, np.array([r["flags"] if forced_flags is None else forced_flags for r in res]), None)
    return level


def test_active_reference_and_fallback():
    fs, L = 2000, 8000
    key = rng.stream_key(6, "half")
    y = np.zeros((1, 2, L), dtype=np.float32)
    y[0, :, :L // 2] = 0.2 * np.stack([rng.normals(key, 0, d, L // 2) for d in range(2)])         # two seconds of steady speech, two of silence
    dn = np.stack([rng.normals(key, NZ.NOISE_FIELD, d, L) for d in range(2)]).astype(np.float32)[None]
    rms = NZ.mix_at_snr(y, dn, None, 10.0, None, fs)
    act = NZ.mix_at_snr(y, dn, None, 10.0, None, fs, reference="active", level=_meter())
    res = _meter.last[0]
    assert act.reference == ["active"] and act.flags == [""] and res["flags"] == 0
    assert abs(res["activity"] - (0.5 + 0.2 * fs / L)) < 0.02                # the half that speaks plus the hangover
    got = 20.0 * math.log10(act.gain_diffuse[0] / rms.gain_diffuse[0])       # the noise follows the louder reference
    tol = LR.tol_level(res, 4096) + 2e-6                                     # the level tool's own tolerance, plus the fp32 rounding of two gains
    assert abs(got + 10.0 * math.log10(res["activity"])) <= tol
    assert abs(float(act.snr_measured_db[0]) - 10.0) < 1e-3                  # against the active power
    assert abs(float(_snr_of(act, y)[0]) - (10.0 + 10.0 * math.log10(res["activity"]))) < 1e-3      # so the rms SNR is lower by the activity
    flagged = NZ.mix_at_snr(y, dn, None, 10.0, None, fs, reference="active", level=_meter(LV.EDGE))
    assert flagged.reference == ["rms"] and flagged.flags == ["ACTIVE_FALLBACK:EDGE"]
    assert flagged.gain_diffuse[0] == rms.gain_diffuse[0] and np.array_equal(flagged.mixed, rms.mixed)
