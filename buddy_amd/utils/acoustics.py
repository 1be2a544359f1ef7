"""Room-acoustic parameters of room impulse responses (ISO 3382-1; definitions in DESIGN.md section 16): per RIR row and band -- broadband,
then octave bands -- the decay times EDT, T20 and T30 from the Schroeder curve, clarity C50, direct-to-reverberant ratio DRR and centre time Ts.
No reference counterpart: the reference writes its estimated RIRs to wav files and stops there.

The octave filters are designed on the host in double (numpy only) and go to the device as fp32, the same split as ``utils/resample.design_filter``;
the analysis is three library calls (``buddy_row_argmax_abs``, ``buddy_fir_bank``, ``buddy_decay_metrics``; ``csrc/acoustics.hip``) and has no CPU
form: a CPU tensor raises ``BuddyHipError``."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from .. import _lib
from .report import write_report

OCTAVES = (125, 250, 500, 1000, 2000, 4000)
VALUES = ("EDT", "T20", "T30", "C50", "DRR", "Ts")        # order of the last axis of ``values``; flag bit q = value q is defined
FIT_VALID_BIT = 6                                          # flag bit 6 + q: the fit of decay time q (EDT, T20, T30) is valid (not bent by truncation)
ERROR_VALUES = ("EDT", "T20", "T30", "C50", "DRR")         # values whose signed error (estimate - true) the paired report carries


def octave_bank(fs, centres=OCTAVES, beta=5.0, periods=8):
    """(len(centres), Nh) float64, one zero-phase band-pass per centre ``fc``: the ideal band-pass with edges fc / sqrt 2 and fc * sqrt 2 under a
    Kaiser window (``beta``) of ``ceil(periods * fs / fc) | 1`` taps, centred and zero-padded to the one odd length ``Nh`` of the longest filter.
    A centre whose upper edge exceeds 0.45 fs is refused.  Cached per argument tuple (the same read-only array on every call)."""
    return _octave_bank(float(fs), tuple(float(c) for c in centres), float(beta), float(periods))


@functools.lru_cache(maxsize=None)
def _octave_bank(fs, centres, beta, periods):
    assert fs > 0 and all(c > 0 for c in centres), "rate and centres must be positive"
    for fc in centres:
        if fc * math.sqrt(2.0) > 0.45 * fs:
            raise ValueError(f"octave_bank: the {fc:g} Hz band reaches {fc * math.sqrt(2.0):.0f} Hz, above 0.45 fs = {0.45 * fs:.0f} Hz")
    lengths = [int(math.ceil(periods * fs / fc)) | 1 for fc in centres]
    Nh = max(lengths, default=1)
    bank = np.zeros((len(centres), Nh), dtype=np.float64)
    for k, (fc, n_taps) in enumerate(zip(centres, lengths)):
        half = (n_taps - 1) // 2
        n = np.arange(-half, half + 1, dtype=np.float64)
        lo, hi = 2.0 * fc / math.sqrt(2.0) / fs, 2.0 * fc * math.sqrt(2.0) / fs      # edges in units of the Nyquist rate
        taps = (hi * np.sinc(hi * n) - lo * np.sinc(lo * n)) * np.kaiser(n_taps, float(beta))
        bank[k, (Nh - 1) // 2 - half:(Nh - 1) // 2 + half + 1] = taps
    bank.setflags(write=False)
    return bank


def analysis_bank(fs, centres=OCTAVES):
    """(1 + len(centres), Nh) float64: row 0 is the broadband band, a unit impulse at the centre tap, then ``octave_bank(fs, centres)``"""
    oct_rows = octave_bank(fs, tuple(centres))
    bank = np.zeros((1 + oct_rows.shape[0], oct_rows.shape[1]), dtype=np.float64)
    bank[0, (bank.shape[1] - 1) // 2] = 1.0
    bank[1:] = oct_rows
    return bank


_device_banks = {}


def _bank_on(fs, centres, device):
    key = (int(fs), tuple(float(c) for c in centres), str(device))
    if key not in _device_banks:
        _device_banks[key] = torch.from_numpy(analysis_bank(fs, centres).astype(np.float32)).to(device)
    return _device_banks[key]


class RirAcoustics:
    """result of ``rir_acoustics``: ``bands`` (0.0 = broadband, then the centres in Hz), ``values`` (B, nb, 6) float64 on the CPU in the order
    ``VALUES`` (seconds, dB, dB, seconds; NaN where undefined), ``flags`` (B, nb) int32 on the CPU, ``n0`` (B,) int32 on the CPU, ``edc_db``
    (B, nb, N + P) float32 on the device or None (NaN outside the analysed part of a row)"""

    def __init__(self, bands, values, flags, n0, edc_db=None):
        self.bands, self.values, self.flags, self.n0, self.edc_db = bands, values, flags, n0, edc_db


def rir_acoustics(h, fs, lens=None, centres=OCTAVES, return_edc=False):
    """h (B, N) float32 on the GPU, one RIR per row at rate ``fs`` (an int); ``lens`` (B ints, default N): valid samples per row, the rest is ignored"""
    if not isinstance(h, torch.Tensor) or not h.is_cuda:
        raise _lib.BuddyHipError("rir_acoustics: the analysis runs on the MI355X only (got a CPU tensor)")
    lib = _lib.require_gpu()
    assert h.dim() == 2 and h.dtype == torch.float32, "rir_acoustics takes (B, N) float32"
    assert int(fs) == fs, "rir_acoustics takes an integer sample rate"
    fs = int(fs)
    h = h.contiguous()
    B, N = h.shape
    dev = h.device
    lens_t = torch.full((B,), N, dtype=torch.int32) if lens is None else torch.as_tensor(lens, dtype=torch.int32).reshape(B).cpu()
    bank = _bank_on(fs, centres, dev)
    nb, Nh = bank.shape
    P = (Nh - 1) // 2
    ldg = N + P
    lens_d, lens_g = lens_t.to(dev), (lens_t + P).to(dev)
    n0 = torch.empty(B, dtype=torch.int32, device=dev)
    g = torch.empty(B, nb, ldg, dtype=torch.float32, device=dev)
    out = torch.empty(B, nb, 6, dtype=torch.float64, device=dev)
    flags = torch.empty(B, nb, dtype=torch.int32, device=dev)
    edc = torch.full((B, nb, ldg), float("nan"), dtype=torch.float32, device=dev) if return_edc else None
    st = _lib.stream_ptr()
    _lib.check(lib.buddy_row_argmax_abs(_lib.ptr(h), lens_d.data_ptr(), B, N, n0.data_ptr(), st))
    _lib.check(lib.buddy_fir_bank(_lib.ptr(h), lens_d.data_ptr(), B, N, _lib.ptr(bank), nb, Nh, _lib.ptr(g), ldg, st))
    _lib.check(lib.buddy_decay_metrics(_lib.ptr(g), lens_g.data_ptr(), n0.data_ptr(), B, nb, ldg, fs, out.data_ptr(), flags.data_ptr(), _lib.ptr(edc), st))
    return RirAcoustics((0.0,) + tuple(float(c) for c in centres), out.cpu(), flags.cpu(), n0.cpu(), edc)


# ---- CSV reports (written by utils/report.py: NaN as an empty field, flags as an integer) ---------------------------------------------------------
def band_label(band):
    return "broadband" if float(band) == 0.0 else f"{float(band):g}"


def report_rows(names, est, true=None):
    """one dict per (name, band) from a ``RirAcoustics`` of the estimates (rows in the order of ``names``) and, optionally, of the true RIRs:
    ``true_*`` values and flags, and the signed errors estimate - true of ``ERROR_VALUES``"""
    rows = []
    for b, name in enumerate(names):
        for k, band in enumerate(est.bands):
            row = {"file": name, "band": band_label(band)}
            for q, v in enumerate(VALUES):
                row[v] = float(est.values[b, k, q])
            row["flags"] = int(est.flags[b, k])
            if true is not None:
                for q, v in enumerate(VALUES):
                    row["true_" + v] = float(true.values[b, k, q])
                row["true_flags"] = int(true.flags[b, k])
                for v in ERROR_VALUES:
                    row["err_" + v] = row[v] - row["true_" + v]
            rows.append(row)
    return rows


def parameter_rows(names, params):
    """one dict per (name, exponential, knot) from ``BlindSubbandFiltering.acoustic_parameters()``; ``names[b]`` is operator row b"""
    rows = []
    freqs, t60, wts = params["freqs"], params["T60"], params["weights"]
    for b, name in enumerate(names):
        for e in range(t60.shape[1]):
            for j, fq in enumerate(freqs):
                rows.append({"file": name, "exponential": e, "freq_hz": float(fq), "T60": float(t60[b, e, j]), "weight": float(wts[b, e, j])})
    return rows


def write_parameters(path, rows):
    write_report(path, rows)
