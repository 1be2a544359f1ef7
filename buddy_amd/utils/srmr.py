"""SRMR, the speech-to-reverberation modulation energy ratio (Falk, Zheng & Chan 2010), as restated in DESIGN.md section 18: a score of a single
signal -- no clean signal is needed -- that falls as reverberation grows and does not depend on the signal's gain.  It is what the real-recordings
mode can be scored with.

``srmr`` scores rows on the GPU through ``csrc/srmr.hip`` (a 23-channel complex FIR gammatone bank, eight modulation band-pass filters on every
envelope, windowed frame energies, the band-limited ratio) and, for a rate other than 16 kHz, the project's own resampler.  It has no CPU form: a
CPU tensor raises ``BuddyHipError``.  The two banks are designed here in float64 and cached.  ``score_signals`` batches signals of several rates and
lengths; ``report_rows`` / ``summary_rows`` / ``write_report`` make the CSV report of the tester and of ``tools/srmr.py``."""
import functools
import math

import numpy as np
import torch

from .. import _lib
from . import _rows, report
from .metrics import format_summary  # noqa: F401  -- the summary as lines of text (what the tool prints)
from .report import write_report  # noqa: F401  -- the CSV conventions of every report: NaN as an empty field, repr(float)

FS = 16000                                           # the rate the analysis runs at
MIN_FS = 8000
CHANNELS, LOW_FREQ = 23, 125.0
EAR_Q, MIN_BW = 9.26449, 24.7
TAP_FLOOR = 1e-4                                     # a channel ends with the last tap whose envelope is at least this share of the envelope's peak
MOD_BANDS, MOD_Q, MOD_LOW, MOD_HIGH = 8, 2.0, 4.0, 128.0
WINDOW, HOP = 4096, 1024


def erb(f):
    return np.asarray(f, dtype=np.float64) / EAR_Q + MIN_BW


class GammatoneBank:
    """``centres`` (23,) Hz from the highest channel to the lowest; ``taps``: one complex128 array per channel, unit gain at its centre; ``lengths``"""

    def __init__(self, centres, taps):
        self.centres, self.taps = centres, taps
        self.lengths = tuple(len(t) for t in taps)


@functools.lru_cache(maxsize=None)
def gammatone_bank():
    """The analysis bank at 16 kHz, float64, cached: Slaney's ERB spacing between 125 Hz and 8 kHz, channel j the complex FIR
    g_j[n] = t^3 exp(-b_j t) exp(i 2 pi cf_j t), t = n / 16000, b_j = 2 pi 1.019 erb(cf_j), cut behind the last n >= 1 whose envelope is at least
    1e-4 of the envelope's peak (3 / b_j)^3 e^-3 and divided by its gain at cf_j."""
    c = EAR_Q * MIN_BW
    i = np.arange(1, CHANNELS + 1, dtype=np.float64)
    cf = -c + np.exp(i * (math.log(LOW_FREQ + c) - math.log(FS / 2.0 + c)) / CHANNELS) * (FS / 2.0 + c)
    taps = []
    for f in cf:
        b = 2.0 * math.pi * 1.019 * float(erb(f))
        peak = (3.0 / b) ** 3 * math.exp(-3.0)
        n = np.arange(1, int(FS))                    # the envelope of every channel is below the floor long before one second
        envl = (n / float(FS)) ** 3 * np.exp(-b * n / float(FS))
        last = int(n[envl >= TAP_FLOOR * peak][-1])
        t = np.arange(last + 1, dtype=np.float64) / float(FS)
        g = t ** 3 * np.exp(-b * t) * np.exp(2j * math.pi * f * t)
        g = g / abs(np.sum(g * np.exp(-2j * math.pi * f * t)))
        g.setflags(write=False)
        taps.append(g)
    cf.setflags(write=False)
    return GammatoneBank(cf, tuple(taps))


class ModulationBank:
    """``centres`` (8,) Hz, ``lower_edges`` (8,) Hz, ``coef`` (8, 6) float64: b0 b1 b2 a0 a1 a2 of each band-pass filter, a0 = 1"""

    def __init__(self, centres, lower_edges, coef):
        self.centres, self.lower_edges, self.coef = centres, lower_edges, coef


@functools.lru_cache(maxsize=None)
def modulation_bank():
    """Eight second-order band-pass filters, Q = 2, centres 4 * 32^(k/7) Hz, running on the envelopes at 16 kHz; float64, cached"""
    f = MOD_LOW * (MOD_HIGH / MOD_LOW) ** (np.arange(MOD_BANDS, dtype=np.float64) / (MOD_BANDS - 1))
    w = np.tan(math.pi * f / FS)
    b0 = w / MOD_Q
    a0 = 1.0 + b0 + w * w
    coef = np.stack([b0 / a0, np.zeros_like(f), -b0 / a0, np.ones_like(f), (2.0 * w * w - 2.0) / a0, (1.0 - b0 + w * w) / a0], axis=1)
    low = f * (math.sqrt(1.0 + 1.0 / (4.0 * MOD_Q * MOD_Q)) - 1.0 / (2.0 * MOD_Q))
    for a in (f, low, coef):
        a.setflags(write=False)
    return ModulationBank(f, low, coef)


def frames_of(n):
    """full frames of 4096 samples at hop 1024"""
    return (int(n) - WINDOW) // HOP + 1 if int(n) >= WINDOW else 0


_device_bank = {}


def _bank_on(device):
    """the gammatone taps as the library takes them: fp32 real and imaginary parts with a host offset table, the channels in ASCENDING centre
    frequency (the order ``buddy_srmr_scores`` visits them in), i.e. ``gammatone_bank()`` reversed"""
    key = str(device)
    if key not in _device_bank:
        bank = gammatone_bank()
        taps = bank.taps[::-1]
        off = np.concatenate([[0], np.cumsum([len(t) for t in taps])]).astype(np.int32)
        g = np.concatenate(taps)
        _device_bank[key] = (torch.from_numpy(g.real.astype(np.float32)).to(device), torch.from_numpy(g.imag.astype(np.float32)).to(device),
                             (_lib.C.c_int * len(off))(*off.tolist()))
    return _device_bank[key]


class Srmr:
    """result of ``srmr``, all on the CPU: ``values`` (B,) float64 (NaN where undefined), ``kstar`` (B,) int32: modulation bands up to K* - 1 form the
    denominator (0 where undefined), ``bandwidth`` (B,) float64: the ERB [Hz] of the channel that closes 90 % of the energy, ``frames`` (B,) int32
    full frames at 16 kHz, ``flags`` (B,) int32: 1 where the value is defined, ``samples`` (B,) int32: the samples scored per row at the input's
    rate, ``energies`` (B, 23, 8) float64: the mean frame energy per channel (in the order of ``gammatone_bank()``) and modulation band;
    ``envelope``: None, or on request the (B, 23, stride) float32 envelopes at 16 kHz on the GPU, channels in that order, valid up to each row's end"""

    def __init__(self, values, kstar, bandwidth, frames, flags, samples, energies, envelope=None):
        self.values, self.kstar, self.bandwidth, self.frames, self.flags, self.samples, self.energies = values, kstar, bandwidth, frames, flags, samples, energies
        self.envelope = envelope


def srmr(x, fs, lens=None, return_envelope=False):
    """x (B, L) float32 on the GPU at rate ``fs`` (an int >= 8000); ``lens`` (B ints, default L): valid samples per row, the rest is ignored.
    ``return_envelope`` keeps the gammatone envelopes (23 floats per sample) in the result."""
    lib, (x,), lens_t = _rows.enter((x,), lens, "srmr: the score runs on the MI355X only (got a CPU tensor)", "srmr takes a (B, L) float32 tensor", fs, MIN_FS,
                                    f"srmr: the sample rate must be an integer >= {MIN_FS} Hz, got {fs}")
    B, dev = x.shape[0], x.device
    (x16,), lens16 = _rows.to_rate((x,), lens_t, int(fs), FS)
    L16 = x16.shape[1]
    lens_d = lens16.to(dev)
    st = _lib.stream_ptr()
    g_re, g_im, off = _bank_on(dev)
    J, mod = CHANNELS, modulation_bank()
    K = MOD_BANDS
    lde = (int(lens16.max()) + 3) // 4 * 4
    env = torch.empty(B, J, lde, dtype=torch.float32, device=dev)
    _lib.check(lib.buddy_gammatone_env(_lib.ptr(x16), lens_d.data_ptr(), B, L16, _lib.ptr(g_re), _lib.ptr(g_im), off, J, _lib.ptr(env), lde, st))
    ldm = max(frames_of(int(lens16.max())), 1)
    E = torch.empty(B, J, K, ldm, dtype=torch.float64, device=dev)
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    coef = (_lib.C.c_double * (K * 6))(*mod.coef.reshape(-1).tolist())
    _lib.check(lib.buddy_modulation_energies(_lib.ptr(env), lens_d.data_ptr(), B, J, lde, coef, K, WINDOW, HOP, E.data_ptr(), ldm, frames.data_ptr(), st))
    out = torch.empty(B, 3, dtype=torch.float64, device=dev)
    ebar = torch.empty(B, J, K, dtype=torch.float64, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    erbs = (_lib.C.c_double * J)(*erb(gammatone_bank().centres[::-1]).tolist())
    low = (_lib.C.c_double * K)(*mod.lower_edges.tolist())
    _lib.check(lib.buddy_srmr_scores(E.data_ptr(), frames.data_ptr(), B, J, K, ldm, erbs, low, out.data_ptr(), ebar.data_ptr(), flags.data_ptr(), st))
    out = out.cpu()
    ks = out[:, 1]
    kstar = torch.where(torch.isnan(ks), torch.zeros_like(ks), ks).to(torch.int32)
    return Srmr(out[:, 0].clone(), kstar, out[:, 2].clone(), frames.cpu(), flags.cpu(), lens_t.clone(), ebar.cpu().flip(1), env.flip(1) if return_envelope else None)


# ---- signals of several rates and lengths -------------------------------------------------------------------------------------------------------
BATCH_SAMPLES = 1 << 21                              # padded input samples per call: bounds the envelope array (23 floats per sample at 16 kHz)


def score_signals(signals, device):
    """``signals``: (1-D float32 tensor or array, rate) pairs -> one dict per signal (``srmr``, ``kstar``, ``bw``, ``flags``, ``frames``, ``samples``).
    Signals of one rate go through ``srmr`` as zero-padded batches with ``lens``; a row's result does not depend on its batch."""
    rows = [None] * len(signals)
    by_rate = {}
    for i, (_, fs) in enumerate(signals):
        by_rate.setdefault(int(fs), []).append(i)
    for fs, idx in by_rate.items():
        idx = sorted(idx, key=lambda i: len(signals[i][0]))         # neighbours in length share a batch: little padding
        s = 0
        while s < len(idx):
            e = s + 1
            while e < len(idx) and (e + 1 - s) * len(signals[idx[e]][0]) <= BATCH_SAMPLES:
                e += 1
            part = idx[s:e]
            lens = [len(signals[i][0]) for i in part]
            xb = torch.zeros(len(part), max(lens), dtype=torch.float32, device=device)
            for b, i in enumerate(part):
                xb[b, :lens[b]] = torch.as_tensor(signals[i][0], dtype=torch.float32).flatten().to(device)
            r = srmr(xb, fs, lens=lens)
            for b, i in enumerate(part):
                rows[i] = {"srmr": float(r.values[b]), "kstar": int(r.kstar[b]), "bw": float(r.bandwidth[b]), "flags": int(r.flags[b]),
                           "frames": int(r.frames[b]), "samples": int(r.samples[b])}
            s = e
    return rows


# ---- the CSV report ------------------------------------------------------------------------------------------------------------------------
_UNSCORED = {"srmr": float("nan"), "kstar": 0, "bw": float("nan"), "flags": 0, "frames": 0, "samples": 0}


def report_rows(names, inp, out, clean=None):
    """one dict per file from the ``score_signals`` rows of the degraded input (``inp``; None: those columns stay empty), of the reconstruction
    (``out``) and, in a paired mode, of the clean signal (``clean``)"""
    rows = []
    for b, name in enumerate(names):
        i, o = (_UNSCORED if inp is None else inp[b]), out[b]
        row = {"file": name, "samples_in": i["samples"], "samples_out": o["samples"], "srmr_in": i["srmr"], "srmr_out": o["srmr"],
               "srmr_delta": o["srmr"] - i["srmr"], "kstar_in": i["kstar"], "kstar_out": o["kstar"], "bw_in": i["bw"], "bw_out": o["bw"],
               "flags_in": i["flags"], "flags_out": o["flags"], "frames_in": i["frames"], "frames_out": o["frames"]}
        if clean is not None:
            row["srmr_clean"], row["kstar_clean"], row["bw_clean"] = clean[b]["srmr"], clean[b]["kstar"], clean[b]["bw"]
        rows.append(row)
    return rows


def summary_rows(rows):
    """one dict per ``srmr_*`` column of ``report_rows``: the number of files where it is defined, and their mean, median and standard deviation
    (numpy's, population form); NaN where no file defines it"""
    return report.summarise(rows, lambda col: col.startswith("srmr_"))
