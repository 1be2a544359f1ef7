"""Blind decay time: how long a signal's own free decays -- the stretches after speech offsets in which its energy only falls -- would take to fall
by 60 dB, broadband and per octave band, as defined in DESIGN.md section 30 (the free-decay-region family of Prego, de Lima, Netto & Lee 2012 and
Loellmann et al. 2010, restated there with every constant fixed).  It needs neither a clean signal nor an impulse response, so it scores the
degraded and the reconstructed signal of every mode in seconds ("0.71 s in, 0.24 s out").

``decay_times`` scores rows on the GPU through ``csrc/decay.hip`` (band energies of 512-sample frames, smoothing, the regions and their slopes, an
exact select of the median and quartiles) and, for a rate other than 16 kHz, the project's own resampler.  It has no CPU form: a CPU tensor raises
``BuddyHipError``.  ``score_signals`` batches signals of several rates and lengths; ``report_rows`` / ``summary_rows`` / ``write_report`` make the
CSV report of the tester and of ``tools/decay.py``."""
import math

import torch

from .. import _lib
from . import _rows, report
from .report import write_report  # noqa: F401  -- the CSV conventions of every report: NaN as an empty field, repr(float)

FS = 16000                                           # the rate the analysis runs at
MIN_FS = 8000
FRAME, HOP = 512, 128
BIN_HZ = FS / FRAME                                  # 31.25
K_SMOOTH = 5                                         # frames summed into one smoothed value
BROADBAND = (88.39, 5656.85)                         # Hz: the lower edge of the 125 Hz octave to the upper edge of the 4 kHz octave
CENTRES = (125, 250, 500, 1000, 2000, 4000)
BANDS = 1 + len(CENTRES)
RATE_SHARE = 0.45                                    # a band must end below this share of the input's rate
DEFINED, FEW, ABOVE_RATE, SHORT = 1, 2, 4, 8
NAMES = ("t60",) + tuple(f"t60_{f}" for f in CENTRES)      # the report's name of each band


def frames_of(n):
    """full frames of 512 samples at hop 128"""
    return (int(n) - FRAME) // HOP + 1 if int(n) >= FRAME else 0


def band_edges(fs):
    """[(lo, hi, above)] per band in Hz for an input at rate ``fs``: band 0 broadband with its upper edge clipped to 0.45 fs, bands 1..6 the octaves
    [f / sqrt 2, f sqrt 2); ``above``: the octave's upper edge exceeds 0.45 fs, which leaves the band undefined"""
    top = RATE_SHARE * float(fs)
    edges = [(BROADBAND[0], min(BROADBAND[1], top), False)]
    r = math.sqrt(2.0)
    for f in CENTRES:
        edges.append((f / r, f * r, f * r > top))
    return edges


def bin_ranges(fs):
    """(lo_bins, hi_bins, above) per band: the bins k whose centre k * 31.25 Hz lies in [lo, hi); an undefined band is the empty range (0, 0)"""
    lo, hi, above = [], [], []
    for a, b, ab in band_edges(fs):
        lo.append(0 if ab else int(math.ceil(a / BIN_HZ)))
        hi.append(0 if ab else min(int(math.ceil(b / BIN_HZ)), FRAME // 2 + 1))
        above.append(ab)
    return lo, hi, above


def flag_word(n, frames, above, lmin):
    """the flag word of a (row, band) from its kept regions, its row's frames and whether its band is above the rate"""
    return (DEFINED if n >= 1 else 0) | (FEW if n < 3 else 0) | (ABOVE_RATE if above else 0) | (SHORT if frames < K_SMOOTH + lmin else 0)


class DecayTimes:
    """result of ``decay_times``, all on the CPU: ``t60``, ``q1``, ``q3`` (B, 7) float64 seconds: the lower median and the quartiles of the regions'
    decay times per band (band 0 broadband, 1..6 the octaves at 125 .. 4000 Hz; NaN where no region is kept), ``regions`` (B, 7) int32 kept regions,
    ``flags`` (B, 7) int32 (DEFINED = 1, FEW = 2, ABOVE_RATE = 4, SHORT = 8), ``frames`` (B,) int32 full frames at 16 kHz, ``samples`` (B,) int32:
    the samples scored per row at the input's rate"""

    def __init__(self, t60, q1, q3, regions, flags, frames, samples):
        self.t60, self.q1, self.q3, self.regions, self.flags, self.frames, self.samples = t60, q1, q3, regions, flags, frames, samples


def decay_times(x, fs, lens=None, drop_db=10.0, floor_db=-60.0, lmin=6):
    """x (B, L) float32 on the GPU at rate ``fs`` (an int >= 8000); ``lens`` (B ints, default L): valid samples per row, the rest is ignored.
    ``drop_db``: a region must fall by at least this much; ``floor_db``: smoothed energies this far below the row's largest end a region;
    ``lmin``: the fewest frames of a region."""
    lib, (x,), lens_t = _rows.enter((x,), lens, "decay_times: the measure runs on the MI355X only (got a CPU tensor)", "decay_times takes a (B, L) float32 tensor",
                                    fs, MIN_FS, f"decay_times: the sample rate must be an integer >= {MIN_FS} Hz, got {fs}")
    if not (drop_db > 0.0 and floor_db < 0.0 and int(lmin) == lmin and lmin >= 2):
        raise ValueError(f"decay_times: drop_db must be > 0, floor_db < 0 and lmin an integer >= 2, got {drop_db}, {floor_db}, {lmin}")
    B, dev = x.shape[0], x.device
    (x16,), lens16 = _rows.to_rate((x,), lens_t, int(fs), FS)
    lens_d = lens16.to(dev)
    st = _lib.stream_ptr()
    lo, hi, above = bin_ranges(int(fs))
    NB = BANDS
    ldm = max(frames_of(int(lens16.max())), 1)
    E = torch.empty(B, NB, ldm, dtype=torch.float64, device=dev)
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.buddy_decay_energies(_lib.ptr(x16), lens_d.data_ptr(), B, x16.shape[1], (_lib.C.c_int * NB)(*lo), (_lib.C.c_int * NB)(*hi), NB, E.data_ptr(),
                                        ldm, frames.data_ptr(), st))
    T = torch.empty(B, NB, ldm, dtype=torch.float64, device=dev)
    rl = torch.empty(B, NB, ldm, dtype=torch.int32, device=dev)
    q, floor_rel = 10.0 ** (-float(drop_db) / 10.0), 10.0 ** (float(floor_db) / 10.0)
    _lib.check(lib.buddy_decay_regions(E.data_ptr(), frames.data_ptr(), B, NB, ldm, K_SMOOTH, int(lmin), q, floor_rel, T.data_ptr(), rl.data_ptr(), st))
    out = torch.empty(B, NB, 3, dtype=torch.float64, device=dev)
    counts = torch.empty(B, NB, dtype=torch.int32, device=dev)
    _lib.check(lib.buddy_decay_select(T.data_ptr(), frames.data_ptr(), B, NB, ldm, out.data_ptr(), counts.data_ptr(), st))
    out, counts, frames = out.cpu(), counts.cpu(), frames.cpu()
    flags = torch.tensor([[flag_word(int(counts[b, i]), int(frames[b]), above[i], int(lmin)) for i in range(NB)] for b in range(B)], dtype=torch.int32)
    return DecayTimes(out[:, :, 0].clone(), out[:, :, 1].clone(), out[:, :, 2].clone(), counts, flags, frames, lens_t.clone())


# ---- signals of several rates and lengths -------------------------------------------------------------------------------------------------------
BATCH_SAMPLES = 1 << 23                              # padded input samples per call


def score_signals(signals, device):
    """``signals``: (1-D float32 tensor or array, rate) pairs -> one dict per signal: ``t60``, ``q1``, ``q3``, ``regions``, ``flags`` (lists of 7, band 0
    broadband), ``frames``, ``samples``.  Signals of one rate go through ``decay_times`` as zero-padded batches with ``lens``; a row's result does not
    depend on its batch."""
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
            r = decay_times(xb, fs, lens=lens)
            for b, i in enumerate(part):
                rows[i] = {"t60": r.t60[b].tolist(), "q1": r.q1[b].tolist(), "q3": r.q3[b].tolist(), "regions": r.regions[b].tolist(),
                           "flags": r.flags[b].tolist(), "frames": int(r.frames[b]), "samples": int(r.samples[b])}
            s = e
    return rows


# ---- the CSV report ------------------------------------------------------------------------------------------------------------------------
_NAN7, _ZERO7 = [float("nan")] * BANDS, [0] * BANDS
_UNSCORED = {"t60": _NAN7, "q1": _NAN7, "q3": _NAN7, "regions": _ZERO7, "flags": _ZERO7, "frames": 0, "samples": 0}


def report_rows(names, inp, out, clean=None):
    """one dict per file from the ``score_signals`` rows of the degraded input (``inp``; None: those columns stay empty), of the reconstruction
    (``out``) and, in a paired mode, of the clean signal (``clean``: the floor that speech itself sets).  Columns: the decay times ``t60_*``
    (broadband) and ``t60_<f>_*`` per octave, then per band the kept regions, the spread q3 - q1 and the flag word."""
    rows = []
    for b, name in enumerate(names):
        i, o = (_UNSCORED if inp is None else inp[b]), out[b]
        row = {"file": name, "samples_in": i["samples"], "samples_out": o["samples"], "frames_in": i["frames"], "frames_out": o["frames"]}
        for k, n in enumerate(NAMES):
            row[n + "_in"], row[n + "_out"], row[n + "_delta"] = i["t60"][k], o["t60"][k], o["t60"][k] - i["t60"][k]
        for col, get in (("regions", lambda r, k: r["regions"][k]), ("spread", lambda r, k: r["q3"][k] - r["q1"][k]), ("flags", lambda r, k: r["flags"][k])):
            for k, n in enumerate(NAMES):
                row[col + n[3:] + "_in"], row[col + n[3:] + "_out"] = get(i, k), get(o, k)
        if clean is not None:
            for k, n in enumerate(NAMES):
                row[n + "_clean"] = clean[b]["t60"][k]
            for k, n in enumerate(NAMES):
                row["regions" + n[3:] + "_clean"] = clean[b]["regions"][k]
        rows.append(row)
    return rows


def summary_rows(rows):
    """one dict per ``t60*`` column of ``report_rows``: the number of files where it is defined, and their mean, median and standard deviation
    (numpy's, population form); NaN where no file defines it"""
    return report.summarise(rows, lambda col: col.startswith("t60"))


def format_summary(summary):
    """the summary as lines of text (what the tool prints)"""
    return report.format_summary(summary, 16, 4)
