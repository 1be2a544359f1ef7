"""SI-SDR (not in the reference): 10 log10(||a s||^2 / ||a s - s_hat||^2), a = <s_hat,s>/||s||^2, zero-mean.

``evaluate`` scores (estimate, clean) pairs on the GPU -- SI-SDR, STOI, ESTOI and the log-spectral distance, definitions in DESIGN.md section 17 --
through ``csrc/metrics.hip`` and, for the 10 kHz step of STOI, the project's own resampler.  It has no CPU form: a CPU tensor raises
``BuddyHipError``.  ``report_rows`` / ``summary_rows`` / ``write_report`` turn two evaluations (input and output of a run against the clean
signals) into the CSV report of the tester and of ``tools/evaluate.py``.  ``align`` (``csrc/align.hip``) estimates one integer
lag per pair and trims the pair to its overlap; ``evaluate(..., align=ms)`` scores after it.  It is off unless asked for."""
import functools

import numpy as np
import torch

from .. import _lib
from . import _rows, report
from .report import write_report  # noqa: F401  -- the CSV conventions of every report: NaN as an empty field, repr(float)


def si_sdr(est, ref):
    est = est.double() - est.double().mean(-1, keepdim=True)
    ref = ref.double() - ref.double().mean(-1, keepdim=True)
    a = (est * ref).sum(-1, keepdim=True) / (ref * ref).sum(-1, keepdim=True).clamp_min(1e-30)
    t = a * ref
    return 10 * torch.log10((t * t).sum(-1) / ((t - est) ** 2).sum(-1).clamp_min(1e-30))


VALUES = ("si_sdr", "stoi", "estoi", "lsd")         # order of the last axis of ``Evaluation.values``; flag bit q = value q is defined
STOI_FS = 10000                                      # the rate STOI and ESTOI are defined at
FRAME, HOP, NFFT, SEGMENT = 256, 128, 512, 30


@functools.lru_cache(maxsize=None)
def third_octave_bands(fs=STOI_FS, nfft=NFFT, num_bands=15, first_centre=150.0):
    """((lo, hi),) * num_bands: band j is the bins [lo, hi) of an ``nfft``-point transform at ``fs``, from the bin nearest the lower edge
    cf_j 2^(-1/6) to the bin nearest the upper edge cf_j 2^(1/6), cf_j = first_centre 2^(j/3).  Designed in float64, cached."""
    f = np.arange(nfft // 2 + 1, dtype=np.float64) * (float(fs) / nfft)
    cf = float(first_centre) * 2.0 ** (np.arange(num_bands, dtype=np.float64) / 3.0)
    lo = [int(np.argmin(np.abs(f - c * 2.0 ** (-1.0 / 6.0)))) for c in cf]
    hi = [int(np.argmin(np.abs(f - c * 2.0 ** (1.0 / 6.0)))) for c in cf]
    return tuple(zip(lo, hi))


def frames_of(n):
    """full frames of 256 samples at hop 128"""
    return (int(n) - FRAME) // HOP + 1 if int(n) >= FRAME else 0


class Evaluation:
    """result of ``evaluate``: ``values`` (B, 4) float64 on the CPU in the order ``VALUES`` (dB, 0..1, 0..1, dB; NaN where undefined or not asked
    for), ``flags`` (B,) int32 (bit q: value q is defined), ``kept_frames`` / ``frames`` (B,) int32: the 10 kHz frames STOI kept and had,
    ``samples`` (B,) int32: the samples scored per row, ``names``: the values asked for"""

    def __init__(self, values, flags, kept_frames, frames, samples, names, alignment=None):
        self.values, self.flags, self.kept_frames, self.frames, self.samples, self.names = values, flags, kept_frames, frames, samples, names
        self.alignment = alignment                   # the ``Alignment`` the rows were scored after (``evaluate(..., align=ms)``), or None

    @classmethod
    def blank_like(cls, out):
        """the "before" side of a report without input signals: no value, no flag, the clean signal's frame counts and the samples of ``out``"""
        return cls(torch.full_like(out.values, float("nan")), torch.zeros_like(out.flags), out.kept_frames, out.frames, out.samples, out.names)


ALIGN_FLAGS = ("defined", "edge", "inverted")        # bits 0..2 of ``Alignment.flags``
MAX_LAG_MS = 50.0                                    # default search window: +-50 ms, about 17 m of path difference.  A choice, not a measurement


class Alignment:
    """result of ``align``: per row ``lag`` (B,) int32 -- positive: the estimate is late --, ``rho`` (B,) float64: the normalised cross-correlation at
    that lag, signed, ``frac`` (B,) float64: the sub-sample offset of the peak by a parabola through its neighbours (reported, never applied),
    ``flags`` (B,) int32 (bit 0: defined, bit 1: the peak lies on the edge of the window, bit 2: rho < 0), all on the CPU; ``est``, ``ref`` (B, L) on the
    GPU: the pair shifted to its overlap, zeros behind it, and ``lens`` (B,) int32 on the CPU: the overlap, input length - |lag|; ``max_lag``: the
    window K in samples, ``fs``: the rate.  A row that is not defined (fewer than two samples, a constant or non-finite signal) has lag 0 and rho NaN."""

    def __init__(self, lag, rho, frac, flags, est, ref, lens, max_lag, fs):
        self.lag, self.rho, self.frac, self.flags, self.est, self.ref, self.lens, self.max_lag, self.fs = lag, rho, frac, flags, est, ref, lens, max_lag, fs


def align(est, ref, fs, lens=None, max_lag_ms=MAX_LAG_MS):
    """Time-align (B, L) float32 estimates to their clean signals on the GPU (``csrc/align.hip``): one integer lag per row, the
    largest |cross-correlation| of the zero-mean signals within +-K = round(max_lag_ms fs / 1000) samples, and both signals trimmed to the
    overlap.  ``lens`` as in ``evaluate``.  Returns an ``Alignment``."""
    lib, (est, ref), lens_t = _rows.enter((est, ref), lens, "align: the alignment runs on the MI355X only (got a CPU tensor)",
                                          "align takes two (B, L) float32 tensors")
    K = int(round(float(max_lag_ms) * float(fs) / 1000.0))
    if not 0 <= K <= 65535:
        raise ValueError(f"align: max_lag_ms = {max_lag_ms} at {fs} Hz is a window of {K} samples; it must be in 0..65535")
    B, L = est.shape
    dev = est.device
    lens_d = lens_t.to(dev)
    st = _lib.stream_ptr()
    lag, flags, lens_o = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    out = torch.empty(B, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.buddy_xcorr_lag_workspace(B, int(lens_t.max()), K) // 8, dtype=torch.float64, device=dev)
    _lib.check(lib.buddy_xcorr_lag(_lib.ptr(est), _lib.ptr(ref), lens_d.data_ptr(), B, L, K, lag.data_ptr(), out.data_ptr(), flags.data_ptr(), None,
                                   ws.data_ptr(), ws.numel() * 8, st))
    eo, xo = torch.empty_like(est), torch.empty_like(ref)
    _lib.check(lib.buddy_align_pair(_lib.ptr(est), _lib.ptr(ref), lens_d.data_ptr(), lag.data_ptr(), B, L, _lib.ptr(eo), _lib.ptr(xo), L, lens_o.data_ptr(), st))
    out = out.cpu()
    return Alignment(lag.cpu(), out[:, 0].clone(), out[:, 1].clone(), flags.cpu(), eo, xo, lens_o.cpu(), K, fs)


_align = align                                       # ``evaluate`` has a keyword of the same name


def evaluate(est, ref, fs, lens=None, values=VALUES, align=None):
    """est, ref (B, L) float32 on the GPU at rate ``fs`` (an int >= 10 000): the estimates and the clean signals, row by row; ``lens`` (B ints,
    default L): valid samples per row, the rest is ignored.  ``align`` = None: no time alignment, the pairs are scored as they are.  ``align`` = a
    search window in ms: every pair is first shifted by its own integer lag and trimmed to the overlap (``align`` above); the result carries the
    ``Alignment`` and ``samples`` is the overlap."""
    lib, (est, ref), lens_t = _rows.enter(
        (est, ref), lens, "evaluate: the metrics run on the MI355X only (got a CPU tensor)", "evaluate takes two (B, L) float32 tensors", fs, STOI_FS,
        f"evaluate: the sample rate must be an integer >= {STOI_FS} Hz (STOI is defined at 10 kHz and nothing here upsamples to it), got {fs}")
    names = tuple(v for v in VALUES if v in tuple(values))
    unknown = sorted(set(values) - set(VALUES))
    if unknown:
        raise ValueError(f"evaluate: unknown values {unknown}; known: {list(VALUES)}")
    fs = int(fs)
    B, L = est.shape
    dev = est.device
    alignment = None
    if align is not None:
        alignment = _align(est, ref, fs, lens=lens_t, max_lag_ms=float(align))
        est, ref, lens_t = alignment.est, alignment.ref, _rows.lengths(alignment.lens, B, L)
    lens_d = lens_t.to(dev)
    st = _lib.stream_ptr()
    out = torch.full((B, 4), float("nan"), dtype=torch.float64)
    flags = torch.zeros(B, dtype=torch.int32)
    kept, frames = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)

    mom = torch.empty(B, 4, dtype=torch.float64, device=dev)
    mom_fl = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.buddy_pair_moments(_lib.ptr(est), _lib.ptr(ref), lens_d.data_ptr(), B, L, mom.data_ptr(), mom_fl.data_ptr(), st))
    if "si_sdr" in names:
        out[:, 0] = mom[:, 3].cpu()
        flags |= mom_fl.cpu()

    if "stoi" in names or "estoi" in names:
        (e10, x10), lens10 = _rows.to_rate((est, ref), lens_t, fs, STOI_FS)
        L10 = x10.shape[1]
        lens10_d = lens10.to(dev)
        maxF = frames_of(int(lens10.max()))
        ldf, ldo = max(maxF, 1), max((maxF - 1) * HOP + FRAME, 1)
        xo, eo = torch.empty(B, ldo, dtype=torch.float32, device=dev), torch.empty(B, ldo, dtype=torch.float32, device=dev)
        lens_o, K, F = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
        src = torch.empty(B, ldf, dtype=torch.int32, device=dev)
        ws = torch.empty(B * ldf, dtype=torch.float64, device=dev)
        _lib.check(lib.buddy_stoi_select(_lib.ptr(x10), _lib.ptr(e10), lens10_d.data_ptr(), B, L10, _lib.ptr(xo), _lib.ptr(eo), ldo, lens_o.data_ptr(),
                                         K.data_ptr(), F.data_ptr(), src.data_ptr(), ldf, ws.data_ptr(), ws.numel() * 8, st))
        kept, frames = K.cpu(), F.cpu()
        ldm = max(int(kept.max()), 1)            # a signal rebuilt from K frames has K full frames
        bands = third_octave_bands()
        J = len(bands)
        lo, hi = (_lib.C.c_int * J)(*[b[0] for b in bands]), (_lib.C.c_int * J)(*[b[1] for b in bands])
        X, Y = torch.empty(B, J, ldm, dtype=torch.float32, device=dev), torch.empty(B, J, ldm, dtype=torch.float32, device=dev)
        _lib.check(lib.buddy_band_spectra(_lib.ptr(xo), lens_o.data_ptr(), B, ldo, lo, hi, J, _lib.ptr(X), ldm, st))
        _lib.check(lib.buddy_band_spectra(_lib.ptr(eo), lens_o.data_ptr(), B, ldo, lo, hi, J, _lib.ptr(Y), ldm, st))
        sc = torch.empty(B, 2, dtype=torch.float64, device=dev)
        sc_fl = torch.empty(B, dtype=torch.int32, device=dev)
        ws2 = torch.empty(lib.buddy_stoi_scores_workspace(B, ldm) // 8, dtype=torch.float64, device=dev)
        _lib.check(lib.buddy_stoi_scores(_lib.ptr(X), _lib.ptr(Y), K.data_ptr(), B, J, ldm, sc.data_ptr(), sc_fl.data_ptr(), ws2.data_ptr(), ws2.numel() * 8, st))
        sc, sc_fl = sc.cpu(), sc_fl.cpu()
        for q, name in ((1, "stoi"), (2, "estoi")):
            if name in names:
                out[:, q] = sc[:, q - 1]
                flags |= sc_fl << q

    if "lsd" in names:
        ws = torch.empty(lib.buddy_lsd_workspace(B, int(lens_t.max())) // 8, dtype=torch.float64, device=dev)
        mean_p = torch.empty(B, dtype=torch.float64, device=dev)
        _lib.check(lib.buddy_frame_power(_lib.ptr(ref), lens_d.data_ptr(), B, L, mean_p.data_ptr(), ws.data_ptr(), ws.numel() * 8, st))
        gain = _rows.pair_gain(mom)
        delta = (1e-8 * mean_p).contiguous()
        lsd = torch.empty(B, dtype=torch.float64, device=dev)
        lsd_fl = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(lib.buddy_lsd(_lib.ptr(est), _lib.ptr(ref), lens_d.data_ptr(), B, L, gain.data_ptr(), delta.data_ptr(), lsd.data_ptr(), lsd_fl.data_ptr(),
                                 ws.data_ptr(), ws.numel() * 8, st))
        out[:, 3] = lsd.cpu()
        flags |= lsd_fl.cpu() << 3
    return Evaluation(out, flags, kept, frames, lens_t.clone(), names, alignment)


# ---- the CSV report ------------------------------------------------------------------------------------------------------------------------
def report_rows(names, inp, out):
    """one dict per file from two ``Evaluation``s of the same rows against the clean signals -- ``inp``: the degraded input, ``out``: the
    reconstruction: ``<m>_in``, ``<m>_out`` and ``<m>_delta`` = out - in per value asked for, both flag words, and the frame counts of the
    clean signal (the same in both).  Where an evaluation carries an ``Alignment`` the row ends with ``lag_in`` / ``lag_out`` (samples, positive: late),
    ``lag_ms_*``, ``xcorr_*`` (rho) and ``align_flags_*``; the side without one has empty fields and flag word 0.  Without any, the columns are those
    above and nothing else."""
    rows = []
    for b, name in enumerate(names):
        row = {"file": name, "samples": int(out.samples[b]), **report.delta_columns(VALUES, out.names, inp, out, b)}
        row["flags_in"], row["flags_out"] = int(inp.flags[b]), int(out.flags[b])
        row["kept_frames"], row["frames"] = int(out.kept_frames[b]), int(out.frames[b])
        row.update(report.alignment_columns(inp, out, b))
        rows.append(row)
    return rows


def summary_rows(rows):
    """one dict per value column of ``report_rows``: the number of files where it is defined, and their mean, median and standard deviation
    (numpy's, population form); NaN where no file defines it.  Of an aligned report the ``lag_ms_*`` and ``xcorr_*`` columns are summarised too, the
    integer lags and the flag words are not"""
    return report.summarise(rows, report.paired)


def format_summary(summary):
    """the summary as lines of text (what the tool prints)"""
    return report.format_summary(summary, 14, 4)
