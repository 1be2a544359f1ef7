"""Spectral-envelope distortion of (estimate, clean) pairs, as restated in DESIGN.md section 21: cepstral distance (CD, dB), log-likelihood ratio (LLR)
and frequency-weighted segmental SNR (fwSegSNR, dB) -- with SRMR (utils/srmr.py) the four objective measures the dereverberation literature reports.

``evaluate`` scores rows on the GPU through ``csrc/spectral.hip`` and, for a rate above 16 kHz, the project's own resampler.  It has no CPU form: a
CPU tensor raises ``BuddyHipError``.  The mel bands are designed here in float64 and cached.  ``report_rows`` / ``summary_rows`` / ``write_report`` make
the CSV report of the tester and of ``tools/spectral.py``, in the conventions of utils/metrics.py."""
import functools
import math

import numpy as np
import torch

from .. import _lib
from . import _rows, report
from .metrics import align as _align
from .report import write_report  # noqa: F401  -- the CSV conventions of every report: NaN as an empty field, repr(float)

VALUES = ("cd", "llr", "fwsegsnr")                   # order of the last axis of ``SpectralEvaluation.values``; flag bit q = value q is defined
FS = 16000                                           # the rate the three measures are defined at
FRAME, HOP, NFFT, BINS = 400, 160, 512, 257
LPC_ORDER = 12
MEL_BANDS = 23
FLOOR = 1e-8                                         # the log floor of the cepstra relative to the per-bin power of a white signal of the clean row's variance


@functools.lru_cache(maxsize=None)
def mel_bands(fs=FS, nfft=NFFT, num_bands=MEL_BANDS):
    """(num_bands, nfft / 2 + 1) float64, read-only: band j is the triangle of height 1 between points j, j + 1 and j + 2 of num_bands + 2 points
    equally spaced in mel(f) = 2595 log10(1 + f / 700) from 0 to fs / 2, sampled at the bin frequencies k fs / nfft.  Designed in float64, cached."""
    top = 2595.0 * math.log10(1.0 + 0.5 * float(fs) / 700.0)
    pts = 700.0 * (10.0 ** (np.arange(num_bands + 2, dtype=np.float64) * (top / (num_bands + 1)) / 2595.0) - 1.0)
    f = np.arange(nfft // 2 + 1, dtype=np.float64) * (float(fs) / nfft)
    lo, c, hi = pts[:-2, None], pts[1:-1, None], pts[2:, None]
    M = np.maximum(0.0, np.minimum((f[None, :] - lo) / (c - lo), (hi - f[None, :]) / (hi - c)))
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def _window_energy():
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(FRAME, dtype=np.float64) + 1.0) / (FRAME + 1.0))
    return float(np.sum(w * w))


def frames_of(n):
    """full frames of 400 samples at hop 160"""
    return (int(n) - FRAME) // HOP + 1 if int(n) >= FRAME else 0


_device_bands = {}


def _bands_on(device):
    key = str(device)
    if key not in _device_bands:
        _device_bands[key] = torch.from_numpy(mel_bands().copy()).to(device)     # the cached table is read-only
    return _device_bands[key]


class SpectralEvaluation:
    """result of ``evaluate``, all on the CPU: ``values`` (B, 3) float64 in the order ``VALUES`` (dB, natural log, dB; NaN where undefined or not asked
    for), ``flags`` (B,) int32 (bit q: value q is defined), ``frames`` (B,) int32: full frames at 16 kHz, ``llr_frames`` / ``fwsegsnr_frames`` (B,) int32:
    the frames those means were taken over, ``samples`` (B,) int32: the samples scored per row at the input's rate, ``names``: the values asked for,
    ``alignment``: the ``Alignment`` the rows were scored after, or None"""

    def __init__(self, values, flags, frames, llr_frames, fwsegsnr_frames, samples, names, alignment=None):
        self.values, self.flags, self.frames, self.llr_frames, self.fwsegsnr_frames = values, flags, frames, llr_frames, fwsegsnr_frames
        self.samples, self.names, self.alignment = samples, names, alignment

    @classmethod
    def blank_like(cls, out):
        """the "before" side of a report without input signals: no value, no flag, no counted frame, the frames and the samples of ``out``"""
        zero = torch.zeros_like(out.flags)
        return cls(torch.full_like(out.values, float("nan")), zero, out.frames, zero, zero, out.samples, out.names)


def evaluate(est, ref, fs, lens=None, values=VALUES, align=None):
    """est, ref (B, L) float32 on the GPU at rate ``fs`` (an int >= 16 000): the estimates and the clean signals, row by row; ``lens`` (B ints, default
    L): valid samples per row, the rest is ignored.  Above 16 kHz both signals go through the project's resampler first.  ``align`` as in
    ``metrics.evaluate``: None scores the pairs as they are, a search window in ms shifts every pair by its own integer lag and trims it to the
    overlap first (at the input's rate); the result carries the ``Alignment`` and ``samples`` is the overlap."""
    lib, (est, ref), lens_t = _rows.enter(
        (est, ref), lens, "spectral.evaluate: the measures run on the MI355X only (got a CPU tensor)", "evaluate takes two (B, L) float32 tensors", fs, FS,
        f"spectral.evaluate: the sample rate must be an integer >= {FS} Hz (the measures are defined at 16 kHz and nothing here upsamples to it), got {fs}")
    unknown = sorted(set(values) - set(VALUES))
    if unknown:
        raise ValueError(f"spectral.evaluate: unknown values {unknown}; known: {list(VALUES)}")
    names = tuple(v for v in VALUES if v in tuple(values))
    fs = int(fs)
    B, L = est.shape
    dev = est.device
    alignment = None
    if align is not None:
        alignment = _align(est, ref, fs, lens=lens_t, max_lag_ms=float(align))
        est, ref, lens_t = alignment.est, alignment.ref, _rows.lengths(alignment.lens, B, L)
    (e16, x16), lens16 = _rows.to_rate((est, ref), lens_t, fs, FS)
    L16 = x16.shape[1]
    lens_d = lens16.to(dev)
    st = _lib.stream_ptr()
    out = torch.full((B, 3), float("nan"), dtype=torch.float64)
    flags = torch.zeros(B, dtype=torch.int32)
    frames = torch.tensor([frames_of(int(n)) for n in lens16], dtype=torch.int32)
    counts = {m: torch.zeros(B, dtype=torch.int32) for m in ("llr", "fwsegsnr")}
    maxF = int(frames.max())
    ldf = max(maxF, 1)
    val = torch.empty(B, dtype=torch.float64, device=dev)
    cnt, fl = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)

    if "cd" in names or "fwsegsnr" in names:
        mom = torch.empty(B, 4, dtype=torch.float64, device=dev)
        mom_fl = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(lib.buddy_pair_moments(_lib.ptr(e16), _lib.ptr(x16), lens_d.data_ptr(), B, L16, mom.data_ptr(), mom_fl.data_ptr(), st))
        gain = _rows.pair_gain(mom)
        delta = (FLOOR * (mom[:, 1] / lens_d.double()) * _window_energy()).contiguous()
        frames_d = frames.to(dev)
        X, E = (torch.empty(B, ldf, BINS, dtype=torch.float32, device=dev) for _ in range(2))
        for sig, S in ((x16, X), (e16, E)):
            _lib.check(lib.buddy_frame_spectra(_lib.ptr(sig), lens_d.data_ptr(), B, L16, FRAME, HOP, _lib.ptr(S), ldf, st))
        if "cd" in names:
            ws = torch.empty(lib.buddy_cepstral_distance_workspace(B, maxF) // 8, dtype=torch.float64, device=dev)
            _lib.check(lib.buddy_cepstral_distance(_lib.ptr(X), _lib.ptr(E), frames_d.data_ptr(), B, ldf, gain.data_ptr(), delta.data_ptr(), val.data_ptr(),
                                                   fl.data_ptr(), ws.data_ptr(), ws.numel() * 8, st))
            out[:, 0] = val.cpu()
            flags |= fl.cpu()
        if "fwsegsnr" in names:
            M = _bands_on(dev)
            ws = torch.empty(lib.buddy_fwsegsnr_workspace(B, maxF) // 8, dtype=torch.float64, device=dev)
            _lib.check(lib.buddy_fwsegsnr(_lib.ptr(X), _lib.ptr(E), frames_d.data_ptr(), B, ldf, gain.data_ptr(), M.data_ptr(), M.shape[0], val.data_ptr(),
                                          cnt.data_ptr(), fl.data_ptr(), ws.data_ptr(), ws.numel() * 8, st))
            out[:, 2] = val.cpu()
            flags |= fl.cpu() << 2
            counts["fwsegsnr"] = cnt.cpu()

    if "llr" in names:
        ws = torch.empty(lib.buddy_llr_workspace(B, int(lens16.max()), FRAME, HOP) // 8, dtype=torch.float64, device=dev)
        _lib.check(lib.buddy_llr(_lib.ptr(e16), _lib.ptr(x16), lens_d.data_ptr(), B, L16, FRAME, HOP, LPC_ORDER, val.data_ptr(), cnt.data_ptr(), fl.data_ptr(),
                                 ws.data_ptr(), ws.numel() * 8, st))
        out[:, 1] = val.cpu()
        flags |= fl.cpu() << 1
        counts["llr"] = cnt.cpu()
    return SpectralEvaluation(out, flags, frames, counts["llr"], counts["fwsegsnr"], lens_t.clone(), names, alignment)


# ---- the CSV report ------------------------------------------------------------------------------------------------------------------------
def report_rows(names, inp, out):
    """one dict per file from two ``SpectralEvaluation``s of the same rows against the clean signals -- ``inp``: the degraded input, ``out``: the
    reconstruction: ``<m>_in``, ``<m>_out`` and ``<m>_delta`` = out - in per value asked for, both flag words, the frames at 16 kHz and the frames the
    LLR and fwSegSNR means were taken over, per side.  Where an evaluation carries an ``Alignment`` the row ends with the ``lag_*``, ``lag_ms_*``,
    ``xcorr_*`` and ``align_flags_*`` columns of ``metrics.report_rows``."""
    rows = []
    for b, name in enumerate(names):
        row = {"file": name, "samples": int(out.samples[b]), **report.delta_columns(VALUES, out.names, inp, out, b)}
        row["flags_in"], row["flags_out"] = int(inp.flags[b]), int(out.flags[b])
        row["frames"] = int(out.frames[b])
        row["llr_frames_in"], row["llr_frames_out"] = int(inp.llr_frames[b]), int(out.llr_frames[b])
        row["fwsegsnr_frames_in"], row["fwsegsnr_frames_out"] = int(inp.fwsegsnr_frames[b]), int(out.fwsegsnr_frames[b])
        row.update(report.alignment_columns(inp, out, b))
        rows.append(row)
    return rows


def summary_rows(rows):
    """one dict per value column of ``report_rows``: the number of files where it is defined, and their mean, median and standard deviation
    (numpy's, population form); NaN where no file defines it.  Of an aligned report the ``lag_ms_*`` and ``xcorr_*`` columns are summarised too; the
    integer lags, the frame counts and the flag words are not"""
    return report.summarise(rows, lambda col: report.paired(col) and not col.startswith(("llr_frames", "fwsegsnr_frames")))


def format_summary(summary):
    """the summary as lines of text (what the tool prints)"""
    return report.format_summary(summary, 16, 4)
