"""Projection SDR of (estimate, clean) pairs over filter lengths, as restated in DESIGN.md section 31: the BSS-Eval SDR of one source (Vincent et al.
2006) -- the estimate projected onto the clean signal and its delayed copies 0..m - 1; what the projection explains is target, the rest distortion -- at
several m from one Levinson recursion.  1 tap forgives a scale, 64 taps (4 ms at 16 kHz) colouration, 512 taps (32 ms) is BSS-Eval's default, 2048 taps
(128 ms) forgive everything up to the late tail.  The values are not pinned to ``mir_eval``, which was not at hand.

``evaluate`` scores rows on the GPU through ``csrc/sdr.hip`` and, for a rate above 16 kHz, the project's own resampler.  It has no CPU form: a CPU
tensor raises ``BuddyHipError``.  ``report_rows`` / ``summary_rows`` / ``write_report`` make the CSV report of the tester and of ``tools/sdr.py``, in the
conventions of utils/spectral.py."""
import torch

from .. import _lib
from . import _rows, report
from .metrics import align as _align
from .report import write_report  # noqa: F401  -- the CSV conventions of every report: NaN as an empty field, repr(float)

FS = 16000                                           # the rate the filter lengths are defined at
TAPS = (1, 64, 512, 2048)                            # the default orders: scale, colouration, BSS-Eval's default, up to the late tail
MAX_TAPS, MAX_ORDERS = 2048, 8                       # the limits of buddy_sdr_solve
LOADING = 1e-9                                       # lambda: r[0] (1 + lambda) on the diagonal, the loading buddy_llr uses; sets a ceiling of about 90 dB
DEFINED, CEILING, ILL = 1, 2, 4                      # the bits of ``flags``


def taps_of(values):
    """the orders asked for, ascending and unique, as ints; refuses anything outside 1..2048 and more than eight"""
    vals = list(values)
    if not 1 <= len(vals) <= MAX_ORDERS or any(int(v) != v or not 1 <= v <= MAX_TAPS for v in vals) or len(set(vals)) != len(vals):
        raise ValueError(f"sdr.evaluate: the taps must be 1 to {MAX_ORDERS} different whole numbers in 1..{MAX_TAPS}, got {vals}")
    return tuple(sorted(int(v) for v in vals))


def names_of(taps):
    return tuple(f"sdr{m}" for m in taps)


class SdrEvaluation:
    """result of ``evaluate``, all on the CPU: ``values`` (B, J) float64, dB, in ascending order of ``taps`` (NaN where the row is not defined), ``flags``
    (B,) int32 (bit 0: defined; bit 1: some order sits at the loading's ceiling; bit 2: a pivot of the recursion fell below 2^-26), ``samples`` (B,)
    int32: the samples scored per row at the input's rate, ``taps``: the J orders, ``names``: their columns (``sdr<m>``), ``filters``: (B, max taps)
    float64, the fitted filter of the largest order at 16 kHz (zeros where the row is not defined), or None, ``alignment``: the ``Alignment`` the rows
    were scored after, or None"""

    def __init__(self, values, flags, samples, taps, filters=None, alignment=None):
        self.values, self.flags, self.samples, self.taps, self.names = values, flags, samples, tuple(taps), names_of(taps)
        self.filters, self.alignment = filters, alignment

    @classmethod
    def blank_like(cls, out):
        """the "before" side of a report without input signals: no value, no flag, the samples of ``out``"""
        return cls(torch.full_like(out.values, float("nan")), torch.zeros_like(out.flags), out.samples, out.taps)


def evaluate(est, ref, fs, lens=None, values=TAPS, align=None, loading=LOADING, filters=False):
    """est, ref (B, L) float32 on the GPU at rate ``fs`` (an int >= 16 000): the estimates and the clean signals, row by row; ``lens`` (B ints, default
    L): valid samples per row, the rest is ignored.  ``values``: the filter lengths in taps at 16 kHz (the name is that of the other paired reports'
    argument, so that one caller drives them all).  Above 16 kHz both signals go through the project's resampler first.  ``align`` as in
    ``metrics.evaluate``: the filter is causal, so an estimate that is early is not absorbed unless the pair is aligned first.  ``loading``: lambda.
    ``filters``: also return the fitted filter of the largest order."""
    lib, (est, ref), lens_t = _rows.enter(
        (est, ref), lens, "sdr.evaluate: the measure runs on the MI355X only (got a CPU tensor)", "evaluate takes two (B, L) float32 tensors", fs, FS,
        f"sdr.evaluate: the sample rate must be an integer >= {FS} Hz (the filter lengths are defined at 16 kHz and nothing here upsamples to it), got {fs}")
    taps = taps_of(values)
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
    N, J = taps[-1], len(taps)
    r, d = (torch.empty(B, N, dtype=torch.float64, device=dev) for _ in range(2))
    ee = torch.empty(B, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.buddy_sdr_products_workspace(B, int(lens16.max()), N) // 8, dtype=torch.float64, device=dev)
    _lib.check(lib.buddy_sdr_products(_lib.ptr(e16), _lib.ptr(x16), lens_d.data_ptr(), B, L16, N, r.data_ptr(), d.data_ptr(), ee.data_ptr(), ws.data_ptr(),
                                      ws.numel() * 8, st))
    val, p = (torch.empty(B, J, dtype=torch.float64, device=dev) for _ in range(2))
    fl = torch.empty(B, dtype=torch.int32, device=dev)
    h = torch.empty(B, N, dtype=torch.float64, device=dev) if filters else None
    _lib.check(lib.buddy_sdr_solve(r.data_ptr(), d.data_ptr(), ee.data_ptr(), lens_d.data_ptr(), B, N, (_lib.C.c_int * J)(*taps), J, float(loading),
                                   val.data_ptr(), p.data_ptr(), fl.data_ptr(), _lib.ptr(h), st))
    return SdrEvaluation(val.cpu(), fl.cpu(), lens_t.clone(), taps, h.cpu() if filters else None, alignment)


# ---- the CSV report ------------------------------------------------------------------------------------------------------------------------
def report_rows(names, inp, out):
    """one dict per file from two ``SdrEvaluation``s of the same rows against the clean signals -- ``inp``: the degraded input, ``out``: the
    reconstruction: ``sdr<m>_in``, ``sdr<m>_out`` and ``sdr<m>_delta`` = out - in per order, both flag words and the samples.  Where an evaluation
    carries an ``Alignment`` the row ends with the ``lag_*``, ``lag_ms_*``, ``xcorr_*`` and ``align_flags_*`` columns of ``metrics.report_rows``."""
    rows = []
    for b, name in enumerate(names):
        row = {"file": name, **report.delta_columns(out.names, out.names, inp, out, b)}
        row["flags_in"], row["flags_out"], row["samples"] = int(inp.flags[b]), int(out.flags[b]), int(out.samples[b])
        row.update(report.alignment_columns(inp, out, b))
        rows.append(row)
    return rows


def summary_rows(rows):
    """one dict per value column of ``report_rows``: the number of files where it is defined, and their mean, median and standard deviation
    (numpy's, population form); NaN where no file defines it.  Of an aligned report the ``lag_ms_*`` and ``xcorr_*`` columns are summarised too; the
    integer lags, the samples and the flag words are not"""
    return report.summarise(rows, report.paired)


def format_summary(summary):
    """the summary as lines of text (what the tool prints)"""
    return report.format_summary(summary, 16, 4)
