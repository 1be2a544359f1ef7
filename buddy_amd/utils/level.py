"""Active speech level, ITU-T P.56 method B as restated in DESIGN.md section 23: how loud the speech of a signal is WHILE someone speaks, so that two
recordings of one talker at one loudness read the same whatever their share of pauses.  It is what ``real_recordings.level: active`` scales a
recording by, and what ``tools/speech_level.py`` measures folders with.  The value is P.56 as restated there; it is not pinned to the ITU software
tool library.

``speech_level`` measures rows on the GPU through ``csrc/level.hip`` (row statistics, the two-pole envelope as one class byte per sample, the hangover
counts).  It has no CPU form: a CPU tensor raises ``BuddyHipError``.  The finish from the sixteen counts of a row -- the dB values, the
interpolation at the margin, the flags -- is float64 host code here (``finish``).  ``active_gain`` is the scaling rule of the real-recordings mode;
``report_rows`` / ``summary_rows`` / ``write_report`` make the CSV report of the tester and of the tool."""
import math

import numpy as np
import torch

from .. import _lib
from . import report
from .report import write_report  # noqa: F401  -- the CSV conventions of every report: NaN as an empty field, repr(float)

THRESHOLDS = 16                                      # c_j = R 2^(j - 15)
MARGIN_DB, TIME_CONSTANT, HANGOVER = 15.9, 0.03, 0.2
BELOW, ABOVE, EDGE, UNDEFINED = 1, 2, 4, 8           # bits of ``flags``
FLAG_NAMES = ((BELOW, "BELOW"), (ABOVE, "ABOVE"), (EDGE, "EDGE"), (UNDEFINED, "UNDEFINED"))


def flag_text(flags):
    """``"EDGE"``, ``"BELOW|UNDEFINED"``, ``""`` for none"""
    return "|".join(name for bit, name in FLAG_NAMES if int(flags) & bit)


def hangover_samples(hangover, fs):
    """I = floor(hangover fs + 0.5)"""
    return int(math.floor(float(hangover) * float(fs) + 0.5))


class SpeechLevel:
    """result of ``speech_level``, all on the CPU: ``level_db`` (B,) float64 = 10 log10 of the mean square while active (NaN where undefined),
    ``activity`` (B,) float64 in (0, 1], ``active_rms`` (B,) float64 = 10^(level_db / 20), ``rms_db`` (B,) float64 of the whole row, ``peak`` (B,)
    float64: the reference amplitude the thresholds hung from, ``counts`` (B, 16) int64: active samples per threshold, ``flags`` (B,) int32 (0: the
    normal case), ``samples`` (B,) int32"""

    def __init__(self, level_db, activity, active_rms, rms_db, peak, counts, flags, samples):
        self.level_db, self.activity, self.active_rms, self.rms_db = level_db, activity, active_rms, rms_db
        self.peak, self.counts, self.flags, self.samples = peak, counts, flags, samples


def finish(counts, sq, n, ref, margin_db=MARGIN_DB):
    """(level_db, activity, rms_db, flags) of one row from its counts a_j (16 ints), sq = sum (x - o)^2, its n samples and the reference amplitude;
    float64 throughout.  Flags: BELOW -- already the lowest threshold is within the margin; ABOVE -- none is; EDGE -- the first threshold within
    the margin has no active sample, so there is nothing to interpolate to; UNDEFINED -- no sample, no energy, or a sample that is not finite."""
    nan = float("nan")
    n, sq, ref = int(n), float(sq), float(ref)
    if n < 1 or not math.isfinite(sq) or not sq > 0.0 or not math.isfinite(ref) or not ref > 0.0:
        return nan, nan, nan, UNDEFINED
    rms_db = 10.0 * math.log10(sq / n)
    a = [int(v) for v in counts]
    A = [10.0 * math.log10(sq / v) if v > 0 else nan for v in a]
    D = [A[j] - 20.0 * math.log10(ref * 2.0 ** (j - 15)) if a[j] > 0 else -math.inf for j in range(THRESHOLDS)]
    js = next((j for j in range(THRESHOLDS) if D[j] <= margin_db), None)
    flags = 0
    if js is None:
        level, flags = A[THRESHOLDS - 1], ABOVE
    elif js == 0:
        if a[0] == 0:
            return nan, nan, rms_db, BELOW | UNDEFINED
        level, flags = A[0], BELOW
    elif a[js] == 0:
        level, flags = A[js - 1], EDGE
    else:
        t = (D[js - 1] - margin_db) / (D[js - 1] - D[js])
        level = A[js - 1] + t * (A[js] - A[js - 1])
    return level, 10.0 ** ((rms_db - level) / 10.0), rms_db, flags


def check_arguments(fs, full_scale, margin_db, time_constant, hangover, rows):
    """the checks of ``speech_level`` that need no GPU -> (fs, None or the (rows,) float64 reference amplitudes, I)"""
    fs = float(fs)
    if not math.isfinite(fs) or not fs > 0.0:
        raise ValueError(f"speech_level: the sample rate must be finite and > 0, got {fs}")
    if not math.isfinite(float(margin_db)):
        raise ValueError(f"speech_level: margin_db must be finite, got {margin_db}")
    if not math.isfinite(float(time_constant)) or not float(time_constant) > 0.0:
        raise ValueError(f"speech_level: time_constant must be finite and > 0, got {time_constant}")
    if not math.isfinite(float(hangover)) or float(hangover) < 0.0 or float(hangover) * fs >= 2.0 ** 31 - 1:
        raise ValueError(f"speech_level: hangover must be finite, >= 0 and below 2^31 samples, got {hangover}")
    if isinstance(full_scale, str):
        if full_scale != "peak":
            raise ValueError(f"speech_level: full_scale is 'peak', a number or one number per row, got {full_scale!r}")
        ref = None
    else:
        ref = np.asarray(full_scale.detach().cpu() if isinstance(full_scale, torch.Tensor) else full_scale, dtype=np.float64).reshape(-1)
        if ref.size == 1:
            ref = np.repeat(ref, rows)
        if ref.size != rows:
            raise ValueError(f"speech_level: full_scale has {ref.size} values for {rows} rows")
        if not np.all(np.isfinite(ref)) or not np.all(ref > 0.0):
            raise ValueError("speech_level: every full_scale must be finite and > 0")
    return fs, ref, hangover_samples(hangover, fs)


def _workspace(query, B, longest, dev):
    nbytes = int(query(B, longest))
    assert nbytes >= 0
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev), nbytes


def speech_level(x, fs, lengths=None, full_scale="peak", remove_mean=True, margin_db=MARGIN_DB, time_constant=TIME_CONSTANT, hangover=HANGOVER):
    """x (B, L) or (L,) float32 on the GPU at rate ``fs``; ``lengths`` (B ints in 0..L, default L): valid samples per row, the rest is ignored.
    ``full_scale``: the amplitude R the sixteen thresholds R 2^(j - 15) hang from -- ``"peak"``: the row's own max |x| (with ``remove_mean``:
    max |x| + |mean|, an upper bound of max |x - mean|), which makes the level follow a gain, as float wavs of arbitrary scale need; a number or one
    per row: a fixed grid (1.0 is the ITU's for full-scale-1 signals).  ``remove_mean``: the row mean is the offset o, else 0."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.BuddyHipError("speech_level: the meter runs on the MI355X only (got a CPU tensor)")
    lib = _lib.require_gpu()
    if x.dim() == 1:
        x = x[None]
    assert x.dim() == 2 and x.dtype == torch.float32, "speech_level takes a (B, L) float32 tensor"
    x = x.contiguous()
    B, L = x.shape
    fs, ref, hang = check_arguments(fs, full_scale, margin_db, time_constant, hangover, B)
    dev = x.device
    lens_t = torch.full((B,), L, dtype=torch.int32) if lengths is None else torch.as_tensor(lengths, dtype=torch.int32).reshape(B).cpu()
    if L < 1 or int(lens_t.min()) < 0 or int(lens_t.max()) > L:
        raise ValueError("speech_level: every length must be in 0..L, L >= 1")
    n = lens_t.numpy().astype(np.int64)
    longest = int(n.max())
    lens_d = lens_t.to(dev)
    st = _lib.stream_ptr()
    stats = torch.empty(B, 2, dtype=torch.float64, device=dev)
    ws, nbytes = _workspace(lib.buddy_level_stats_workspace, B, longest, dev)
    _lib.check(lib.buddy_level_stats(_lib.ptr(x), L, lens_d.data_ptr(), B, stats.data_ptr(), ws.data_ptr(), nbytes, st))
    stats = stats.cpu().numpy()
    mean = np.where(n > 0, stats[:, 0] / np.maximum(n, 1), 0.0) if remove_mean else np.zeros(B)
    peak = stats[:, 1] + np.abs(mean)
    if ref is None:
        ref = peak
    ref = np.array(ref, dtype=np.float64)
    dead = ~(np.isfinite(mean) & np.isfinite(ref) & (ref > 0.0))          # an empty, all-zero or non-finite row: measured on a stand-in grid, reported undefined
    off_d = torch.from_numpy(np.where(dead, 0.0, mean)).to(dev)
    ref_d = torch.from_numpy(np.where(dead, 1.0, ref)).to(dev)
    klass = torch.empty(B, L, dtype=torch.uint8, device=dev)
    sq = torch.empty(B, dtype=torch.float64, device=dev)
    ws, nbytes = _workspace(lib.buddy_level_classes_workspace, B, longest, dev)
    _lib.check(lib.buddy_level_classes(_lib.ptr(x), L, lens_d.data_ptr(), off_d.data_ptr(), ref_d.data_ptr(), B, fs, float(time_constant), klass.data_ptr(), L,
                                       sq.data_ptr(), ws.data_ptr(), nbytes, st))
    counts = torch.empty(B, THRESHOLDS, dtype=torch.int64, device=dev)
    ws, nbytes = _workspace(lib.buddy_level_counts_workspace, B, longest, dev)
    _lib.check(lib.buddy_level_counts(klass.data_ptr(), L, lens_d.data_ptr(), B, hang, counts.data_ptr(), ws.data_ptr(), nbytes, st))
    counts, sq = counts.cpu(), sq.cpu().numpy()
    rows = [finish(counts[b].tolist(), sq[b], n[b], float("nan") if dead[b] else ref[b], float(margin_db)) for b in range(B)]
    level = torch.tensor([r[0] for r in rows], dtype=torch.float64)
    return SpeechLevel(level, torch.tensor([r[1] for r in rows], dtype=torch.float64), 10.0 ** (level / 20.0),
                       torch.tensor([r[2] for r in rows], dtype=torch.float64), torch.from_numpy(ref.copy()), counts,
                       torch.tensor([r[3] for r in rows], dtype=torch.int32), lens_t.clone())


# ---- the scaling rule of the real-recordings mode ---------------------------------------------------------------------------------------------
def level_options(rr):
    """(level, reference_activity) of a ``real_recordings`` block; a config written before the keys existed means ("std", None).  ``active`` without
    a reference activity stops here, before anything is sampled."""
    level = str(rr.get("level", "std"))
    if level not in ("std", "active"):
        raise ValueError(f"real_recordings.level is 'std' or 'active', got {level!r}")
    ra = rr.get("reference_activity", None)
    if level == "std":
        return level, None
    if ra is None:
        raise ValueError("real_recordings.level=active needs real_recordings.reference_activity: the activity factor (share of time speech is active, "
                         "ITU-T P.56) typical of the segments the network was trained on, in (0, 1].  A file of that activity is scaled exactly as "
                         "level=std scales it.  Measure it: run tools/speech_level.py --segment-seconds <training segment length> on the training "
                         "wavs and take the median activity it prints.  No default is shipped.")
    ra = float(ra)
    if not (0.0 < ra <= 1.0):
        raise ValueError(f"real_recordings.reference_activity must be in (0, 1], got {ra}")
    return level, ra


def active_gain(gain, scaling_factor, active_rms, reference_activity):
    """g = gain scaling_factor / (active_rms sqrt(reference_activity)): a row whose activity equals the reference has active_rms sqrt(activity) = its
    rms, the scale ``gain scaling_factor / std`` gives it"""
    return float(gain) * float(scaling_factor) / (float(active_rms) * math.sqrt(float(reference_activity)))


# ---- the CSV reports -------------------------------------------------------------------------------------------------------------------------
def report_rows(names, res, extra=None):
    """one dict per row of a ``SpeechLevel``; ``extra``: per row a dict of further columns (the tester's rule and g)"""
    rows = []
    for b, name in enumerate(names):
        row = {"file": name, "samples": int(res.samples[b]), "level_db": float(res.level_db[b]), "activity": float(res.activity[b]),
               "rms_db": float(res.rms_db[b]), "peak": float(res.peak[b]), "flags": flag_text(res.flags[b])}
        if extra is not None:
            row.update(extra[b])
        rows.append(row)
    return rows


def summary_rows(rows):
    """n, mean, median and standard deviation (numpy's, population form) of ``level_db``, ``activity`` and ``rms_db - level_db`` over the rows where
    the level is defined; NaN where there is none"""
    return report.summarise(rows, {"level_db": lambda r: r["level_db"], "activity": lambda r: r["activity"],
                                   "rms_db-level_db": lambda r: r["rms_db"] - r["level_db"]})


def format_summary(summary):
    """the summary as lines of text (what the tool prints)"""
    return report.format_summary(summary, 16, 5)
