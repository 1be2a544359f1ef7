#!/usr/bin/env python
"""Score a folder of results with the project's evaluation metrics (buddy_amd/utils/metrics.py): SI-SDR, STOI, ESTOI and LSD of
every estimate against its clean signal, on the GPU.

    python tools/evaluate.py <mode dir>                                    # its original/, degraded/ and reconstructed/
    python tools/evaluate.py --reference DIR --estimate DIR [--input DIR] [--out DIR]
    python tools/evaluate.py <mode dir> --align [MS]                       # time-align every pair first, within +-MS ms (default 50)

Wavs are matched by file name; int or float wavs of any ONE rate >= 10 kHz per pair (a pair of two rates is refused, nothing is resampled to match).  Nothing is time-aligned unless ``--align`` is given: then every estimate (and every input) is shifted by its own integer
lag against its clean signal -- the largest |cross-correlation| within the window -- and the pair is trimmed to the overlap before it is scored; the
lags, their correlations and flags become further columns.  The 50 ms default, about 17 m of path difference, is a choice nobody
has measured.  A pair of different lengths is cut to the shorter, and ``samples`` says so.  Files of equal length and rate are scored as
one batch.  Writes ``metrics.csv`` and ``metrics_summary.csv`` (the tester's files) into the mode directory or ``--out`` (default: the estimate's
directory) and prints the summary.  Without ``--input`` the ``_in`` columns are empty.  This is the way to score a multi-rank run as a whole, or the
output folders of another implementation."""
import argparse
import collections
import os
import sys

import numpy as np
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.utils import metrics  # noqa: E402


def read_wav(path):
    """(rate, float32 mono samples): integer formats are scaled by their full scale; of several channels the first is taken"""
    fs, a = wavfile.read(path)
    if a.ndim > 1:
        a = a[:, 0]
    if a.dtype.kind == "i":
        a = a.astype(np.float64) / float(2 ** (8 * a.dtype.itemsize - 1))
    elif a.dtype.kind == "u":
        a = (a.astype(np.float64) - 128.0) / 128.0
    return int(fs), np.ascontiguousarray(a, dtype=np.float32)


def wav_names(d):
    return sorted(f for f in os.listdir(d) if f.lower().endswith(".wav"))


# what tells this tool from tools/spectral.py: the module that scores, the lowest rate it takes, the prefix of the messages and what they call the
# values, and the stem of the two files
Kind = collections.namedtuple("Kind", "module min_fs who noun stem")
METRICS = Kind(metrics, metrics.STOI_FS, "evaluate", "metrics", "metrics")


def score_pairs(kind, reference, estimate, inp, values, device, align):
    """the rows of ``kind.module.report_rows`` for every wav name present in ``reference`` and ``estimate`` (and ``inp``, when given); ``align``: the
    search window in ms of its ``evaluate``, None = score the pairs as they are"""
    module, who = kind.module, kind.who
    names = [n for n in wav_names(estimate) if os.path.exists(os.path.join(reference, n)) and (inp is None or os.path.exists(os.path.join(inp, n)))]
    if not names:
        raise SystemExit(f"{who}: no wav name is common to {reference} and {estimate}" + (f" and {inp}" if inp else ""))
    items, groups = [], {}
    for n in names:
        sigs = [read_wav(os.path.join(d, n)) for d in (reference, estimate) + ((inp,) if inp else ())]
        rates = {fs for fs, _ in sigs}
        if len(rates) > 1:
            raise SystemExit(f"{who}: {n} has the rates {sorted(rates)}; the signals of a pair must share one rate")
        fs = rates.pop()
        if fs < kind.min_fs:
            raise SystemExit(f"{who}: {n} is at {fs} Hz; the {kind.noun} need at least {kind.min_fs} Hz")
        L = min(len(a) for _, a in sigs)
        if L < 1:
            raise SystemExit(f"{who}: {n} is empty")
        groups.setdefault((fs, L), []).append(len(items))
        items.append([a[:L] for _, a in sigs])
    rows = [None] * len(items)
    for (fs, L), idx in groups.items():
        ref, est = (torch.from_numpy(np.stack([items[i][k] for i in idx])).to(device) for k in (0, 1))
        out = module.evaluate(est, ref, fs, values=values, align=align)
        if inp:
            before = module.evaluate(torch.from_numpy(np.stack([items[i][2] for i in idx])).to(device), ref, fs, values=values, align=align)
        else:       # no input signals: the _in and _delta columns stay empty
            before = type(out).blank_like(out)
        for i, row in zip(idx, module.report_rows([names[i][:-4] for i in idx], before, out)):
            rows[i] = row
    return rows


def score(reference, estimate, inp=None, values=metrics.VALUES, device="cuda:0", align=None):
    """``score_pairs`` with ``metrics.evaluate``"""
    return score_pairs(METRICS, reference, estimate, inp, values, device, align)


def run(kind, doc, argv=None):
    """the command line of this tool and of tools/spectral.py; ``doc``: the tool's own module docstring"""
    module, stem = kind.module, kind.stem
    ap = argparse.ArgumentParser(description=doc.split("\n\n")[0])
    ap.add_argument("mode_dir", nargs="?", help="a mode directory of a test run: holds original/, degraded/ and reconstructed/")
    ap.add_argument("--reference", help="directory of the clean wavs")
    ap.add_argument("--estimate", help="directory of the wavs to score")
    ap.add_argument("--input", help="directory of the degraded wavs (fills the _in and _delta columns)")
    ap.add_argument("--out", help=f"directory for {stem}.csv and {stem}_summary.csv")
    ap.add_argument("--values", default=",".join(module.VALUES), help="comma-separated subset of " + ",".join(module.VALUES))
    ap.add_argument("--align", nargs="?", type=float, const=metrics.MAX_LAG_MS, default=None, metavar="MS",
                    help="time-align every pair before it is scored: integer lag within +-MS ms (default %(const)s), pair trimmed to the overlap")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.mode_dir:
        if a.reference or a.estimate or a.input:
            ap.error("give either a mode directory or --reference/--estimate")
        ref, est, inp = (os.path.join(a.mode_dir, s) for s in ("original", "reconstructed", "degraded"))
        out = a.out or a.mode_dir
    else:
        if not (a.reference and a.estimate):
            ap.error("give a mode directory, or both --reference and --estimate")
        ref, est, inp, out = a.reference, a.estimate, a.input, a.out or a.estimate
    rows = score_pairs(kind, ref, est, inp, tuple(v for v in a.values.split(",") if v), a.device, a.align)
    os.makedirs(out, exist_ok=True)
    summary = module.summary_rows(rows)
    module.write_report(os.path.join(out, f"{stem}.csv"), rows)
    module.write_report(os.path.join(out, f"{stem}_summary.csv"), summary)
    print(module.format_summary(summary))
    print(os.path.join(out, f"{stem}.csv"))
    return rows


def main(argv=None):
    return run(METRICS, __doc__, argv)


if __name__ == "__main__":
    main()
