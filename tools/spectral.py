#!/usr/bin/env python
"""Score a folder of results with the project's spectral distortion measures (buddy_amd/utils/spectral.py): cepstral distance,
log-likelihood ratio and frequency-weighted segmental SNR of every estimate against its clean signal, on the GPU.

    python tools/spectral.py <mode dir>                                    # its original/, degraded/ and reconstructed/
    python tools/spectral.py --reference DIR --estimate DIR [--input DIR] [--out DIR]
    python tools/spectral.py <mode dir> --align [MS]                       # time-align every pair first, within +-MS ms (default 50)

Wavs are matched by file name; int or float wavs of any ONE rate >= 16 kHz per pair (a pair of two rates is refused; a rate above 16 kHz goes through
the project's resampler).  Nothing is time-aligned unless ``--align`` is given; then the pairs are shifted and trimmed exactly as ``tools/evaluate.py
--align`` does, and the lags, their correlations and flags become further columns.  A pair of different lengths is cut to the
shorter, and ``samples`` says so.  Files of equal length and rate are scored as one batch.  Writes ``spectral.csv`` and ``spectral_summary.csv`` (the
tester's files) into the mode directory or ``--out`` (default: the estimate's directory) and prints the summary.  Without ``--input`` the ``_in``
columns are empty.  This is the way to score a multi-rank run as a whole, or the output folders of another implementation."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from buddy_amd.utils import metrics, spectral  # noqa: E402
from evaluate import read_wav, wav_names  # noqa: E402


def score(reference, estimate, inp=None, values=spectral.VALUES, device="cuda:0", align=None):
    """the rows of ``spectral.report_rows`` for every wav name present in ``reference`` and ``estimate`` (and ``inp``, when given); ``align``: the
    search window in ms of ``spectral.evaluate``, None = score the pairs as they are"""
    names = [n for n in wav_names(estimate) if os.path.exists(os.path.join(reference, n)) and (inp is None or os.path.exists(os.path.join(inp, n)))]
    if not names:
        raise SystemExit(f"spectral: no wav name is common to {reference} and {estimate}" + (f" and {inp}" if inp else ""))
    items, groups = [], {}
    for n in names:
        sigs = [read_wav(os.path.join(d, n)) for d in (reference, estimate) + ((inp,) if inp else ())]
        rates = {fs for fs, _ in sigs}
        if len(rates) > 1:
            raise SystemExit(f"spectral: {n} has the rates {sorted(rates)}; the signals of a pair must share one rate")
        fs = rates.pop()
        if fs < spectral.FS:
            raise SystemExit(f"spectral: {n} is at {fs} Hz; the measures need at least {spectral.FS} Hz")
        L = min(len(a) for _, a in sigs)
        if L < 1:
            raise SystemExit(f"spectral: {n} is empty")
        groups.setdefault((fs, L), []).append(len(items))
        items.append([a[:L] for _, a in sigs])
    rows = [None] * len(items)
    for (fs, L), idx in groups.items():
        ref, est = (torch.from_numpy(np.stack([items[i][k] for i in idx])).to(device) for k in (0, 1))
        out = spectral.evaluate(est, ref, fs, values=values, align=align)
        if inp:
            before = spectral.evaluate(torch.from_numpy(np.stack([items[i][2] for i in idx])).to(device), ref, fs, values=values, align=align)
        else:       # no input signals: the _in and _delta columns stay empty
            nan = torch.full_like(out.values, float("nan"))
            zero = torch.zeros_like(out.flags)
            before = spectral.SpectralEvaluation(nan, zero, out.frames, zero, zero, out.samples, out.names)
        for i, row in zip(idx, spectral.report_rows([names[i][:-4] for i in idx], before, out)):
            rows[i] = row
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mode_dir", nargs="?", help="a mode directory of a test run: holds original/, degraded/ and reconstructed/")
    ap.add_argument("--reference", help="directory of the clean wavs")
    ap.add_argument("--estimate", help="directory of the wavs to score")
    ap.add_argument("--input", help="directory of the degraded wavs (fills the _in and _delta columns)")
    ap.add_argument("--out", help="directory for spectral.csv and spectral_summary.csv")
    ap.add_argument("--values", default=",".join(spectral.VALUES), help="comma-separated subset of " + ",".join(spectral.VALUES))
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
    rows = score(ref, est, inp, values=tuple(v for v in a.values.split(",") if v), device=a.device, align=a.align)
    os.makedirs(out, exist_ok=True)
    summary = spectral.summary_rows(rows)
    spectral.write_report(os.path.join(out, "spectral.csv"), rows)
    spectral.write_report(os.path.join(out, "spectral_summary.csv"), summary)
    print(spectral.format_summary(summary))
    print(os.path.join(out, "spectral.csv"))
    return rows


if __name__ == "__main__":
    main()
