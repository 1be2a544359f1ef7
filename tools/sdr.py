#!/usr/bin/env python
"""Score a folder of results with the project's projection SDR (buddy_amd/utils/sdr.py): the BSS-Eval SDR of every estimate against
its clean signal -- the estimate projected onto the clean signal and its delayed copies -- at several filter lengths from one recursion, on the GPU.

    python tools/sdr.py <mode dir>                                         # its original/, degraded/ and reconstructed/
    python tools/sdr.py --reference DIR --estimate DIR [--input DIR] [--out DIR]
    python tools/sdr.py <mode dir> --align [MS]                            # time-align every pair first, within +-MS ms (default 50)
    python tools/sdr.py <mode dir> --taps 1 16 64 256 512 2048 --write-filters DIR

Wavs are matched by file name; int or float wavs of any ONE rate >= 16 kHz per pair (a pair of two rates is refused; a rate above 16 kHz goes through
the project's resampler: the taps are counted at 16 kHz).  The filter is causal: an estimate that is EARLY is not absorbed unless ``--align`` is given;
then the pairs are shifted and trimmed exactly as ``tools/evaluate.py --align`` does, and the lags, their correlations and flags become further columns
(DESIGN.md section 19).  A pair of different lengths is cut to the shorter, and ``samples`` says so.  Files of equal length and rate are scored as one
batch.  ``--taps``: up to 8 filter lengths within 1..2048 (default 1 64 512 2048; 512 is BSS-Eval's).  ``--loading``: the relative diagonal loading
(default 1e-9, a ceiling of about 90 dB).  ``--write-filters DIR``: each estimate's fitted filter of the largest length -- the residual room response
from the clean signal to the estimate -- as a float32 wav at 16 kHz, which ``tools/rir_report.py`` can analyse.  Writes ``sdr.csv`` and
``sdr_summary.csv`` (the tester's files) into the mode directory or ``--out`` (default: the estimate's directory) and prints the summary.  Without
``--input`` the ``_in`` columns are empty.  The values are not pinned to ``mir_eval``, which was not at hand when this was written."""
import argparse
import os
import sys

import numpy as np
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from buddy_amd.utils import metrics, sdr  # noqa: E402
from evaluate import Kind, score_pairs  # noqa: E402  -- the scoring loop is tools/evaluate.py's


class _Scorer:
    """utils/sdr.py as ``score_pairs`` drives a module: the loading bound, and the fitted filters of the estimates kept by file name"""

    def __init__(self, loading, filters):
        self.loading, self.filters, self.fitted = loading, filters, {}

    def evaluate(self, est, ref, fs, values, align):
        return sdr.evaluate(est, ref, fs, values=values, align=align, loading=self.loading, filters=self.filters)

    def report_rows(self, names, inp, out):
        if self.filters:
            self.fitted.update({n: out.filters[b].numpy() for b, n in enumerate(names)})
        return sdr.report_rows(names, inp, out)


def score(reference, estimate, inp=None, taps=sdr.TAPS, device="cuda:0", align=None, loading=sdr.LOADING, filters=False):
    """``score_pairs`` with ``sdr.evaluate``; with ``filters`` -> (rows, {file name without .wav: the estimate's filter of the largest order, float64})"""
    scorer = _Scorer(loading, filters)
    rows = score_pairs(Kind(scorer, sdr.FS, "sdr", "filter lengths", "sdr"), reference, estimate, inp, taps, device, align)
    return (rows, scorer.fitted) if filters else rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("mode_dir", nargs="?", help="a mode directory of a test run: holds original/, degraded/ and reconstructed/")
    ap.add_argument("--reference", help="directory of the clean wavs")
    ap.add_argument("--estimate", help="directory of the wavs to score")
    ap.add_argument("--input", help="directory of the degraded wavs (fills the _in and _delta columns)")
    ap.add_argument("--out", help="directory for sdr.csv and sdr_summary.csv")
    ap.add_argument("--taps", nargs="+", type=int, default=list(sdr.TAPS), metavar="M",
                    help=f"filter lengths in taps at 16 kHz: at most {sdr.MAX_ORDERS} different ones within 1..{sdr.MAX_TAPS} (default %(default)s)")
    ap.add_argument("--loading", type=float, default=sdr.LOADING, help="relative diagonal loading of the Toeplitz system (default %(default)s)")
    ap.add_argument("--align", nargs="?", type=float, const=metrics.MAX_LAG_MS, default=None, metavar="MS",
                    help="time-align every pair before it is scored: integer lag within +-MS ms (default %(const)s), pair trimmed to the overlap")
    ap.add_argument("--write-filters", metavar="DIR", help="write every estimate's fitted filter of the largest length there, float32 wavs at 16 kHz")
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
    try:
        taps = sdr.taps_of(a.taps)
    except ValueError as e:
        ap.error(str(e))
    if not (a.loading >= 0.0 and np.isfinite(a.loading)):
        ap.error(f"--loading must be finite and >= 0, got {a.loading}")
    rows = score(ref, est, inp, taps, a.device, a.align, a.loading, bool(a.write_filters))
    if a.write_filters:
        rows, fitted = rows
        os.makedirs(a.write_filters, exist_ok=True)
        for n, h in fitted.items():
            wavfile.write(os.path.join(a.write_filters, n + ".wav"), sdr.FS, h.astype(np.float32))
    os.makedirs(out, exist_ok=True)
    summary = sdr.summary_rows(rows)
    sdr.write_report(os.path.join(out, "sdr.csv"), rows)
    sdr.write_report(os.path.join(out, "sdr_summary.csv"), summary)
    print(sdr.format_summary(summary))
    print(os.path.join(out, "sdr.csv"))
    return rows


if __name__ == "__main__":
    main()
