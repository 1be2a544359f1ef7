#!/usr/bin/env python
"""Score wavs with the project's reference-free measure (buddy_amd/utils/srmr.py): the speech-to-reverberation modulation
energy ratio of every file, on the GPU.  No clean signal is needed.

    python tools/srmr.py <mode dir>                         # its degraded/ and reconstructed/ (and original/, when the mode has one)
    python tools/srmr.py a.wav b.wav ...                    # any wavs: their scores fill the _out columns
    python tools/srmr.py --input DIR --estimate DIR [--out DIR]

Int or float wavs of any integer rate >= 8 kHz, each scored at its own rate (the two wavs of a pair may differ in rate and length); several channels
are averaged to mono, as the real-recordings mode reads them.  Directories are matched by file name.  Writes ``srmr.csv`` and ``srmr_summary.csv``
(the tester's files) into the mode directory or ``--out`` (default: the estimate's directory; a list of wavs writes only with ``--out``) and prints
the summary.  This is the way to score a multi-rank run as a whole, or the output folders of another implementation."""
import argparse
import os
import sys

import numpy as np
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.utils import srmr  # noqa: E402


def read_wav(path):
    """(float32 mono samples, rate): integer formats are scaled by their full scale, several channels averaged"""
    fs, a = wavfile.read(path)
    if a.dtype.kind == "i":
        a = a.astype(np.float64) / float(2 ** (8 * a.dtype.itemsize - 1))
    elif a.dtype.kind == "u":
        a = (a.astype(np.float64) - 128.0) / 128.0
    if a.ndim > 1:
        a = np.mean(a, axis=1)
    if fs < srmr.MIN_FS:
        raise SystemExit(f"srmr: {path} is at {fs} Hz; the score needs at least {srmr.MIN_FS} Hz")
    if len(a) < 1:
        raise SystemExit(f"srmr: {path} is empty")
    return np.ascontiguousarray(a, dtype=np.float32), int(fs)


def wav_names(d):
    return sorted(f for f in os.listdir(d) if f.lower().endswith(".wav"))


def score_dirs(estimate, inp=None, clean=None, device="cuda:0"):
    """the rows of ``srmr.report_rows`` for every wav name present in ``estimate`` (and in ``inp`` and ``clean``, when given)"""
    names = [n for n in wav_names(estimate) if all(d is None or os.path.exists(os.path.join(d, n)) for d in (inp, clean))]
    if not names:
        raise SystemExit(f"srmr: no wav name is common to {', '.join(d for d in (estimate, inp, clean) if d)}")
    cols = [None if d is None else srmr.score_signals([read_wav(os.path.join(d, n)) for n in names], device) for d in (inp, estimate, clean)]
    return srmr.report_rows([n[:-4] for n in names], cols[0], cols[1], cols[2])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("paths", nargs="*", help="a mode directory of a test run, or wav files")
    ap.add_argument("--input", help="directory of the degraded wavs (fills the _in and _delta columns)")
    ap.add_argument("--estimate", help="directory of the wavs to score")
    ap.add_argument("--out", help="directory for srmr.csv and srmr_summary.csv")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.paths and (a.input or a.estimate):
        ap.error("give a mode directory, or wav files, or --estimate [--input]")
    if len(a.paths) == 1 and os.path.isdir(a.paths[0]):
        base = a.paths[0]
        clean = os.path.join(base, "original")
        rows = score_dirs(os.path.join(base, "reconstructed"), os.path.join(base, "degraded"), clean if os.path.isdir(clean) else None, a.device)
        out = a.out or base
    elif a.paths:
        if any(os.path.isdir(p) for p in a.paths):
            ap.error("give ONE mode directory, or wav files")
        rows = srmr.report_rows([os.path.basename(p)[:-4] for p in a.paths], None, srmr.score_signals([read_wav(p) for p in a.paths], a.device))
        out = a.out
        for r in rows:
            print(f"{r['file']}: SRMR {r['srmr_out']:.4f}  K* {r['kstar_out']}  BW {r['bw_out']:.1f} Hz  frames {r['frames_out']}")
    else:
        if not a.estimate:
            ap.error("give a mode directory, wav files, or --estimate")
        rows = score_dirs(a.estimate, a.input, None, a.device)
        out = a.out or a.estimate
    summary = srmr.summary_rows(rows)
    print(srmr.format_summary(summary))
    if out:
        os.makedirs(out, exist_ok=True)
        srmr.write_report(os.path.join(out, "srmr.csv"), rows)
        srmr.write_report(os.path.join(out, "srmr_summary.csv"), summary)
        print(os.path.join(out, "srmr.csv"))
    return rows


if __name__ == "__main__":
    main()
