#!/usr/bin/env python
"""Score wavs with the project's blind decay time (buddy_amd/utils/decay.py): how long each file's own free decays would take
to fall by 60 dB, broadband and per octave band, on the GPU.  Neither a clean signal nor an impulse response is needed.

    python tools/decay.py <mode dir>                         # its degraded/ and reconstructed/ (and original/, when the mode has one)
    python tools/decay.py a.wav b.wav ...                    # any wavs: their values fill the _out columns
    python tools/decay.py --input DIR --estimate DIR [--out DIR]

Int or float wavs of any integer rate >= 8 kHz, each scored at its own rate (the two wavs of a pair may differ in rate and length); every channel of
a file with several is a row of its own (``<file>.ch<k>``).  Directories are matched by file name.  Writes ``decay.csv`` and ``decay_summary.csv``
(the tester's files) into the mode directory or ``--out`` (default: the estimate's directory; a list of wavs writes only with ``--out``) and prints
the summary.  This is the way to score a multi-rank run as a whole, or the output folders of another implementation."""
import argparse
import os
import sys

import numpy as np
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.utils import decay  # noqa: E402


def read_wav(path):
    """[(row name, float32 samples, rate)] per channel: integer formats are scaled by their full scale"""
    fs, a = wavfile.read(path)
    if a.dtype.kind == "i":
        a = a.astype(np.float64) / float(2 ** (8 * a.dtype.itemsize - 1))
    elif a.dtype.kind == "u":
        a = (a.astype(np.float64) - 128.0) / 128.0
    if fs < decay.MIN_FS:
        raise SystemExit(f"decay: {path} is at {fs} Hz; the measure needs at least {decay.MIN_FS} Hz")
    if len(a) < 1:
        raise SystemExit(f"decay: {path} is empty")
    name = os.path.basename(path)[:-4]
    if a.ndim == 1:
        return [(name, np.ascontiguousarray(a, dtype=np.float32), int(fs))]
    return [(f"{name}.ch{c}", np.ascontiguousarray(a[:, c], dtype=np.float32), int(fs)) for c in range(a.shape[1])]


def wav_names(d):
    return sorted(f for f in os.listdir(d) if f.lower().endswith(".wav"))


def score_files(paths, device):
    """(row names, ``score_signals`` rows) of every channel of every file"""
    chans = [c for p in paths for c in read_wav(p)]
    return [c[0] for c in chans], decay.score_signals([(c[1], c[2]) for c in chans], device)


def score_dirs(estimate, inp=None, clean=None, device="cuda:0"):
    """the rows of ``decay.report_rows`` for every wav name present in ``estimate`` (and in ``inp`` and ``clean``, when given)"""
    names = [n for n in wav_names(estimate) if all(d is None or os.path.exists(os.path.join(d, n)) for d in (inp, clean))]
    if not names:
        raise SystemExit(f"decay: no wav name is common to {', '.join(d for d in (estimate, inp, clean) if d)}")
    cols = [None if d is None else score_files([os.path.join(d, n) for n in names], device) for d in (inp, estimate, clean)]
    for c in cols:
        if c is not None and c[0] != cols[1][0]:
            raise SystemExit("decay: the wavs of a pair differ in their number of channels")
    return decay.report_rows(cols[1][0], None if cols[0] is None else cols[0][1], cols[1][1], None if cols[2] is None else cols[2][1])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("paths", nargs="*", help="a mode directory of a test run, or wav files")
    ap.add_argument("--input", help="directory of the degraded wavs (fills the _in and _delta columns)")
    ap.add_argument("--estimate", help="directory of the wavs to score")
    ap.add_argument("--out", help="directory for decay.csv and decay_summary.csv")
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
        names, scored = score_files(a.paths, a.device)
        rows = decay.report_rows(names, None, scored)
        out = a.out
        for r in rows:
            print(f"{r['file']}: T60 {r['t60_out']:.3f} s  regions {r['regions_out']}  spread {r['spread_out']:.3f} s  flags {r['flags_out']}  frames {r['frames_out']}")
    else:
        if not a.estimate:
            ap.error("give a mode directory, wav files, or --estimate")
        rows = score_dirs(a.estimate, a.input, None, a.device)
        out = a.out or a.estimate
    summary = decay.summary_rows(rows)
    print(decay.format_summary(summary))
    if out:
        os.makedirs(out, exist_ok=True)
        decay.write_report(os.path.join(out, "decay.csv"), rows)
        decay.write_report(os.path.join(out, "decay_summary.csv"), summary)
        print(os.path.join(out, "decay.csv"))
    return rows


if __name__ == "__main__":
    main()
