#!/usr/bin/env python
"""Measure the active speech level (ITU-T P.56 method B as restated in DESIGN.md section 23; buddy_amd/utils/level.py) of wavs, on the GPU.

    python tools/speech_level.py a.wav b.wav dir/ ...                # one row per file (folders are walked for *.wav)
    python tools/speech_level.py <training wavs> --segment-seconds 4.096 --fs-out 16000 --out levels.csv

Int or float wavs of any rate and channel count, read as the real-recordings mode reads them (``AudioFolder``: integer formats scaled by their full
scale, several channels mixed down by their mean), measured at their own rate or, with ``--fs-out``, after the project's resampler.
``--segment-seconds S`` cuts every file into consecutive full segments of S seconds, each a row: this is how the training loader sees speech, and
the MEDIAN ACTIVITY the summary then prints is the ``real_recordings.reference_activity`` that ``level: active`` asks for.  Prints the per-row
values and a summary (n, mean, median, std of level_db, activity and rms_db - level_db); ``--out`` also writes the rows as CSV and the summary next
to it (``<out>`` with ``_summary`` before the extension)."""
import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.datasets.recordings import AudioFolder  # noqa: E402
from buddy_amd.utils import level as lv  # noqa: E402

BATCH_SAMPLES = 1 << 22                              # padded samples per call


def wav_paths(paths):
    out = []
    for p in paths:
        if os.path.isdir(p):
            out += sorted(glob.glob(os.path.join(p, "**", "*.wav"), recursive=True))
        else:
            out.append(p)
    if not out:
        raise SystemExit("speech_level: no wav given or found")
    return out


def read_rows(paths, segment_seconds=None, fs_out=None, device="cuda:0"):
    """(name, 1-D float32 GPU tensor, rate) per row: a file, or each of its consecutive full segments (``name#k``)"""
    from buddy_amd.utils.resample import resample
    rows = []
    reader = AudioFolder.__new__(AudioFolder)
    for p in paths:
        reader.files = [p]
        audio, fs, name = reader[0]
        y = torch.from_numpy(np.asarray(audio)).float().to(device)
        if fs_out is not None and int(fs_out) != fs:
            y, fs = resample(y, fs, int(fs_out)), int(fs_out)
        if segment_seconds is None:
            rows.append((name[:-4], y, fs))
            continue
        seg = int(round(float(segment_seconds) * fs))
        if seg < 1:
            raise SystemExit("speech_level: --segment-seconds is below one sample")
        rows += [(f"{name[:-4]}#{k}", y[k * seg:(k + 1) * seg], fs) for k in range(y.numel() // seg)]
    return rows


def measure(rows, full_scale="peak", device="cuda:0"):
    """``lv.report_rows`` of all rows; rows of one rate share zero-padded batches (a row's result does not depend on its batch)"""
    out = [None] * len(rows)
    by_rate = {}
    for i, (_, _, fs) in enumerate(rows):
        by_rate.setdefault(fs, []).append(i)
    for fs, idx in by_rate.items():
        idx = sorted(idx, key=lambda i: rows[i][1].numel())
        s = 0
        while s < len(idx):
            e = s + 1
            while e < len(idx) and (e + 1 - s) * rows[idx[e]][1].numel() <= BATCH_SAMPLES:
                e += 1
            part = idx[s:e]
            lens = [rows[i][1].numel() for i in part]
            xb = torch.zeros(len(part), max(max(lens), 1), dtype=torch.float32, device=device)
            for b, i in enumerate(part):
                xb[b, :lens[b]] = rows[i][1]
            res = lv.speech_level(xb, fs, lengths=lens, full_scale=full_scale)
            for b, r in enumerate(lv.report_rows([rows[i][0] for i in part], res, [{"fs": fs}] * len(part))):
                out[part[b]] = r
            s = e
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("paths", nargs="+", help="wav files or folders of them")
    ap.add_argument("--segment-seconds", type=float, default=None, help="cut every file into consecutive full segments of this length, each a row")
    ap.add_argument("--fs-out", type=int, default=None, help="resample to this rate first (default: each file at its own rate)")
    ap.add_argument("--full-scale", default="peak", help="'peak' (default: thresholds hang from each row's own peak) or a number such as 1.0 (a fixed grid)")
    ap.add_argument("--out", help="CSV file for the rows; the summary goes next to it")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    full_scale = "peak" if a.full_scale == "peak" else float(a.full_scale)
    rows = measure(read_rows(wav_paths(a.paths), a.segment_seconds, a.fs_out, a.device), full_scale, a.device)
    for r in rows:
        print(f"{r['file']}: level {r['level_db']:.3f} dB  activity {r['activity']:.4f}  rms {r['rms_db']:.3f} dB  peak {r['peak']:.6g}  {r['flags']}".rstrip())
    summary = lv.summary_rows(rows)
    print(lv.format_summary(summary))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        root, ext = os.path.splitext(a.out)
        lv.write_report(a.out, rows)
        lv.write_report(root + "_summary" + (ext or ".csv"), summary)
        print(a.out)
    return rows, summary


if __name__ == "__main__":
    main()
