"""Room-acoustic parameters of measured room impulse responses: the table the tester's `rir_report` writes for its estimates (EDT, T20, T30, C50,
DRR, Ts; broadband and per octave band; buddy_amd/utils/acoustics.py), for wav files.  Every file is read through the real-recordings reader
(datasets.recordings.AudioFolder: any rate, channels mixed down) and analysed at its OWN rate, nothing is resampled; files of one rate share one
library call.  A `!` behind a decay time marks a fit the end of the response has bent (validity rule); measured responses
carry a noise floor this tool does not remove, so read the flags.
usage: python tools/rir_report.py [--csv OUT.csv] [--centres 125,250,...] <wav files or a folder> ..."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from buddy_amd.datasets.recordings import AudioFolder
from buddy_amd.utils import acoustics


def read_all(paths):
    """[(name, audio float32, fs)] of every wav named or found under a named folder"""
    items = []
    for p in paths:
        if os.path.isdir(p):
            folder = AudioFolder(path=p)
        else:
            folder = AudioFolder.__new__(AudioFolder)      # the same reader for one named file, without a folder scan
            folder.files = [p]
        for i in range(len(folder)):
            audio, fs, name = folder[i]
            items.append((name[:-4], np.asarray(audio, np.float32), int(fs)))
    return items


def analyse(items, centres):
    """report rows of all items, each rate in one call (rows of different lengths go through `lens`); a band the rate cannot hold is dropped for that rate"""
    rows = []
    for fs in sorted({it[2] for it in items}):
        group = [it for it in items if it[2] == fs]
        ok = tuple(c for c in centres if c * 2.0 ** 0.5 <= 0.45 * fs)
        lens = [len(it[1]) for it in group]
        h = torch.zeros(len(group), max(lens))
        for b, it in enumerate(group):
            h[b, :lens[b]] = torch.from_numpy(it[1])
        res = acoustics.rir_acoustics(h.cuda(), fs, lens=lens, centres=ok)
        for r in acoustics.report_rows([it[0] for it in group], res):
            rows.append({"file": r["file"], "fs": fs, **{k: v for k, v in r.items() if k != "file"}})
    return rows


def table(rows):
    lines = [f"{'file':<24} {'fs':>6} {'band':>9} {'EDT[s]':>9} {'T20[s]':>9} {'T30[s]':>9} {'C50[dB]':>8} {'DRR[dB]':>8} {'Ts[ms]':>8}"]
    for r in rows:
        def t(q, name):
            if not (r["flags"] >> q) & 1:
                return f"{'-':>9}"
            return f"{r[name]:>8.3f}" + (" " if (r["flags"] >> (acoustics.FIT_VALID_BIT + q)) & 1 else "!")
        db = lambda q, name: f"{r[name]:>8.2f}" if (r["flags"] >> q) & 1 else f"{'-':>8}"
        lines.append(f"{r['file']:<24} {r['fs']:>6} {r['band']:>9} {t(0, 'EDT')} {t(1, 'T20')} {t(2, 'T30')} {db(3, 'C50')} {db(4, 'DRR')} "
                     + (f"{1e3 * r['Ts']:>8.2f}" if (r["flags"] >> 5) & 1 else f"{'-':>8}"))
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--csv", default=None, help="also write the table as CSV (NaN as an empty field)")
    ap.add_argument("--centres", default=",".join(str(c) for c in acoustics.OCTAVES))
    a = ap.parse_args(argv)
    items = read_all(a.paths)
    if not items:
        print("no wav files found")
        return []
    rows = analyse(items, tuple(float(c) for c in a.centres.split(",") if c))
    print(table(rows))
    if a.csv:
        acoustics.write_report(a.csv, rows)
    return rows


if __name__ == "__main__":
    main()
