#!/usr/bin/env python
"""Compare two runs over the same files (buddy_amd/utils/compare.py): per score column of their reports the mean and median
paired difference (run B minus run A) with percentile bootstrap intervals, a sign-flip randomisation test, the sign test and Holm-adjusted p-values.

    python tools/compare.py RUN_A RUN_B                      # every report both runs hold: metrics, spectral, sdr, srmr, decay, denoise, levels
    python tools/compare.py RUN_A RUN_B --report metrics --columns si_sdr_out stoi_out
    python tools/compare.py a/metrics.csv b/metrics.csv      # two CSV files of one report
    python tools/compare.py RUN                              # one run: its own *_delta columns against zero (does the method improve on its input?)

``RUN_*`` are mode directories of a test run (or any folder that holds the report CSVs) or CSV files written by ``report.write_report``; the lines
are joined on the ``file`` column.  Writes ``comparison_<report>.csv`` into ``--out`` (default: RUN_B, or the one run) and prints the same as aligned
text.  Files present in one run only are counted, listed on stderr and flagged UNPAIRED; no common file is an error.  The resampling runs on the GPU
and repeats for the same ``--seed``."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.utils import compare  # noqa: E402

REPORTS = ("metrics", "spectral", "sdr", "srmr", "decay", "denoise", "levels")


def report_paths(run_a, run_b, asked):
    """[(report name, path in A, path in B or None)] for two folders, two CSV files, or one of either"""
    runs = [r for r in (run_a, run_b) if r is not None]
    for r in runs:
        if not os.path.exists(r):
            raise SystemExit(f"compare: {r} does not exist")
    if len({os.path.isdir(r) for r in runs}) > 1:
        raise SystemExit(f"compare: give two folders or two CSV files, not one of each ({run_a}, {run_b})")
    if not os.path.isdir(run_a):
        name = os.path.splitext(os.path.basename(run_a))[0]
        if asked and list(asked) != [name]:
            raise SystemExit(f"compare: --report {' '.join(asked)} does not name the file {run_a}")
        return [(name, run_a, run_b)]
    for r in asked or ():
        if r not in REPORTS:
            raise SystemExit(f"compare: --report takes {', '.join(REPORTS)}, got {r!r}")
    found = []
    for r in asked or REPORTS:
        paths = [os.path.join(d, r + ".csv") for d in runs]
        if all(os.path.isfile(p) for p in paths):
            found.append((r, paths[0], paths[1] if run_b is not None else None))
        elif asked:
            raise SystemExit(f"compare: {r}.csv is not in {' and '.join(runs)}")
    if not found:
        raise SystemExit(f"compare: no report ({', '.join(v + '.csv' for v in REPORTS)}) is in {' and '.join(runs)}")
    return found


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("run_a", help="mode directory or report CSV of run A (alone: its *_delta columns against zero)")
    ap.add_argument("run_b", nargs="?", help="mode directory or report CSV of run B")
    ap.add_argument("--report", nargs="+", help=f"reports to compare (default: those of {', '.join(REPORTS)} that both runs hold)")
    ap.add_argument("--columns", nargs="+", help="score columns (default: every numeric score column)")
    ap.add_argument("--resamples", type=int, default=10000)
    ap.add_argument("--permutations", type=int, default=100000)
    ap.add_argument("--level", type=float, default=0.95)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", help="directory for comparison_<report>.csv (default: RUN_B)")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not 1 <= a.permutations <= 2 ** 30:
        raise SystemExit(f"compare: --permutations must be in 1..2^30, got {a.permutations}")
    if not 1 <= a.resamples <= 2 ** 24:
        raise SystemExit(f"compare: --resamples must be in 1..2^24, got {a.resamples}")
    try:
        compare.interval_ranks(a.resamples, a.level)
    except ValueError as e:
        raise SystemExit(f"compare: --resamples / --level: {e}")
    found = report_paths(a.run_a, a.run_b, a.report)
    last = a.run_b if a.run_b is not None else a.run_a
    out = a.out or (last if os.path.isdir(last) else os.path.dirname(os.path.abspath(last)))
    results = {}
    for name, pa, pb in found:
        try:
            tab = compare.compare_reports(pa, pb, a.columns)
        except ValueError as e:
            if a.columns is None and len(found) > 1 and "no score column" in str(e):
                continue                       # a report without a comparable column (one run: without a *_delta column) among several
            raise SystemExit(str(e))
        for side, names in (("A", tab["only_a"]), ("B", tab["only_b"])):
            if names:
                print(f"compare: {name}: {len(names)} file(s) in run {side} only: {' '.join(names)}", file=sys.stderr)
        try:
            recs = compare.paired(tab["a"], tab["b"], tab["labels"], a.seed, a.resamples, a.permutations, a.level, a.device, len(tab["only_a"]),
                                  len(tab["only_b"]))
        except ValueError as e:
            raise SystemExit(f"compare: {name}: {e}")
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, f"comparison_{name}.csv")
        compare.write_comparison(path, recs)
        print(f"{name}: {len(tab['files'])} common files" + ("" if pb is not None else " (one run: *_delta against zero)"))
        print(compare.format_comparison(recs))
        print(path)
        results[name] = recs
    if not results:
        raise SystemExit(f"compare: no score column to compare in {a.run_a}" + ("" if a.run_b is None else f" and {a.run_b}"))
    return results


if __name__ == "__main__":
    main()
