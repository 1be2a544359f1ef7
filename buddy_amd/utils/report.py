"""The CSV conventions of every evaluation report (acoustics, metrics, spectral, SRMR, speech level) in one place: plain text through the csv module,
NaN as an empty field, floats as repr, flags as an integer; the in / out / delta and alignment columns of a paired report; the summary (n, mean,
median, std per column) and its lines of text.  A new report starts here."""
import csv
import math

import numpy as np


def _field(v):
    if isinstance(v, (float, np.floating)):
        return "" if math.isnan(v) else repr(float(v))
    if isinstance(v, (np.integer,)):
        return int(v)
    return v


def write_report(path, rows):
    """``rows``: dicts with the same keys (``report_rows``); the header is the keys of the first row"""
    rows = list(rows)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        if rows:
            cols = list(rows[0].keys())
            wr.writerow(cols)
            for r in rows:
                wr.writerow([_field(r[c]) for c in cols])


def delta_columns(values, asked, inp, out, b):
    """``<m>_in``, ``<m>_out`` and ``<m>_delta`` = out - in of row ``b`` for every value m of ``values`` that is in ``asked``, from two evaluations"""
    row = {}
    for q, m in enumerate(values):
        if m in asked:
            vi, vo = float(inp.values[b, q]), float(out.values[b, q])
            row[m + "_in"], row[m + "_out"], row[m + "_delta"] = vi, vo, vo - vi
    return row


def alignment_columns(inp, out, b):
    """Where an evaluation carries an ``Alignment``: ``lag_in`` / ``lag_out`` (samples, positive: late), ``lag_ms_*``, ``xcorr_*`` (rho) and
    ``align_flags_*`` of row ``b``; the side without one has empty fields and flag word 0.  Without any, nothing."""
    al = [getattr(ev, "alignment", None) for ev in (inp, out)]
    row = {}
    if al[0] is not None or al[1] is not None:
        nan = float("nan")
        for col, get in (("lag", lambda a: int(a.lag[b])), ("lag_ms", lambda a: 1000.0 * int(a.lag[b]) / float(a.fs)), ("xcorr", lambda a: float(a.rho[b])),
                         ("align_flags", lambda a: int(a.flags[b]))):
            for side, a in zip(("_in", "_out"), al):
                row[col + side] = get(a) if a is not None else (0 if col == "align_flags" else nan)
    return row


def paired(col):
    """the column rule of a paired report's summary: the ``*_in`` / ``*_out`` / ``*_delta`` columns but the flag words and the integer lags"""
    return col.endswith(("_in", "_out", "_delta")) and not col.startswith(("flags", "align_flags")) and col not in ("lag_in", "lag_out")


def summarise(rows, select):
    """one dict per selected column: the number of rows where it is defined, and their mean, median and standard deviation (numpy's, population
    form); NaN where no row defines it.  ``select``: a predicate over the column names of the first row (no rows: no summary), or a mapping from a
    name to the function that takes a row to its value (derived columns; summarised even without rows)."""
    rows = list(rows)
    if callable(select):
        select = {col: (lambda r, col=col: r[col]) for col in (rows[0] if rows else ()) if select(col)}
    nan = float("nan")
    out = []
    for col, get in select.items():
        v = np.array([get(r) for r in rows], dtype=np.float64)
        v = v[~np.isnan(v)]
        out.append({"value": col, "n": int(v.size), "mean": float(np.mean(v)) if v.size else nan, "median": float(np.median(v)) if v.size else nan,
                    "std": float(np.std(v)) if v.size else nan})
    return out


def format_summary(summary, name_width, n_width):
    """the summary as lines of text (what the tools print)"""
    return "\n".join(f"{r['value']:>{name_width}}  n {r['n']:{n_width}d}  mean {r['mean']:10.4f}  median {r['median']:10.4f}  std {r['std']:9.4f}" for r in summary)
