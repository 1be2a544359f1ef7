"""Compare two runs over the same files (no reference counterpart): per score column the mean and median paired difference
with percentile bootstrap intervals, a paired sign-flip randomisation test (exact by enumeration when there are few files), the exact sign test and
Holm-adjusted p-values over the columns of one report.

The resampling runs on the GPU (``csrc/compare.hip``) on the project's Philox streams (``utils/rng.py``): column ``label`` of a report draws from the
stream ``rng.stream_key(seed, label)``, purposes ``COMPARE_BOOT`` and ``COMPARE_SIGN``, so a comparison repeats for the same seed and a column's
numbers do not depend on which other columns are compared with it.  ``bootstrap``, ``select``, ``sign_flip`` and ``count_ge`` are thin, checked
wrappers of the C entries (a CPU tensor raises ``BuddyHipError``: there is no CPU fallback); ``paired`` is the whole comparison of two
``(files, columns)`` arrays; ``compare_reports`` reads the arrays from two report CSVs (``utils/report.py``).  The cheap statistics (moments, wins and
losses, the sign test, Holm) are host code.  tests/_compare_ref.py restates the GPU part in float64 numpy.

Not here: BCa or studentised intervals (the percentile interval undercovers at small n), Wilcoxon's signed-rank test, unpaired designs, more than
two runs."""
import csv
import math

import numpy as np
import torch

from . import report, rng

COMPARE_BOOT, COMPARE_SIGN = 11, 12          # Philox purposes, the next after rooms.TAIL = 10
FEW, DEGENERATE, EXHAUSTIVE, UNPAIRED = 1, 2, 4, 8   # the flag word of a record
FLAG_NAMES = ((FEW, "FEW"), (DEGENERATE, "DEGENERATE"), (EXHAUSTIVE, "EXHAUSTIVE"), (UNPAIRED, "UNPAIRED"))
RANDOM_MODE, EXHAUSTIVE_MODE = 0, 1
COLUMNS = ("column", "n", "only_a", "only_b", "mean_a", "mean_b", "mean_diff", "mean_lo", "mean_hi", "median_diff", "median_lo", "median_hi", "std_diff",
           "dz", "wins", "losses", "ties", "p_sign", "p_signflip", "p_holm", "patterns", "flags")


def max_pairs():
    """the longest column the bootstrap takes (``buddy_compare_max_pairs``)"""
    from .. import _lib
    return int(_lib.load().buddy_compare_max_pairs())


def interval_ranks(resamples, level):
    """(k, R - 1 - k) with k = floor(alpha R / 2), alpha = 1 - level: the 0-based order statistics of the percentile interval, no interpolation.
    alpha R / 2 is taken 1e-9 up before the floor, so that 0.05 x 1000 / 2 = 25 whatever the last bit of 1 - 0.95.  k >= 1 is required."""
    R, level = int(resamples), float(level)
    if not 0.0 < level < 1.0:
        raise ValueError(f"interval_ranks: level must lie in (0, 1), got {level}")
    if R < 1:
        raise ValueError(f"interval_ranks: resamples must be at least 1, got {R}")
    k = int(math.floor((1.0 - level) * R / 2.0 + 1e-9))
    if k < 1:
        raise ValueError(f"interval_ranks: {R} resamples leave no value outside a {level:g} interval (floor(alpha R / 2) = 0); "
                         f"it takes at least {int(math.ceil(2.0 / (1.0 - level)))}")
    return k, R - 1 - k


def _columns(who, d, lens, keys):
    """the checks the resampling wrappers share, made before anything is launched; -> (d, lens int32 array, keys uint32 (C, 2) array)"""
    if not (torch.is_tensor(d) and d.dim() == 2 and d.dtype == torch.float64):
        raise ValueError(f"{who}: d must be a (C, ld) float64 tensor")
    C, ld = d.shape
    lens = np.asarray(lens)
    if lens.shape != (C,) or lens.dtype.kind not in "iu":
        raise ValueError(f"{who}: lens must hold one integer per column, ({C},)")
    keys = np.asarray(keys)
    if keys.shape != (C, 2) or keys.dtype != np.uint32:
        raise ValueError(f"{who}: keys must be a ({C}, 2) uint32 array (rng.stream_key per column)")
    if C < 1 or C > 32767:
        raise ValueError(f"{who}: 1..32767 columns, got {C}")
    cap = max_pairs()
    if lens.min() < 1:
        raise ValueError(f"{who}: a column is empty")
    if lens.max() > cap:
        raise ValueError(f"{who}: a column holds {int(lens.max())} pairs, above the {cap} that buddy_compare_max_pairs() allows")
    if lens.max() > ld:
        raise ValueError(f"{who}: a length ({int(lens.max())}) is above the row stride ({ld})")
    return d, lens.astype(np.int32), np.ascontiguousarray(keys)


def _draws(who, what, count, draw0, top):
    count, draw0 = int(count), int(draw0)
    if count < 1 or count > top:
        raise ValueError(f"{who}: {what} must be in 1..{top}, got {count}")
    if draw0 < 0 or draw0 + count > 2 ** 32:
        raise ValueError(f"{who}: draw0 + {what} passes 2^32 (draw indices are 32-bit)")
    return count, draw0


def _gpu(who, *tensors):
    from .. import _lib
    for t in tensors:
        if not t.is_cuda:
            raise _lib.BuddyHipError(f"{who}: the comparison runs on the GPU and takes device tensors; there is no CPU fallback")
    return _lib.require_gpu()


def _dev(a, like):
    return torch.from_numpy(np.ascontiguousarray(a)).to(like.device)


def bootstrap(d, lens, keys, resamples, draw0=0):
    """Bootstrap means and medians of C ragged columns.  d: (C, ld) float64 device tensor of finite values (what lies behind a column's length is not
    read); lens (C,) integers; keys (C, 2) uint32.  -> (C, 2, resamples) float64: [c, 0] the resample means, [c, 1] the resample medians.
    The columns are sorted on the device first (plumbing: the kernel counts ranks)."""
    from .. import _lib
    who = "compare.bootstrap"
    d, lens, keys = _columns(who, d, lens, keys)
    R, draw0 = _draws(who, "resamples", resamples, draw0, 2 ** 24)
    lib = _gpu(who, d)
    C, ld = d.shape
    lt = _dev(lens, d)
    live = torch.arange(ld, device=d.device)[None, :] < lt[:, None]
    s = torch.where(live, d, torch.full_like(d, float("inf"))).sort(dim=1).values.contiguous()
    kt = _dev(keys.view(np.int32), d)
    out = torch.empty(C, 2, R, dtype=torch.float64, device=d.device)
    _lib.check(lib.buddy_compare_bootstrap(s.data_ptr(), lt.data_ptr(), kt.data_ptr(), C, ld, R, draw0, out.data_ptr(), _lib.stream_ptr()))
    return out


def select(x, ranks):
    """the order statistics ``ranks`` (0-based, ascending) of every row of x, (M, R) float64 on the device -> (M, len(ranks)): ``np.sort(row)[k]``
    exactly, with -0 below +0"""
    from .. import _lib
    who = "compare.select"
    if not (torch.is_tensor(x) and x.dim() == 2 and x.dtype == torch.float64):
        raise ValueError(f"{who}: x must be an (M, R) float64 tensor")
    M, R = x.shape
    ranks = np.asarray(ranks)
    if ranks.ndim != 1 or ranks.size < 1 or ranks.dtype.kind not in "iu":
        raise ValueError(f"{who}: ranks must be a non-empty list of integers")
    if M < 1 or M > 65535 or R < 1:
        raise ValueError(f"{who}: 1..65535 rows of at least one value, got {M} x {R}")
    if ranks.min() < 0 or ranks.max() >= R:
        raise ValueError(f"{who}: a rank is outside 0..{R - 1}")
    lib = _gpu(who, x)
    x = x.contiguous()
    rt = _dev(ranks.astype(np.int32), x)
    out = torch.empty(M, ranks.size, dtype=torch.float64, device=x.device)
    _lib.check(lib.buddy_compare_select(x.data_ptr(), M, R, R, rt.data_ptr(), int(ranks.size), out.data_ptr(), _lib.stream_ptr()))
    return out


def sign_flip(d, lens, keys, permutations, draw0=0):
    """Sign-flip sums of C ragged columns: -> (T (C, P) float64, tobs (C,) float64, patterns (C,) int64 numpy, modes (C,) int32 numpy).  A column
    with 2^n <= P is enumerated (mode 1: patterns = 2^n, T[c, :2^n] is written and the rest is left as allocated, zeros), the others take P random
    patterns (mode 0)."""
    from .. import _lib
    who = "compare.sign_flip"
    d, lens, keys = _columns(who, d, lens, keys)
    P, draw0 = _draws(who, "permutations", permutations, draw0, 2 ** 30)
    lib = _gpu(who, d)
    C, ld = d.shape
    d = d.contiguous()
    modes = np.array([EXHAUSTIVE_MODE if n <= 30 and 2 ** int(n) <= P else RANDOM_MODE for n in lens], dtype=np.int32)
    patterns = np.where(modes == EXHAUSTIVE_MODE, 2 ** np.minimum(lens, 30).astype(np.int64), P).astype(np.int64)
    lt, mt, kt = _dev(lens, d), _dev(modes, d), _dev(keys.view(np.int32), d)
    T = torch.zeros(C, P, dtype=torch.float64, device=d.device)
    tobs = torch.empty(C, dtype=torch.float64, device=d.device)
    _lib.check(lib.buddy_compare_signflip(d.data_ptr(), lt.data_ptr(), mt.data_ptr(), kt.data_ptr(), C, ld, P, draw0, T.data_ptr(), tobs.data_ptr(),
                                          _lib.stream_ptr()))
    return T, tobs, patterns, modes


def count_ge(T, patterns, thr):
    """#{r < patterns[c] : |T[c, r]| >= thr[c]} -> (C,) int64 device tensor.  T (C, P) float64, thr (C,) float64, both on the device"""
    from .. import _lib
    who = "compare.count_ge"
    if not (torch.is_tensor(T) and T.dim() == 2 and T.dtype == torch.float64 and torch.is_tensor(thr) and thr.dtype == torch.float64
            and thr.shape == (T.shape[0],)):
        raise ValueError(f"{who}: T must be a (C, P) float64 tensor and thr a (C,) float64 tensor")
    C, P = T.shape
    patterns = np.asarray(patterns)
    if patterns.shape != (C,) or patterns.dtype.kind not in "iu" or patterns.min() < 1 or patterns.max() > P:
        raise ValueError(f"{who}: patterns must hold one integer in 1..{P} per column")
    if C < 1 or C > 65535:
        raise ValueError(f"{who}: 1..65535 columns, got {C}")
    lib = _gpu(who, T, thr)
    T, thr = T.contiguous(), thr.contiguous()
    pt = _dev(patterns.astype(np.int32), T)
    out = torch.empty(C, dtype=torch.int64, device=T.device)
    _lib.check(lib.buddy_compare_count_ge(T.data_ptr(), pt.data_ptr(), thr.data_ptr(), C, P, out.data_ptr(), _lib.stream_ptr()))
    return out


# ---- host-only statistics -----------------------------------------------------------------------------------------------------------------------
def sign_test(wins, losses):
    """the exact two-sided binomial sign test of ``wins`` against ``losses`` (ties left out): min(1, 2 P[X <= min(w, l)]), X ~ Binomial(w + l, 1/2);
    1 when there is neither a win nor a loss.  Integer arithmetic throughout (C(m, i + 1) = C(m, i) (m - i) / (i + 1), the sum of ``math.comb``
    without its repeated work) and one correctly rounded integer quotient, so 8192 pairs neither overflow nor round twice"""
    m, k = int(wins) + int(losses), min(int(wins), int(losses))
    if m == 0:
        return 1.0
    term = total = 1
    for i in range(k):
        term = term * (m - i) // (i + 1)
        total += term
    return min(1.0, (2 * total) / (1 << m))


def holm(p):
    """Holm's step-down adjustment of the p-values ``p`` (NaN entries take no part and stay NaN): with the m finite values sorted ascending,
    adj_(i) = max_{j <= i} min(1, (m - j + 1) p_(j))"""
    p = np.asarray(p, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    idx = np.flatnonzero(~np.isnan(p))
    order = idx[np.argsort(p[idx], kind="stable")]
    m, run = len(order), 0.0
    for j, i in enumerate(order):
        run = max(run, min(1.0, (m - j) * float(p[i])))
        out[i] = run
    return out


def flag_names(word):
    return "|".join(name for bit, name in FLAG_NAMES if int(word) & bit) or "-"


def paired(a, b, labels, seed=0, resamples=10000, permutations=100000, level=0.95, device="cuda", only_a=0, only_b=0):
    """Compare run B with run A on the same files.  a, b: (files, columns) float64 arrays, NaN (or +-inf) = undefined; a row of a column counts where
    both sides are finite, d = b - a.  ``a=None``: the one-sample form, b holds the differences themselves (mean_a and mean_b are NaN).
    ``labels``: one name per column (its Philox stream).  ``only_a`` / ``only_b``: files present in one run only, reported and flagged UNPAIRED.
    -> one record (dict with the keys ``COLUMNS``) per column.

    FEW (n < 2): std, dz and the tests are NaN, the intervals are the point (NaN for n = 0).  DEGENERATE: all differences are equal (dz is NaN
    where the standard deviation is 0).  EXHAUSTIVE: 2^n <= permutations, all 2^n sign patterns were enumerated and p = count / 2^n; otherwise
    p = (1 + count) / (1 + permutations).  The intervals are percentile intervals at ``level``: order statistics ``interval_ranks`` of the bootstrap
    values, which undercover at small n.  p_holm adjusts p_signflip over the columns of this call."""
    b = np.asarray(b, dtype=np.float64)
    a = None if a is None else np.asarray(a, dtype=np.float64)
    labels = [str(v) for v in labels]
    if b.ndim != 2 or (a is not None and a.shape != b.shape):
        raise ValueError("compare.paired: a and b must be (files, columns) arrays of one shape")
    if len(labels) != b.shape[1] or len(set(labels)) != len(labels):
        raise ValueError(f"compare.paired: one distinct label per column, {b.shape[1]} columns")
    k_lo, k_hi = interval_ranks(resamples, level)
    _draws("compare.paired", "resamples", resamples, 0, 2 ** 24)
    _draws("compare.paired", "permutations", permutations, 0, 2 ** 30)
    cap = max_pairs()
    nan = float("nan")
    cols, recs = [], []
    for c, label in enumerate(labels):
        with np.errstate(invalid="ignore", over="ignore"):
            d = b[:, c] if a is None else b[:, c] - a[:, c]
        ok = np.isfinite(d) if a is None else np.isfinite(d) & np.isfinite(a[:, c]) & np.isfinite(b[:, c])
        d = np.ascontiguousarray(d[ok])
        n = int(d.size)
        if n > cap:
            raise ValueError(f"compare.paired: column {label!r} holds {n} pairs, above the {cap} that buddy_compare_max_pairs() allows")
        flags = (FEW if n < 2 else 0) | (DEGENERATE if n >= 1 and np.all(d == d[0]) else 0) | (UNPAIRED if only_a or only_b else 0)
        mean = float(np.mean(d)) if n else nan
        med = float(np.median(d)) if n else nan
        std = float(np.std(d, ddof=1)) if n >= 2 else nan
        wins, losses = int(np.sum(d > 0)), int(np.sum(d < 0))
        rec = {"column": label, "n": n, "only_a": int(only_a), "only_b": int(only_b),
               "mean_a": float(np.mean(a[ok, c])) if a is not None and n else nan, "mean_b": float(np.mean(b[ok, c])) if a is not None and n else nan,
               "mean_diff": mean, "mean_lo": mean, "mean_hi": mean, "median_diff": med, "median_lo": med, "median_hi": med, "std_diff": std,
               "dz": mean / std if n >= 2 and std > 0.0 else nan, "wins": wins, "losses": losses, "ties": n - wins - losses,
               "p_sign": sign_test(wins, losses) if n >= 2 else nan, "p_signflip": nan, "p_holm": nan, "patterns": 0, "flags": flags}
        recs.append(rec)
        if n >= 2:
            cols.append((rec, d, rng.stream_key(seed, label)))
    if cols:
        C, ld = len(cols), max(d.size for _, d, _ in cols)
        host = np.zeros((C, ld), dtype=np.float64)
        for i, (_, d, _) in enumerate(cols):
            host[i, :d.size] = d
        lens = np.array([d.size for _, d, _ in cols], dtype=np.int32)
        keys = np.array([k for _, _, k in cols], dtype=np.uint32).reshape(C, 2)
        dev = torch.from_numpy(host).to(device)
        boot = bootstrap(dev, lens, keys, resamples)
        edges = select(boot.view(2 * C, int(resamples)), [k_lo, k_hi]).cpu().numpy().reshape(C, 2, 2)
        T, tobs, patterns, modes = sign_flip(dev, lens, keys, permutations)
        count = count_ge(T, patterns, tobs.abs()).cpu().numpy()
        for i, (rec, _, _) in enumerate(cols):
            rec["mean_lo"], rec["mean_hi"] = float(edges[i, 0, 0]), float(edges[i, 0, 1])
            rec["median_lo"], rec["median_hi"] = float(edges[i, 1, 0]), float(edges[i, 1, 1])
            rec["patterns"] = int(patterns[i])
            if modes[i] == EXHAUSTIVE_MODE:
                rec["p_signflip"], rec["flags"] = int(count[i]) / float(patterns[i]), rec["flags"] | EXHAUSTIVE
            else:
                rec["p_signflip"] = (1.0 + int(count[i])) / (1.0 + int(patterns[i]))
    adj = holm([r["p_signflip"] for r in recs])
    for r, v in zip(recs, adj):
        r["p_holm"] = float(v)
    return recs


# ---- report CSVs --------------------------------------------------------------------------------------------------------------------------------
def _read(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    if not rows or "file" not in rows[0]:
        raise ValueError(f"compare: {path} is not a report of write_report (no 'file' column)")
    head, fi = rows[0], rows[0].index("file")
    table = {}
    for r in rows[1:]:
        if r[fi] in table:
            raise ValueError(f"compare: {path} holds the file {r[fi]!r} twice (a report with several lines per file cannot be joined)")
        table[r[fi]] = dict(zip(head, r))
    return head, table


def _as_float(field):
    """a CSV field as a float (empty = NaN), or None where it is no number"""
    if field == "":
        return float("nan")
    try:
        return float(field)
    except ValueError:
        return None


def _is_int(field):
    return field.lstrip("+-").isdigit()


def score_column(col, fields):
    """Is ``col``, with these fields, a numeric score column?  Never a flag word (``flags*``, ``align_flags*``), an integer lag or the file name.
    Otherwise a column whose non-empty fields are all floats as ``write_report`` writes them (repr, never an integer literal: that leaves the
    counts out, ``samples``, ``frames_out``, ...) -- the ``*_in`` / ``*_out`` / ``*_delta`` columns that ``report.paired`` selects and plain float
    columns such as ``level_db`` alike.  A column without any non-empty field counts where ``report.paired`` selects it (it compares as n = 0)."""
    if col == "file" or col.startswith(("flags", "align_flags")) or col in ("lag_in", "lag_out"):
        return False
    filled = [f for f in fields if f != ""]
    if any(_as_float(f) is None or _is_int(f) for f in filled):
        return False
    return bool(filled) or report.paired(col)


def compare_reports(path_a, path_b=None, columns=None):
    """Read two report CSVs written by ``report.write_report`` and join them on ``file``.  -> dict: ``a`` and ``b``, (files, columns) float64 arrays
    for ``paired`` (an empty field is NaN); ``labels``, the picked columns (``columns``, or every ``score_column`` of both files, in the order of
    A); ``files``, the common names in the order of A; ``only_a`` / ``only_b``, the names in one run only.  With ``path_b=None``: the one-run form,
    ``a`` is None and ``b`` holds the ``*_delta`` score columns of the one report, to be tested against zero."""
    head_a, ta = _read(path_a)
    head_b, tb = (head_a, ta) if path_b is None else _read(path_b)
    files = [f for f in ta if f in tb]
    only_a, only_b = [f for f in ta if f not in tb], [f for f in tb if f not in ta]
    if not files:
        raise ValueError(f"compare: no file is common to {path_a} and {path_b}")
    ok = lambda col, head, t: col in head and score_column(col, [t[f][col] for f in files])
    if columns is None:
        labels = [c for c in head_a if ok(c, head_a, ta) and ok(c, head_b, tb) and (path_b is not None or c.endswith("_delta"))]
    else:
        labels = list(columns)
        for c in labels:
            if not (ok(c, head_a, ta) and ok(c, head_b, tb)):
                raise ValueError(f"compare: {c!r} is not a numeric score column of both reports")
    if not labels:
        raise ValueError(f"compare: no score column to compare in {path_a}" + ("" if path_b is None else f" and {path_b}"))
    grid = lambda t: np.array([[_as_float(t[f][c]) for c in labels] for f in files], dtype=np.float64).reshape(len(files), len(labels))
    return {"a": None if path_b is None else grid(ta), "b": grid(tb), "labels": labels, "files": files, "only_a": only_a, "only_b": only_b}


def write_comparison(path, records):
    report.write_report(path, records)


def format_comparison(records):
    """the records as aligned lines of text (what tools/compare.py prints)"""
    w = max([len(r["column"]) for r in records] + [6])
    lines = [f"{'column':>{w}}  {'n':>5}  {'mean_diff':>11} [{'lo':>11}, {'hi':>11}]  {'median':>11} [{'lo':>11}, {'hi':>11}]  {'dz':>7}  "
             f"{'w/l/t':>11}  {'p_sign':>8}  {'p_flip':>8}  {'p_holm':>8}  {'patterns':>8}  flags"]
    for r in records:
        lines.append(f"{r['column']:>{w}}  {r['n']:5d}  {r['mean_diff']:11.4g} [{r['mean_lo']:11.4g}, {r['mean_hi']:11.4g}]  {r['median_diff']:11.4g} "
                     f"[{r['median_lo']:11.4g}, {r['median_hi']:11.4g}]  {r['dz']:7.3f}  {r['wins']:3d}/{r['losses']:3d}/{r['ties']:3d}  {r['p_sign']:8.4f}  "
                     f"{r['p_signflip']:8.4f}  {r['p_holm']:8.4f}  {r['patterns']:8d}  {flag_names(r['flags'])}")
    return "\n".join(lines)
