#!/usr/bin/env python
"""Time one whole paired comparison (buddy_amd/utils/compare.py, csrc/compare.hip): ``compare.paired`` at C = 32 columns of
n = 1000 pairs, R = 10 000 resamples and P = 100 000 sign patterns, host work and transfers included (wall clock around the synchronised call,
once after one warm-up call), and the four entries alone (HIP events).  Beside it, for information, the CPU time of the same definitions in
vectorised float64 numpy (plain ``np.sum``, not the tests' exact sums) on ``--cpu-columns`` columns, scaled to C.  No target is attached.
Writes profiles/compare_time.json."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from buddy_amd.utils import compare, rng  # noqa: E402


def numpy_column(d, key, R, P, k, chunk=1000):
    """one column in numpy: the four interval edges and the sign-flip p-value, by the definitions of section 29"""
    s, n = np.sort(d), d.size
    blocks, sblocks = (n + 3) // 4, ((n + 31) // 32 + 3) // 4
    means, meds = np.empty(R), np.empty(R)
    for r0 in range(0, R, chunk):
        draws = np.arange(r0, min(r0 + chunk, R), dtype=np.uint64)
        w = rng.philox4x32_10((np.arange(blocks, dtype=np.uint64)[None, :], draws[:, None], compare.COMPARE_BOOT, 0), key).reshape(len(draws), -1)[:, :n]
        v = s[((w.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)]
        means[r0:r0 + len(draws)], meds[r0:r0 + len(draws)] = v.mean(axis=1), np.median(v, axis=1)
    count, j = 0, np.arange(n)
    tobs = abs(d.sum())
    for r0 in range(0, P, chunk):
        draws = np.arange(r0, min(r0 + chunk, P), dtype=np.uint64)
        w = rng.philox4x32_10((np.arange(sblocks, dtype=np.uint64)[None, :], draws[:, None], compare.COMPARE_SIGN, 0), key).reshape(len(draws), -1)
        sg = 1.0 - 2.0 * ((w[:, j >> 5] >> (j & 31).astype(np.uint32)) & np.uint32(1))
        count += int(np.sum(np.abs(sg @ d) >= tobs))
    means.sort(), meds.sort()
    return means[k], means[R - 1 - k], meds[k], meds[R - 1 - k], (1.0 + count) / (1.0 + P)


def event_ms(call):
    call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = call()
    t1.record()
    torch.cuda.synchronize()
    return round(t0.elapsed_time(t1), 3), out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--columns", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--resamples", type=int, default=10000)
    ap.add_argument("--permutations", type=int, default=100000)
    ap.add_argument("--cpu-columns", type=int, default=1, help="columns of the numpy restatement to time (0: none)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_time.json"))
    a = ap.parse_args(argv)
    C, n, R, P = a.columns, a.pairs, a.resamples, a.permutations
    rs = np.random.RandomState(a.seed)
    run_a = rs.standard_normal((n, C))
    run_b = run_a + 0.05 + 0.5 * rs.standard_normal((n, C))
    labels = [f"score{c}" for c in range(C)]
    call = lambda: compare.paired(run_a, run_b, labels, a.seed, R, P, 0.95)
    call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    recs = call()
    torch.cuda.synchronize()
    res = {"columns": C, "pairs": n, "resamples": R, "permutations": P, "level": 0.95, "unit": "ms, one call after one warm-up call",
           "paired_wall_ms": round(1e3 * (time.perf_counter() - t0), 3)}
    d = torch.from_numpy(np.ascontiguousarray((run_b - run_a).T)).cuda()
    lens = np.full(C, n)
    keys = np.array([rng.stream_key(a.seed, v) for v in labels], dtype=np.uint32)
    k_lo, k_hi = compare.interval_ranks(R, 0.95)
    res["bootstrap_ms"], boot = event_ms(lambda: compare.bootstrap(d, lens, keys, R))
    res["select_ms"], _ = event_ms(lambda: compare.select(boot.view(2 * C, R), [k_lo, k_hi]))
    res["sign_flip_ms"], (T, tobs, patterns, _) = event_ms(lambda: compare.sign_flip(d, lens, keys, P))
    res["count_ge_ms"], _ = event_ms(lambda: compare.count_ge(T, patterns, tobs.abs()))
    res["note"] = ("the wrappers upload their length, key and rank arrays, the bootstrap sorts its columns with torch, and every entry reads its small "
                   "arrays back once to check them, which synchronises the stream: the event times include all of that")
    if a.cpu_columns > 0:
        t0 = time.perf_counter()
        for c in range(a.cpu_columns):
            got = numpy_column(run_b[:, c] - run_a[:, c], keys[c], R, P, k_lo)
            want = (recs[c]["mean_lo"], recs[c]["mean_hi"], recs[c]["median_lo"], recs[c]["median_hi"], recs[c]["p_signflip"])
            assert np.allclose(got[:2], want[:2], rtol=0, atol=1e-12) and got[2:4] == want[2:4] and abs(got[4] - want[4]) <= 2.0 / (1.0 + P), (got, want)
        dt = time.perf_counter() - t0
        res["numpy_cpu_s_per_column"] = round(dt / a.cpu_columns, 3)
        res["numpy_cpu_s_scaled_to_all_columns"] = round(dt / a.cpu_columns * C, 1)
        res["numpy_columns_timed"] = a.cpu_columns
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
