#!/usr/bin/env python
"""Time the projection SDR report (csrc/sdr.hip, utils/sdr.py) with HIP events at 16 kHz and the default filter lengths (N = 2048): the whole
``sdr.evaluate`` at B = 8 x 64 000 samples, its two C entries separately, and the whole call on one row of 60 s; the median of ``--rounds`` timed calls
after warm-up, every C entry with its own copy of the row lengths to the host, written as one JSON object (default profiles/sdr_time.json).  These are
times per call as the tester pays them, not kernel times.  ``buddy_sdr_solve`` is N dependent steps of one workgroup per row: latency-bound by
construction.  No target is attached; the float64 numpy restatement of one row (lag sums by dot products, one dense LU per order) is timed once on
the host and sits next to it for scale."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_clean, synth_rir  # noqa: E402
from buddy_amd.utils import sdr as S  # noqa: E402


def timed(fn, rounds):
    """[median, min] ms of ``rounds`` calls of ``fn`` between HIP events, after three warm-up calls"""
    for _ in range(3):
        fn()
    ts = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1))
    return [round(statistics.median(ts), 4), round(min(ts), 4)]


def pair(B, L):
    xs = np.stack([synth_clean(u, L) for u in range(B)]).astype(np.float32)
    es = np.stack([signal.fftconvolve(xs[u], synth_rir(u, 4000))[:L].astype(np.float32) for u in range(B)])
    return torch.from_numpy(es).cuda(), torch.from_numpy(xs).cuda()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--length", type=int, default=64000)
    ap.add_argument("--long", type=int, default=960000, help="samples of the one long row")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdr_time.json"))
    a = ap.parse_args(argv)
    lib = _lib.require_gpu()
    B, L, fs, N, J = a.batch, a.length, S.FS, S.TAPS[-1], len(S.TAPS)
    e, x = pair(B, L)
    res = {"batch": B, "length": L, "fs": fs, "taps": list(S.TAPS), "rounds": a.rounds, "unit": "ms per call, median (min)"}
    res["evaluate_whole_call"] = timed(lambda: S.evaluate(e, x, fs), a.rounds)
    res["values_db"] = [[round(float(v), 6) for v in row] for row in S.evaluate(e, x, fs).values]
    # the two entries separately, on the buffers evaluate makes
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    r, d = (torch.empty(B, N, dtype=torch.float64, device="cuda") for _ in range(2))
    ee, val, p = torch.empty(B, dtype=torch.float64, device="cuda"), *(torch.empty(B, J, dtype=torch.float64, device="cuda") for _ in range(2))
    fl = torch.empty(B, dtype=torch.int32, device="cuda")
    nbytes = lib.buddy_sdr_products_workspace(B, L, N)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    st, taps = _lib.stream_ptr(), (_lib.C.c_int * J)(*S.TAPS)
    res["buddy_sdr_products"] = timed(lambda: _lib.check(lib.buddy_sdr_products(_lib.ptr(e), _lib.ptr(x), lens.data_ptr(), B, L, N, r.data_ptr(), d.data_ptr(),
                                                                                ee.data_ptr(), ws.data_ptr(), nbytes, st)), a.rounds)
    res["buddy_sdr_solve"] = timed(lambda: _lib.check(lib.buddy_sdr_solve(r.data_ptr(), d.data_ptr(), ee.data_ptr(), lens.data_ptr(), B, N, taps, J, S.LOADING,
                                                                          val.data_ptr(), p.data_ptr(), fl.data_ptr(), None, st)), a.rounds)
    res["products_multiply_adds"] = 2 * B * L * N
    e1, x1 = pair(1, a.long)
    res["long_row_samples"] = a.long
    res["evaluate_one_long_row"] = timed(lambda: S.evaluate(e1, x1, fs), a.rounds)
    import _sdr_ref as R  # the float64 restatement of the tests
    t0 = time.perf_counter()
    want = R.evaluate(e[0].cpu().numpy(), x[0].cpu().numpy(), S.TAPS)[0]
    res["numpy_restatement_one_row_ms"] = round(1000.0 * (time.perf_counter() - t0), 1)
    res["numpy_restatement_minus_library_db"] = [float(w - float(v)) for w, v in zip(want, S.evaluate(e[:1], x[:1], fs).values[0])]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
