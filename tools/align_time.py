#!/usr/bin/env python
"""Time the alignment step (csrc/align.hip) with HIP events at B = 8 x 64 000 samples, 16 kHz, K = 800 (+-50 ms): the median of `--rounds` timed
calls per entry after warm-up, written as one JSON object (default profiles/align_time.json).  Each C entry includes its own copy of the row
lengths to the host (a stream synchronise), so these are times per call as the tester pays them, not kernel times.  No target is attached."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_clean  # noqa: E402
from buddy_amd.utils import metrics as M  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--length", type=int, default=64000)
    ap.add_argument("--max-lag", type=int, default=800, help="K, the search window in samples")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "align_time.json"))
    a = ap.parse_args(argv)
    lib = _lib.require_gpu()
    B, L, K, fs = a.batch, a.length, a.max_lag, 16000
    rs = np.random.RandomState(0)
    xs = np.stack([synth_clean(u, L + 64)[32:32 + L] for u in range(B)])
    es = np.stack([(synth_clean(u, L + 64)[32 - u:32 - u + L] + 0.3 * xs[u].std() * rs.standard_normal(L)).astype(np.float32) for u in range(B)])      # row u is u samples late
    x, e = torch.from_numpy(xs).cuda(), torch.from_numpy(es).cuda()
    st = _lib.stream_ptr()
    dev = x.device
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    lag, fl, lens_o = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    out = torch.empty(B, 2, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.buddy_xcorr_lag_workspace(B, L, K) // 8, dtype=torch.float64, device=dev)
    eo, xo = torch.empty_like(e), torch.empty_like(x)

    def xcorr():
        _lib.check(lib.buddy_xcorr_lag(_lib.ptr(e), _lib.ptr(x), lens.data_ptr(), B, L, K, lag.data_ptr(), out.data_ptr(), fl.data_ptr(), None, ws.data_ptr(),
                                       ws.numel() * 8, st))

    def pair():
        _lib.check(lib.buddy_align_pair(_lib.ptr(e), _lib.ptr(x), lens.data_ptr(), lag.data_ptr(), B, L, _lib.ptr(eo), _lib.ptr(xo), L, lens_o.data_ptr(), st))

    def whole():
        M.align(e, x, fs, max_lag_ms=1000.0 * K / fs)

    res = {"batch": B, "length": L, "fs": fs, "max_lag": K, "rounds": a.rounds, "unit": "ms per call, median (min)",
           "multiply_adds": B * L * (2 * K + 1), "workspace_bytes": ws.numel() * 8}
    for name, fn in (("xcorr_lag", xcorr), ("align_pair", pair), ("align_whole_call", whole)):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(a.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ts.append(t0.elapsed_time(t1))
        res[name] = [round(statistics.median(ts), 4), round(min(ts), 4)]
    res["lags"] = lag.cpu().tolist()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
