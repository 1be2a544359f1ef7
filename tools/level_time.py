#!/usr/bin/env python
"""Time the active speech level meter (csrc/level.hip, buddy_amd/utils/level.py) with HIP events: the median of `--rounds` timed calls after warm-up,
per C entry and for the whole ``speech_level`` call, at two shapes -- B = 8 rows of 64 000 samples and one row of 600 s, both at 16 kHz -- written as
one JSON object (default profiles/level_time.json).  Each C entry includes its own copy of the row lengths (and of ref / offset) to the host, a
stream synchronise, so these are times per call as a caller pays them, not kernel times.  Measured once; no target is attached."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import level as lv  # noqa: E402


def timed(fn, rounds):
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


def shape(lib, B, L, fs, rounds):
    rs = np.random.RandomState(0)
    gate = (np.sin(2 * np.pi * 0.7 * np.arange(L) / fs + rs.uniform(0, 6, (B, 1))) > 0.2).astype(np.float32)      # bursts and pauses
    x = torch.from_numpy((0.1 * rs.standard_normal((B, L))).astype(np.float32) * gate).cuda()
    st = _lib.stream_ptr()
    dev = x.device
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    off = torch.zeros(B, dtype=torch.float64, device=dev)
    ref = x.abs().amax(dim=1).double()
    stats = torch.empty(B, 2, dtype=torch.float64, device=dev)
    klass = torch.empty(B, L, dtype=torch.uint8, device=dev)
    sq = torch.empty(B, dtype=torch.float64, device=dev)
    counts = torch.empty(B, 16, dtype=torch.int64, device=dev)
    ws = [lv._workspace(q, B, L, dev) for q in (lib.buddy_level_stats_workspace, lib.buddy_level_classes_workspace, lib.buddy_level_counts_workspace)]
    hang = lv.hangover_samples(lv.HANGOVER, fs)

    def stats_fn():
        _lib.check(lib.buddy_level_stats(_lib.ptr(x), L, lens.data_ptr(), B, stats.data_ptr(), ws[0][0].data_ptr(), ws[0][1], st))

    def classes_fn():
        _lib.check(lib.buddy_level_classes(_lib.ptr(x), L, lens.data_ptr(), off.data_ptr(), ref.data_ptr(), B, float(fs), lv.TIME_CONSTANT, klass.data_ptr(), L,
                                           sq.data_ptr(), ws[1][0].data_ptr(), ws[1][1], st))

    def counts_fn():
        _lib.check(lib.buddy_level_counts(klass.data_ptr(), L, lens.data_ptr(), B, hang, counts.data_ptr(), ws[2][0].data_ptr(), ws[2][1], st))

    res = {"batch": B, "length": L, "fs": fs, "level_stats": timed(stats_fn, rounds), "level_classes": timed(classes_fn, rounds),
           "level_counts": timed(counts_fn, rounds), "speech_level_whole_call": timed(lambda: lv.speech_level(x, fs), rounds)}
    r = lv.speech_level(x, fs)
    res["level_db"], res["activity"] = [round(float(v), 4) for v in r.level_db], [round(float(v), 4) for v in r.activity]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "level_time.json"))
    a = ap.parse_args(argv)
    lib = _lib.require_gpu()
    res = {"unit": "ms per call, median (min)", "rounds": a.rounds, "note": "measured once, no target",
           "shapes": [shape(lib, 8, 64000, 16000, a.rounds), shape(lib, 1, 600 * 16000, 16000, a.rounds)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
