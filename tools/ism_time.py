#!/usr/bin/env python
"""Time the room simulator (csrc/ism.hip) with HIP events: eight drawn rooms x 1 s at 16 kHz in one call, no order cap; the median of `--rounds` timed
calls after warm-up, written as one JSON object (default profiles/ism_time.json) with the rooms' estimated image counts.  No target is attached."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import rooms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ism_time.json"))
    a = ap.parse_args(argv)
    lib = _lib.require_gpu()
    B, fs, n = a.batch, a.fs, int(round(a.seconds * a.fs))
    drawn = rooms.draw_rooms([f"room{b}" for b in range(B)], a.seed)
    est = rooms.estimated_images(drawn, fs, n)
    r = torch.from_numpy(drawn).cuda()
    h = torch.empty(B, n, dtype=torch.float32, device="cuda")
    flags = torch.empty(B, dtype=torch.int32, device="cuda")
    st = _lib.stream_ptr()

    def call():
        _lib.check(lib.buddy_shoebox_rir(r.data_ptr(), B, fs, n, -1, _lib.ptr(h), n, flags.data_ptr(), st))

    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1))
    res = {"batch": B, "fs": fs, "samples": n, "max_order": -1, "rounds": a.rounds, "unit": "ms per call, median (min)",
           "tile": lib.buddy_ism_tile(), "list": lib.buddy_ism_list(), "half_width": lib.buddy_ism_half_width(),
           "volumes_m3": [round(float(v), 2) for v in drawn[:, 0] * drawn[:, 1] * drawn[:, 2]],
           "estimated_images": [float(f"{v:.4g}") for v in est], "estimated_images_total": float(f"{float(est.sum()):.4g}"),
           "shoebox_rir": [round(statistics.median(ts), 3), round(min(ts), 3)], "flags": flags.cpu().tolist()}
    res["ns_per_image_tap"] = round(1e6 * statistics.median(ts) / (float(est.sum()) * 2 * lib.buddy_ism_half_width()), 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
