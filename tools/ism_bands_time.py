#!/usr/bin/env python
"""Time the banded room simulator next to the broadband one (csrc/ism.hip) with HIP events: the same eight drawn rooms x 1 s at 16 kHz, no order cap;
`shoebox_rir` on the rows, then `shoebox_bands` + `band_combine` at the default six octave bands and bank.  The median of `--rounds` timed calls after
warm-up, written as one JSON object (default profiles/ism_bands_time.json) with the ratio of the two.  No target is attached."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import rooms  # noqa: E402


def timed(call, rounds):
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        torch.cuda.synchronize()
        ts.append(t0.elapsed_time(t1))
    return [round(statistics.median(ts), 3), round(min(ts), 3)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ism_bands_time.json"))
    a = ap.parse_args(argv)
    lib = _lib.require_gpu()
    B, fs, n = a.batch, a.fs, int(round(a.seconds * a.fs))
    centres = rooms.BAND_CENTRES
    drawn, beta, _ = rooms.draw_band_rooms([f"room{b}" for b in range(B)], a.seed, centres)
    bank = rooms.octave_bank(fs, centres)
    nb, Nh = bank.shape
    est = rooms.estimated_images(drawn, fs, n)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    r, bt, kt = dev(drawn), dev(beta), dev(bank)
    h = torch.empty(B, n, dtype=torch.float32, device="cuda")
    u = torch.empty(B, nb, n, dtype=torch.float64, device="cuda")
    flags = torch.empty(B, dtype=torch.int32, device="cuda")
    st = _lib.stream_ptr()

    def broadband():
        _lib.check(lib.buddy_shoebox_rir(r.data_ptr(), B, fs, n, -1, _lib.ptr(h), n, flags.data_ptr(), st))

    def bands():
        _lib.check(lib.buddy_shoebox_bands(r.data_ptr(), bt.data_ptr(), None, B, nb, fs, n, -1, u.data_ptr(), n, flags.data_ptr(), st))

    def combine():
        _lib.check(lib.buddy_band_combine(u.data_ptr(), B, nb, n, n, kt.data_ptr(), Nh, _lib.ptr(h), n, st))

    def banded():
        bands()
        combine()

    res = {"batch": B, "fs": fs, "samples": n, "max_order": -1, "rounds": a.rounds, "unit": "ms per call, median (min)", "bands": nb, "bank_taps": Nh,
           "tile": lib.buddy_ism_tile(), "list": lib.buddy_ism_list(), "band_list": lib.buddy_ism_band_list(), "combine_tile": lib.buddy_band_combine_tile(),
           "estimated_images_total": float(f"{float(est.sum()):.4g}"),
           "shoebox_rir": timed(broadband, a.rounds), "shoebox_bands": timed(bands, a.rounds), "band_combine": timed(combine, a.rounds),
           "banded_call": timed(banded, a.rounds), "flags": flags.cpu().tolist()}
    res["banded_over_broadband"] = round(res["banded_call"][0] / res["shoebox_rir"][0], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
