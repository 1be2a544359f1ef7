#!/usr/bin/env python
"""Time multichannel WPE (buddy_amd/utils/wpe.py::wpe_mc_dereverb) on the GPU and write ``profiles/wpe_mc_time.json``.  A record, not a gate:
the call runs once per file, outside the sampling loop.

    python tools/wpe_mc_time.py [--out profiles/wpe_mc_time.json] [--repeats 5] [--calls 3]

Three shapes, taps 10 / delay 3 / 3 iterations (nara_wpe's defaults) for the multichannel ones:

    batch      wpe_mc_dereverb, B = 8 x D = 8 x 64 000 samples (eight 4 s array recordings)
    long_row   wpe_mc_dereverb, B = 1 x D = 8 x 960 000 samples (one 60 s array recording: 257 workgroups, one per bin)
    warm_start the existing one-channel wpe_dereverb at B = 8 x 64 000 with ITS defaults (taps 50, delay 2, 5 iterations), for scale

Per shape: one warm-up call, then ``--repeats`` windows of ``--calls`` calls each between two device events; the JSON holds every window's
milliseconds per call, their median, minimum and maximum (the spread), and the work the algorithm needs (complex multiply-adds of R, P,
the Cholesky factorisation and the filter, counted from the shapes)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.utils import wpe  # noqa: E402


def cmacs(B, D, L, taps, iterations):
    """complex multiply-adds of one call: per problem and iteration N (N + 1) / 2 T for R, N D T for P, N^3 / 6 for Cholesky, N D T for the filter"""
    N, T = D * taps, wpe.frames(L)
    return B * 257 * iterations * (N * (N + 1) // 2 * T + 2 * N * D * T + N ** 3 // 6)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wpe_mc_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("wpe_mc_time: needs the GPU (a time taken elsewhere says nothing)")
    g = torch.Generator(device="cuda").manual_seed(0)
    shapes = [("batch", (8, 8, 64000), dict(taps=10, delay=3, iterations=3)),
              ("long_row", (1, 8, 960000), dict(taps=10, delay=3, iterations=3)),
              ("warm_start", (8, 64000), dict(taps=50, delay=2, iterations=5))]
    result = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_window": a.calls, "shapes": {}}
    for name, shape, hp in shapes:
        y = 0.05 * torch.randn(*shape, device="cuda", generator=g)
        fn = (lambda: wpe.wpe_mc_dereverb(y, **hp)) if len(shape) == 3 else (lambda: wpe.wpe_dereverb(y, **hp))
        out = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        ms = [window(fn, a.calls) for _ in range(a.repeats)]
        B, D, L = shape if len(shape) == 3 else (shape[0], 1, shape[1])
        work = cmacs(B, D, L, hp["taps"], hp["iterations"])
        med = float(np.median(ms))
        result["shapes"][name] = {"shape": list(shape), **hp, "frames": wpe.frames(L), "ms_per_call": [round(v, 4) for v in ms], "median_ms": round(med, 4),
                                  "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "complex_macs": work,
                                  "gflops_fp64_at_median": round(8.0 * work / (med * 1e-3) / 1e9, 1)}
        print(f"{name}: {shape} {hp}: median {med:.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f}), {8.0 * work / (med * 1e-3) / 1e9:.0f} GFLOP/s fp64 "
              "(whole call, STFT and iSTFT included in the time, not in the work)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(a.out)
    return result


if __name__ == "__main__":
    main()
