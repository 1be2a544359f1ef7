#!/usr/bin/env python
"""Time the wMPDR beamformer after multichannel WPE (buddy_amd/utils/wpe.py::mpdr_hip, wpe_mc_mpdr_dereverb) on the GPU and write
``profiles/mpdr_time.json``.  A record, not a gate: the call runs once per file, outside the sampling loop.

    python tools/mpdr_time.py [--out profiles/mpdr_time.json] [--repeats 5] [--calls 3]

Shapes (WPE: taps 10 / delay 3 / 3 iterations, nara_wpe's defaults; beamformer: 2 iterations, loading 1e-6):

    mpdr_batch       mpdr_hip alone on the spectra of B = 8 x D = 8 x 64 000 samples: (8 * 257, 8, 506) complex128
    fused_batch      wpe_mc_mpdr_dereverb, B = 8 x D = 8 x 64 000 samples (eight 4 s array recordings)
    wpe_batch        wpe_mc_dereverb on the same input: the WPE-only call, for scale
    fused_long_row   wpe_mc_mpdr_dereverb, B = 1 x D = 8 x 960 000 samples (one 60 s array recording)
    wpe_long_row     wpe_mc_dereverb on the same input

Per shape: one warm-up call, then ``--repeats`` windows of ``--calls`` calls each between two device events; the JSON holds every window's
milliseconds per call, their median, minimum and maximum (the spread), and for the beamformer alone the bytes of X it has to read once."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.utils import wpe  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mpdr_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mpdr_time: needs the GPU (a time taken elsewhere says nothing)")
    g = torch.Generator(device="cuda").manual_seed(0)
    hp, bf = dict(taps=10, delay=3, iterations=3), dict(reference=0, bf_iterations=2, loading=1e-6)
    result = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_window": a.calls, "wpe": hp, "beamformer": bf, "shapes": {}}

    def record(name, shape, fn, extra=None):
        out = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(torch.view_as_real(out) if out.is_complex() else out).all()
        ms = [window(fn, a.calls) for _ in range(a.repeats)]
        med = float(np.median(ms))
        result["shapes"][name] = {"shape": list(shape), "ms_per_call": [round(v, 4) for v in ms], "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
                                  "max_ms": round(max(ms), 4), **(extra or {})}
        print(f"{name}: {tuple(shape)}: median {med:.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f})")
        return med

    B, D, L = 8, 8, 64000
    T = wpe.frames(L)
    X = torch.view_as_complex(0.05 * torch.randn(B * 257, D, T, 2, device="cuda", dtype=torch.float64, generator=g))
    nbytes = X.numel() * 16
    med = record("mpdr_batch", X.shape, lambda: wpe.mpdr_hip(X, reference=0, iterations=2, loading=1e-6), {"x_bytes": nbytes})
    result["shapes"]["mpdr_batch"]["x_gbytes_per_s_at_median"] = round(nbytes / (med * 1e-3) / 1e9, 1)
    del X
    for tag, shape in (("batch", (8, 8, 64000)), ("long_row", (1, 8, 960000))):
        y = 0.05 * torch.randn(*shape, device="cuda", generator=g)
        record("fused_" + tag, shape, lambda: wpe.wpe_mc_mpdr_dereverb(y, **hp, **bf), {"frames": wpe.frames(shape[2])})
        record("wpe_" + tag, shape, lambda: wpe.wpe_mc_dereverb(y, **hp), {"frames": wpe.frames(shape[2])})
        del y
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(a.out)
    return result


if __name__ == "__main__":
    main()
