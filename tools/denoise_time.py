#!/usr/bin/env python
"""Time the noise tracker and spectral post-filter (buddy_amd/utils/denoise.py, csrc/denoise.hip) on the GPU and write ``profiles/denoise_time.json``.
A record, not a gate: the call runs once per file, and its tracker is latency-bound by construction (257 B threads, one dependent step per frame),
so there is no target and no rate.

    python tools/denoise_time.py [--out profiles/denoise_time.json] [--repeats 5] [--calls 1]

Shapes (white noise of standard deviation 0.05 under a 3 Hz amplitude modulation, 16 kHz):

    batch       B = 8 x 64 000 samples (eight 4 s recordings): 503 frames per row
    long_row    B = 1 x 960 000 samples (one 60 s recording): 7503 frames

Per shape the whole ``denoise`` call with both gain rules, and each stage alone (``spectra_hip``, ``gains_hip`` with both rules, ``synthesis_hip``) on
tensors already on the GPU: one warm-up call, then ``--repeats`` windows of ``--calls`` calls each between two device events; the JSON holds every
window's milliseconds per call, their median, minimum and maximum (the spread)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.utils import denoise as dn  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "denoise_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("denoise_time: needs the GPU (a time taken elsewhere says nothing)")
    fs = 16000
    result = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_window": a.calls, "fs": fs, "shapes": {}}

    def record(shape, name, fn):
        fn()
        torch.cuda.synchronize()
        ms = [window(fn, a.calls) for _ in range(a.repeats)]
        med = float(np.median(ms))
        result["shapes"][shape]["entries"][name] = {"ms_per_call": [round(v, 4) for v in ms], "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
                                                    "max_ms": round(max(ms), 4)}
        print(f"{shape} {name}: median {med:.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f})")

    for tag, (B, L) in (("batch", (8, 64000)), ("long_row", (1, 960000))):
        rs = np.random.RandomState(0)
        env = 1.0 + 0.5 * np.sin(2.0 * np.pi * 3.0 * np.arange(L) / fs)
        x = torch.from_numpy((0.05 * env[None, :] * rs.standard_normal((B, L))).astype(np.float32)).cuda()
        lens = [L] * B
        result["shapes"][tag] = {"shape": [B, L], "frames": dn.frames(L), "entries": {}}
        for rule in dn.GAINS:
            record(tag, f"denoise_{rule}", lambda: dn.denoise(x, gain=rule))
        Y = dn.spectra_hip(x)
        phi = dn.row_floor(x, torch.tensor(lens, dtype=torch.int32))
        G, _ = dn.gains_hip(Y, lens, phi)
        assert torch.isfinite(dn.synthesis_hip(Y, G, lens)).all()
        record(tag, "spectra", lambda: dn.spectra_hip(x))
        for rule in dn.GAINS:
            record(tag, f"gains_{rule}", lambda: dn.gains_hip(Y, lens, phi, rule))
        record(tag, "synthesis", lambda: dn.synthesis_hip(Y, G, lens))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(a.out)
    return result


if __name__ == "__main__":
    main()
