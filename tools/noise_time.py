#!/usr/bin/env python
"""Time the diffuse-noise field (buddy_amd/utils/noise.py::diffuse_noise: the host's filter design, the upload and ``buddy_noise_bank``) on the GPU and
write ``profiles/noise_time.json``.  A record, not a gate: the call runs once per file of a simulated set.

    python tools/noise_time.py [--out profiles/noise_time.json] [--repeats 5] [--calls 1]

Shapes (8 microphones on a circle of 0.1 m, 512 plane waves of the spherical lattice, 16 kHz, white):

    batch       B = 8 x D = 8 x 64 000 samples (eight 4 s array recordings, one geometry each)
    long_row    B = 1 x D = 8 x 960 000 samples (one 60 s array recording)
    bank_batch  ``noise_bank_hip`` alone on the batch, taps already on the GPU: the kernel without the host's share

Per shape: one warm-up call, then ``--repeats`` windows of ``--calls`` calls each between two device events; the JSON holds every window's
milliseconds per call, their median, minimum and maximum (the spread), and the multiply-adds of the bank B L N D W."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.utils import noise, rng  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "noise_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("noise_time: needs the GPU (a time taken elsewhere says nothing)")
    D, N, fs = 8, 512, 16000
    result = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_window": a.calls, "mics": D, "waves": N, "fs": fs,
              "taps": noise.TAPS, "shapes": {}}

    def record(name, shape, fn):
        out = fn()
        torch.cuda.synchronize()
        assert tuple(out.shape) == tuple(shape) and torch.isfinite(out).all()
        ms = [window(fn, a.calls) for _ in range(a.repeats)]
        med = float(np.median(ms))
        macs = shape[0] * shape[2] * N * D * noise.TAPS
        result["shapes"][name] = {"shape": list(shape), "ms_per_call": [round(v, 4) for v in ms], "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
                                  "max_ms": round(max(ms), 4), "multiply_adds": macs, "tera_multiply_adds_per_s_at_median": round(macs / (med * 1e-3) / 1e12, 2)}
        print(f"{name}: {tuple(shape)}: median {med:.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f})")

    def geometry(B):
        phi = 2.0 * np.pi * np.arange(D) / D
        return np.stack([np.stack([0.1 * np.cos(phi + 0.1 * b), 0.1 * np.sin(phi + 0.1 * b), np.zeros(D)], axis=1) for b in range(B)])

    for tag, (B, L) in (("batch", (8, 64000)), ("long_row", (1, 960000))):
        pos = geometry(B)
        keys = np.array([rng.stream_key(0, f"time/{b}") for b in range(B)], dtype=np.uint32)
        record(tag, (B, D, L), lambda: noise.diffuse_noise(pos, keys, L, fs, waves=N))
        if tag == "batch":
            both = [noise.delay_taps(p, noise.sphere_directions(N), fs) for p in pos]
            tt = torch.from_numpy(np.stack([t for t, _ in both])).cuda()
            ft = torch.from_numpy(np.stack([f for _, f in both])).cuda()
            kt = torch.from_numpy(keys.view(np.int32).copy()).cuda()
            record("bank_batch", (B, D, L), lambda: noise.noise_bank_hip(tt, ft, kt, L))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(a.out)
    return result


if __name__ == "__main__":
    main()
