#!/usr/bin/env python
"""Time the spectral distortion report (csrc/spectral.hip, utils/spectral.py) with HIP events at B = 8 x 64 000 samples, 16 kHz: the median of
`--rounds` timed calls of the whole ``spectral.evaluate`` after warm-up -- two magnitude-spectra calls, the cepstral distance, fwSegSNR and LLR, every C
entry with its own copy of the row lengths to the host -- written as one JSON object (default profiles/spectral_time.json).  These are times per call as
the tester pays them, not kernel times.  No target is attached."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_clean, synth_rir  # noqa: E402
from buddy_amd.utils import spectral as S  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--length", type=int, default=64000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spectral_time.json"))
    a = ap.parse_args(argv)
    _lib.require_gpu()
    B, L, fs = a.batch, a.length, S.FS
    from scipy import signal
    xs = np.stack([synth_clean(u, L) for u in range(B)]).astype(np.float32)
    es = np.stack([signal.fftconvolve(xs[u], synth_rir(u, 4000))[:L].astype(np.float32) for u in range(B)])
    x, e = torch.from_numpy(xs).cuda(), torch.from_numpy(es).cuda()
    res = {"batch": B, "length": L, "fs": fs, "rounds": a.rounds, "unit": "ms per call, median (min)"}
    for name, values in (("evaluate_whole_call", S.VALUES), ("evaluate_cd_only", ("cd",)), ("evaluate_llr_only", ("llr",)), ("evaluate_fwsegsnr_only", ("fwsegsnr",))):
        for _ in range(3):
            r = S.evaluate(e, x, fs, values=values)
        ts = []
        for _ in range(a.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            r = S.evaluate(e, x, fs, values=values)
            t1.record()
            torch.cuda.synchronize()
            ts.append(t0.elapsed_time(t1))
        res[name] = [round(statistics.median(ts), 4), round(min(ts), 4)]
        if values == S.VALUES:
            res["frames"] = r.frames.tolist()
            res["values"] = [[round(float(v), 6) for v in row] for row in r.values]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
