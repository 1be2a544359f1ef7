#!/usr/bin/env python
"""Time the three kernels of the SRMR score (csrc/srmr.hip) with HIP events at B = 8 x 64 000 samples, 16 kHz: the median of `--rounds` timed calls
per entry after warm-up, written as one JSON object (default profiles/srmr_time.json).  Each C entry includes its own copy of the row lengths to
the host (a stream synchronise), so these are times per call as the tester pays them, not kernel times.  The envelope entry's arithmetic load
(4 flops per tap and input sample) is reported next to its time.  No target is attached."""
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
from buddy_amd.utils import srmr as S  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--length", type=int, default=64000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "srmr_time.json"))
    a = ap.parse_args(argv)
    lib = _lib.require_gpu()
    B, L, fs = a.batch, a.length, S.FS
    from scipy import signal
    xs = np.stack([signal.fftconvolve(synth_clean(u, L), synth_rir(u, 4000))[:L].astype(np.float32) for u in range(B)])
    x = torch.from_numpy(xs).cuda()
    st = _lib.stream_ptr()
    dev = x.device
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    g_re, g_im, off = S._bank_on(dev)
    J, K, mod = S.CHANNELS, S.MOD_BANDS, S.modulation_bank()
    M = S.frames_of(L)
    env = torch.empty(B, J, L, dtype=torch.float32, device=dev)
    E = torch.empty(B, J, K, M, dtype=torch.float64, device=dev)
    frames, flags = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    out, ebar = torch.empty(B, 3, dtype=torch.float64, device=dev), torch.empty(B, J, K, dtype=torch.float64, device=dev)
    coef = (_lib.C.c_double * (K * 6))(*mod.coef.reshape(-1).tolist())
    erbs = (_lib.C.c_double * J)(*S.erb(S.gammatone_bank().centres[::-1]).tolist())
    low = (_lib.C.c_double * K)(*mod.lower_edges.tolist())

    def envelope():
        _lib.check(lib.buddy_gammatone_env(_lib.ptr(x), lens.data_ptr(), B, L, _lib.ptr(g_re), _lib.ptr(g_im), off, J, _lib.ptr(env), L, st))

    def modulation():
        _lib.check(lib.buddy_modulation_energies(_lib.ptr(env), lens.data_ptr(), B, J, L, coef, K, S.WINDOW, S.HOP, E.data_ptr(), M, frames.data_ptr(), st))

    def scores():
        _lib.check(lib.buddy_srmr_scores(E.data_ptr(), frames.data_ptr(), B, J, K, M, erbs, low, out.data_ptr(), ebar.data_ptr(), flags.data_ptr(), st))

    res = {"batch": B, "length": L, "fs": fs, "rounds": a.rounds, "unit": "ms per call, median (min)"}
    for name, fn in (("gammatone_env", envelope), ("modulation_energies", modulation), ("srmr_scores", scores)):
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
    whole = []
    for _ in range(5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        S.srmr(x, fs)
        t1.record()
        torch.cuda.synchronize()
        whole.append(t0.elapsed_time(t1))
    res["srmr_whole_call"] = [round(statistics.median(whole), 4), round(min(whole), 4)]
    taps = sum(S.gammatone_bank().lengths)
    res["gammatone_env_gflop"] = round(4.0 * taps * B * L / 1e9, 3)
    res["gammatone_env_tflops_at_median"] = round(4.0 * taps * B * L / (res["gammatone_env"][0] * 1e-3) / 1e12, 3)
    res["frames"], res["values"] = frames.cpu().tolist(), [round(float(v), 6) for v in out[:, 0].cpu()]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
