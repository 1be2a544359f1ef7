#!/usr/bin/env python
"""Time the three entries of the blind decay time (csrc/decay.hip) with HIP events at B = 8 x 64 000 samples and for one row of 600 s, 16 kHz: the
median of `--rounds` timed calls per entry after warm-up, written as one JSON object (default profiles/decay_time.json).  Each C entry includes its
own copy of the row lengths to the host (a stream synchronise), so these are times per call as the tester pays them, not kernel times.  No target is
attached: the work is small and latency-bound."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import decay as D  # noqa: E402


def bursts(seed, n, t60=0.5):
    """gated noise bursts through an exponentially decaying noise response: a signal with free decays"""
    rs = np.random.RandomState(seed)
    gate = np.repeat((rs.uniform(size=n // 4000 + 1) < 0.5).astype(np.float64), 4000)[:n]
    h = np.exp(-6.908 * np.arange(int(t60 * D.FS)) / D.FS / t60) * rs.standard_normal(int(t60 * D.FS)) * 0.3
    h[0] = 1.0
    L = 1 << (n + len(h) - 2).bit_length()
    return np.fft.irfft(np.fft.rfft(gate * rs.standard_normal(n), L) * np.fft.rfft(h, L), L)[:n].astype(np.float32)


def time_shape(lib, B, L, rounds):
    x = torch.from_numpy(np.stack([bursts(u, L) for u in range(B)])).cuda()
    st, dev = _lib.stream_ptr(), x.device
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    lo, hi, _ = D.bin_ranges(D.FS)
    NB, M = D.BANDS, D.frames_of(L)
    c_lo, c_hi = (_lib.C.c_int * NB)(*lo), (_lib.C.c_int * NB)(*hi)
    E, T = torch.empty(B, NB, M, dtype=torch.float64, device=dev), torch.empty(B, NB, M, dtype=torch.float64, device=dev)
    rl, frames = torch.empty(B, NB, M, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    out, counts = torch.empty(B, NB, 3, dtype=torch.float64, device=dev), torch.empty(B, NB, dtype=torch.int32, device=dev)

    def energies():
        _lib.check(lib.buddy_decay_energies(_lib.ptr(x), lens.data_ptr(), B, L, c_lo, c_hi, NB, E.data_ptr(), M, frames.data_ptr(), st))

    def regions():
        _lib.check(lib.buddy_decay_regions(E.data_ptr(), frames.data_ptr(), B, NB, M, D.K_SMOOTH, 6, 0.1, 1e-6, T.data_ptr(), rl.data_ptr(), st))

    def select():
        _lib.check(lib.buddy_decay_select(T.data_ptr(), frames.data_ptr(), B, NB, M, out.data_ptr(), counts.data_ptr(), st))

    def whole():
        D.decay_times(x, D.FS)

    res = {"batch": B, "length": L, "frames": M}
    for name, fn, n in (("decay_energies", energies, rounds), ("decay_regions", regions, rounds), ("decay_select", select, rounds), ("decay_times_whole_call", whole, 5)):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(n):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ts.append(t0.elapsed_time(t1))
        res[name] = [round(statistics.median(ts), 4), round(min(ts), 4)]
    res["regions_broadband"], res["t60_broadband"] = counts[:, 0].cpu().tolist(), [round(float(v), 4) for v in out[:, 0, 0].cpu()]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "decay_time.json"))
    a = ap.parse_args(argv)
    lib = _lib.require_gpu()
    res = {"fs": D.FS, "rounds": a.rounds, "unit": "ms per call, median (min)", "batch_8x64000": time_shape(lib, 8, 64000, a.rounds),
           "one_row_600s": time_shape(lib, 1, 600 * D.FS, a.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
