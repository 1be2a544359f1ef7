#!/usr/bin/env python
"""Time the kernel groups of the evaluation metrics (csrc/metrics.hip) with HIP events at B = 8 x 64 000 samples, 16 kHz: the median of `--rounds`
timed calls per group after warm-up, written as one JSON object (default profiles/metrics_time.json).  Each C entry includes its own copy of the
row lengths to the host (a stream synchronise), so these are times per call as the tester pays them, not kernel times.  No target is attached."""
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
from buddy_amd.utils import metrics as M, resample as RS  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--length", type=int, default=64000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "metrics_time.json"))
    a = ap.parse_args(argv)
    lib = _lib.require_gpu()
    B, L, fs = a.batch, a.length, 16000
    from scipy import signal
    xs = np.stack([synth_clean(u, L) for u in range(B)])
    es = np.stack([signal.fftconvolve(xs[u], synth_rir(u, 4000))[:L].astype(np.float32) for u in range(B)])
    x, e = torch.from_numpy(xs).cuda(), torch.from_numpy(es).cuda()
    st = _lib.stream_ptr()
    dev = x.device
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    mom, fl = torch.empty(B, 4, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    x10, e10 = RS.resample(x, fs, 10000), RS.resample(e, fs, 10000)
    L10 = x10.shape[1]
    lens10 = torch.full((B,), L10, dtype=torch.int32, device=dev)
    F = M.frames_of(L10)
    ldo = (F - 1) * M.HOP + M.FRAME
    xo, eo = torch.empty(B, ldo, device=dev), torch.empty(B, ldo, device=dev)
    lens_o, K, Fd = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    src = torch.empty(B, F, dtype=torch.int32, device=dev)
    ws = torch.empty(B * max(F, M.frames_of(L)), dtype=torch.float64, device=dev)
    bands = M.third_octave_bands()
    J = len(bands)
    lo, hi = (_lib.C.c_int * J)(*[b[0] for b in bands]), (_lib.C.c_int * J)(*[b[1] for b in bands])
    X, Y = torch.empty(B, J, F, device=dev), torch.empty(B, J, F, device=dev)
    sc = torch.empty(B, 2, dtype=torch.float64, device=dev)
    ws2 = torch.empty(lib.buddy_stoi_scores_workspace(B, F) // 8, dtype=torch.float64, device=dev)
    mean_p, lsd = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)

    def moments():
        _lib.check(lib.buddy_pair_moments(_lib.ptr(e), _lib.ptr(x), lens.data_ptr(), B, L, mom.data_ptr(), fl.data_ptr(), st))

    def resample():
        RS.resample(x, fs, 10000), RS.resample(e, fs, 10000)

    def select():
        _lib.check(lib.buddy_stoi_select(_lib.ptr(x10), _lib.ptr(e10), lens10.data_ptr(), B, L10, _lib.ptr(xo), _lib.ptr(eo), ldo, lens_o.data_ptr(), K.data_ptr(),
                                         Fd.data_ptr(), src.data_ptr(), F, ws.data_ptr(), ws.numel() * 8, st))

    def spectra():
        _lib.check(lib.buddy_band_spectra(_lib.ptr(xo), lens_o.data_ptr(), B, ldo, lo, hi, J, _lib.ptr(X), F, st))
        _lib.check(lib.buddy_band_spectra(_lib.ptr(eo), lens_o.data_ptr(), B, ldo, lo, hi, J, _lib.ptr(Y), F, st))

    def scores():
        _lib.check(lib.buddy_stoi_scores(_lib.ptr(X), _lib.ptr(Y), K.data_ptr(), B, J, F, sc.data_ptr(), fl.data_ptr(), ws2.data_ptr(), ws2.numel() * 8, st))

    def lsd_group():
        _lib.check(lib.buddy_frame_power(_lib.ptr(x), lens.data_ptr(), B, L, mean_p.data_ptr(), ws.data_ptr(), ws.numel() * 8, st))
        gain = torch.where(mom[:, 0] > 0, torch.sqrt(mom[:, 1] / mom[:, 0]), torch.ones_like(mom[:, 0])).contiguous()
        delta = (1e-8 * mean_p).contiguous()
        _lib.check(lib.buddy_lsd(_lib.ptr(e), _lib.ptr(x), lens.data_ptr(), B, L, gain.data_ptr(), delta.data_ptr(), lsd.data_ptr(), fl.data_ptr(), ws.data_ptr(),
                                 ws.numel() * 8, st))

    res = {"batch": B, "length": L, "fs": fs, "rounds": a.rounds, "unit": "ms per call, median (min)"}
    for name, fn in (("pair_moments", moments), ("resample_to_10k_x2", resample), ("stoi_select", select), ("band_spectra_x2", spectra),
                     ("stoi_scores", scores), ("frame_power_and_lsd", lsd_group)):
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
        M.evaluate(e, x, fs)
        t1.record()
        torch.cuda.synchronize()
        whole.append(t0.elapsed_time(t1))
    res["evaluate_whole_call"] = [round(statistics.median(whole), 4), round(min(whole), 4)]
    res["kept_frames"], res["frames"] = K.cpu().tolist(), Fd.cpu().tolist()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
