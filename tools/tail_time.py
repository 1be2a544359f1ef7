#!/usr/bin/env python
"""Time the hybrid room response (csrc/tail.hip after csrc/ism.hip) against the pure image-source call, with HIP events, and
tabulate what the tail does to the measured acoustics.  No target is attached.

  profiles/tail_time.json    eight drawn rooms x 1 s at 16 kHz in one call: ``rooms.shoebox_rir_hybrid`` (host work and transfers included: wall
                             clock around a synchronised call) against ``rooms.shoebox_rir``; the two tail kernels alone (HIP events); and one room
                             of nominal T60 = 3 s at 4.5 s, which the pure call refuses above ``max_images``
  profiles/tail_effect.txt   32 drawn rooms (``draw_rooms``, seed 0, response 1.5 x nominal): nominal T60 against EDT, T20, T30, C50 and DRR of the
                             pure response and of the hybrid one"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import acoustics, rng, rooms  # noqa: E402


def wall_ms(call, rounds):
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return [round(statistics.median(ts), 3), round(min(ts), 3)]


def event_ms(call, rounds):
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


def timing(a):
    lib = _lib.require_gpu()
    B, fs, n = a.batch, a.fs, int(round(a.seconds * a.fs))
    names = [f"room{b}" for b in range(B)]
    drawn, nominal = rooms._draw_rooms(names, a.seed, (0.2, 1.0), ((3, 8), (3, 8), (2.4, 3.5)), 0.5, 0.5, 343.0, 1000)
    keys = np.array([rng.stream_key(a.seed, v) for v in names], dtype=np.uint32)
    win = rooms.tail_window(drawn, fs, a.tail_ms, a.ramp)
    res = {"batch": B, "fs": fs, "samples": n, "tail_ms": a.tail_ms, "ramp": a.ramp, "rounds": a.rounds, "unit": "ms per call, median (min)",
           "tile": lib.buddy_tail_tile(), "ism_samples": int(win[:, 3].max()),
           "estimated_images_pure": float(f"{float(rooms.estimated_images(drawn, fs, n).sum()):.4g}"),
           "estimated_images_hybrid": float(f"{float(rooms.estimated_images(drawn, fs, int(win[:, 3].max())).sum()):.4g}")}
    res["shoebox_rir_wall"] = wall_ms(lambda: rooms.shoebox_rir(drawn, fs, n), a.rounds)
    res["shoebox_rir_hybrid_wall"] = wall_ms(lambda: rooms.shoebox_rir_hybrid(drawn, fs, n, nominal, keys, a.tail_ms, a.ramp), a.rounds)
    res["speedup_wall_at_median"] = round(res["shoebox_rir_wall"][0] / res["shoebox_rir_hybrid_wall"][0], 2)
    # the two tail kernels alone, on the image-source part of the same rooms
    ln = int(win[:, 3].max())
    u = rooms.shoebox_rir(drawn, fs, ln)[0]
    on = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    wt, dt, kt = on(win[:, 1:3].astype(np.int32)), on((3.0 * np.log(10.0) / nominal).reshape(B, 1)), on(keys.view(np.int32))
    amp, fl = torch.empty(B, 1, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    out = torch.empty(B, n, dtype=torch.float32, device="cuda")
    st = _lib.stream_ptr()
    res["tail_fit"] = event_ms(lambda: _lib.check(lib.buddy_tail_fit(u.data_ptr(), 0, B, 1, 1, ln, ln, ln, wt.data_ptr(), dt.data_ptr(), None, fs, amp.data_ptr(),
                                                                    fl.data_ptr(), st)), a.rounds)
    res["tail_mix"] = event_ms(lambda: _lib.check(lib.buddy_tail_mix(u.data_ptr(), 0, B, 1, 1, ln, ln, ln, wt.data_ptr(), a.ramp, dt.data_ptr(), amp.data_ptr(), None, 0,
                                                                    kt.data_ptr(), rooms.TAIL, fs, n, out.data_ptr(), n, n, st)), a.rounds)
    res["note"] = "both entries read their windows and decays back once to check them, which synchronises the stream: the event times include that"
    # the long room
    t60, nl = 3.0, int(round(4.5 * fs))
    rm = rooms.room_row((3.2, 3.5, 2.5), (1.0, 1.2, 1.3), (2.2, 2.6, 1.5), rooms.eyring_beta((3.2, 3.5, 2.5), t60))[None]
    kl = np.array([rng.stream_key(a.seed, "long")], dtype=np.uint32)
    res["long_room"] = {"nominal_t60": t60, "samples": nl, "estimated_images_pure": float(f"{float(rooms.estimated_images(rm, fs, nl)[0]):.4g}"),
                        "ism_samples": int(rooms.tail_window(rm, fs, a.tail_ms, a.ramp)[0, 3]),
                        "shoebox_rir_hybrid_wall": wall_ms(lambda: rooms.shoebox_rir_hybrid(rm, fs, nl, t60, kl, a.tail_ms, a.ramp), a.rounds)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def effect(a):
    fs = a.fs
    names = [f"room{b}" for b in range(32)]
    drawn, nominal = rooms._draw_rooms(names, 0, (0.2, 1.0), ((3, 8), (3, 8), (2.4, 3.5)), 0.5, 0.5, 343.0, 1000)
    cols = ("EDT", "T20", "T30", "C50", "DRR")
    lines = [f"# 32 rooms of draw_rooms (seed 0), fs {fs}, response 1.5 x nominal T60; pure image-source response | with --diffuse-tail "
             f"({a.tail_ms:g} ms, ramp {a.ramp}); times in s, C50 and DRR in dB",
             "room  T60   | " + " ".join(f"{c:>7}" for c in cols) + " | " + " ".join(f"{c:>7}" for c in cols)]
    vals = np.empty((32, 2, 5))
    for b, name in enumerate(names):
        n = int(round(1.5 * nominal[b] * fs))
        pure = rooms.shoebox_rir(drawn[b:b + 1], fs, n)[0]
        tail = rooms.shoebox_rir_hybrid(drawn[b:b + 1], fs, n, nominal[b], np.array([rng.stream_key(0, name)], dtype=np.uint32), a.tail_ms, a.ramp)[0]
        vals[b] = acoustics.rir_acoustics(torch.cat([pure, tail]), fs).values[:, 0, :5].numpy()
        lines.append(f"{b:4d}  {nominal[b]:.3f} | " + " ".join(f"{v:7.3f}" for v in vals[b, 0]) + " | " + " ".join(f"{v:7.3f}" for v in vals[b, 1]))
    rel = np.abs(vals[:, :, :3] / nominal[:, None, None] - 1.0)
    lines.append("# |T / T60 - 1|, median (max) over the rooms: " + "; ".join(
        f"{c} pure {np.median(rel[:, 0, q]):.3f} ({rel[:, 0, q].max():.3f}) tail {np.median(rel[:, 1, q]):.3f} ({rel[:, 1, q].max():.3f})" for q, c in enumerate(cols[:3])))
    d = vals[:, 1, 3:] - vals[:, 0, 3:]
    lines.append("# tail minus pure, median (min .. max) over the rooms: " + "; ".join(
        f"{c} {np.median(d[:, q]):+.2f} dB ({d[:, q].min():+.2f} .. {d[:, q].max():+.2f})" for q, c in enumerate(cols[3:])))
    with open(a.effect, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tail-ms", type=float, default=rooms.TAIL_MS)
    ap.add_argument("--ramp", type=int, default=rooms.TAIL_RAMP)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tail_time.json"))
    ap.add_argument("--effect", default=os.path.join(ROOT, "profiles", "tail_effect.txt"))
    a = ap.parse_args(argv)
    for p in (a.out, a.effect):
        os.makedirs(os.path.dirname(os.path.abspath(p)), exist_ok=True)
    timing(a)
    effect(a)


if __name__ == "__main__":
    main()
