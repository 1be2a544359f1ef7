"""Speed of gemm = "f16" (the opt-in fast mode of the Winograd-domain GEMMs) against the default f16x2, on the headline workload:
blind DPS, B = 8 x 64000 samples, T = 50 schedule, the shipped operator updates per step, synthetic seeded data (bench.py's build_stack / StepRunner).
Two handles on the same prepared weights in one process (the f16 one a replica with gemm = 3), timed alternately with device events after a warm-up.
Timing only: the two legs draw their injected noise in turn, so their outputs are not comparable.  The end result of the mode (whole chains, both
arithmetics on the same noise streams) is gated by tests/test_hip_gemm_f16.py (informed and blind chains against the default).
usage: python tools/gemm_f16_leg.py [--rounds 3] [--steps 10] [--warmup 3] [--out profiles/r07_gemm_f16_leg.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternations f16x2 / f16 (at least 3 for the record)")
    ap.add_argument("--steps", type=int, default=10, help="timed sampler steps per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--length", type=int, default=64000)
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--out", default=None, help="JSON file to write (e.g. profiles/r07_gemm_f16_leg.json)")
    a = ap.parse_args()
    ns = argparse.Namespace(T=a.T, length=a.length, attention=None, gemm=None)
    device = "cuda:0"
    _, net, _, tester, _, y, op = bench.build_stack(ns, device, a.batch, 0)
    _, net16, _, tester16, _, y16, op16 = bench.build_stack(ns, device, a.batch, 0, net)
    net16.set_option("gemm", 3)
    legs = {"f16x2": bench.StepRunner(tester, y, op, device), "f16": bench.StepRunner(tester16, y16, op16, device)}
    for _ in range(a.warmup):
        for r in legs.values():
            r.step()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, r in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                r.step()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {
        "what": f"blind DPS, B = {a.batch} x {a.length}, T = {a.T} schedule, shipped operator updates per step; two handles on shared weights (f16x2 default, "
                f"f16 = replica with gemm = 3), {a.rounds} alternating rounds of {a.steps} steps each after {a.warmup} warm-up steps per leg; HIP events",
        "ms_per_step": {k: v for k, v in ms.items()},
        "ms_per_step_median": med,
        "spread_pct": {k: 100.0 * (max(v) - min(v)) / statistics.median(v) for k, v in ms.items()},
        "speedup_f16_vs_f16x2": med["f16x2"] / med["f16"],
        "time": time.strftime("%Y-%m-%d %H:%M:%S"),
    }
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
