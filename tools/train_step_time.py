"""Time one training step of the score network on one MI355X: EDM loss_fn + forward + parameter VJP + clip_grad_norm_ + Adam, at the reference's
training segment (conf/exp/VCTK_16k_4s_time.yaml: 65 536 samples) and batch B = 8, nf = 128 (conf/network/ncsnpp.yaml).

    python tools/train_step_time.py [--B 8] [--L 65536] [--steps 10] [--warmup 3] [--gemm f16x2] [--path torch|fused|both] [--rounds 3]
    python tools/train_step_time.py --stats kernel_stats.csv   # weight-gradient kernels' share and TFLOP/s from a rocprofv3 --stats run

The weight-gradient FLOPs of a step (2 M N K of every GEMM wgrad_kernel runs, from the grid of each layer) are printed so that the stats
summary can turn kernel time into TFLOP/s.  The figure is approximate: it counts useful FLOPs, not the padded tiles of the thin layers.
--path torch is torch's clip_grad_norm_ + Adam on the separate parameter tensors; --path fused is buddy_amd.training.fused.FusedAdam (two library calls
on flat buffers); --path both alternates the two in --rounds rounds in one process, each on its own network with the same weights, and also reports
for each the time from the end of the parameter VJP to the point where the next forward can start (optimizer + weight push), synchronised.
The time of one buddy_ncsnpp_update_params (the weight push after each optimizer step) is measured on its own.  Yardstick: the fp32 matrix peak, 64 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz = 157 TFLOP/s."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WGRAD_KERNELS = ("wgrad_kernel", "wgrad_reduce_kernel", "colsum_part_kernel", "colsum_final_kernel", "gn_pgrad_part_kernel",
                 "gn_pgrad_final_kernel", "linear_bwd_w_kernel", "linear_bwd_x_kernel")
PEAK = 64 * 1024 * 2.4e9


def wgrad_flops(net, B):
    """2 M N K of every weight gradient that wgrad_kernel computes: the 3x3 / 1x1 convolutions (input conv, ResBlocks, Combine, pyramid heads,
    output_layer) and the attention NINs, M = the pixels of the grid each GEMM runs on (a ResBlock's output grid; the input grid for the
    Conv_2 of an up block, which runs before its nearest upsample).  Dense / Linear layers (a few MFLOP) are left out."""
    specs = {n: s for n, s, *_ in net._specs}
    dims = {}

    def grid(idx):                      # B x the pixels of all_modules[idx]'s output; None: the module has no tap
        if idx not in dims:
            try:
                _, Hh, Ww, _ = net.tap(idx).shape
                dims[idx] = B * Hh * Ww
            except Exception:
                dims[idx] = None
        return dims[idx]
    flops = 0.0
    for name, shape in specs.items():
        if name.startswith("output_layer") and name.endswith("weight"):
            flops += 2.0 * grid(3) * shape[0] * shape[1]
            continue
        if not (name.endswith(".weight") or name.endswith(".W")) or len(shape) < 2 or "Dense_0" in name or name.split(".")[1] in ("1", "2"):
            continue
        idx = int(name.split(".")[1])
        M = grid(idx)
        if M is None:
            continue
        if name.endswith("Conv_2.weight") and grid(idx - 1) is not None and grid(idx - 1) < M:
            M = grid(idx - 1)           # an up block: Conv_2 runs at the input resolution
        flops += 2.0 * M * float(np.prod(shape))
    return flops


def summarise(path, flops):
    tot = wg = wg_gemm = 0.0
    with open(path) as f:
        for row in csv.DictReader(f):
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            tot += ns
            if any(k in row["Name"] for k in WGRAD_KERNELS):
                wg += ns
            if "wgrad_kernel" in row["Name"] and "reduce" not in row["Name"]:
                wg_gemm += ns
    out = {"kernel_ms_total": tot / 1e6, "param_grad_kernels_ms": wg / 1e6, "param_grad_share": wg / tot if tot else None,
           "wgrad_gemm_ms": wg_gemm / 1e6}
    if flops:
        out["wgrad_gemm_tflops"] = flops / (wg_gemm * 1e-9) / 1e12 if wg_gemm else None
        out["wgrad_gemm_fraction_of_fp32_peak"] = out["wgrad_gemm_tflops"] * 1e12 / PEAK if wg_gemm else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--L", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gemm", default=None)
    ap.add_argument("--nf", type=int, default=None, help="network width (default: conf/network/ncsnpp.yaml)")
    ap.add_argument("--path", default="torch", choices=("torch", "fused", "both"))
    ap.add_argument("--rounds", type=int, default=3, help="--path both: alternating rounds")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this tool: summarise it")
    ap.add_argument("--flops", type=float, default=0.0, help="weight-gradient FLOPs per step (printed by a timing run) for --stats")
    ap.add_argument("--stats-steps", type=int, default=1, help="training steps the profiled run executed (warmup included)")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(summarise(a.stats, a.flops * a.stats_steps)))
        return
    import torch
    from buddy_amd.config import load_yaml, CONF_DIR, AttrDict
    from buddy_amd.diff_params.edm import EDM
    from buddy_amd.networks.ncsnpp import NCSNppTime
    from buddy_amd.synth import synth_state_dict
    cfg = load_yaml(os.path.join(CONF_DIR, "network", "ncsnpp.yaml"))
    cfg.pop("_target_")
    cfg["gemm"] = a.gemm
    if a.nf:
        cfg["nf"] = a.nf
    cfg["stft"] = AttrDict(n_fft=cfg["stft"]["n_fft"], hop_length=cfg["stft"]["hop_length"], center=True)
    edm = EDM("ve_karras", SimpleNamespace(sigma_data=0.05, sigma_min=1e-5, sigma_max=10.0, rho=10.0))
    torch.manual_seed(0)
    x = 0.05 * torch.randn(a.B, a.L, device="cuda")

    def make(path):
        net = NCSNppTime(**cfg)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(0, net.nf, net.ch_mult, net.num_res_blocks).items()})
        net = net.cuda().requires_grad_(True)
        if path == "fused":
            from buddy_amd.training.fused import FusedAdam
            net.all_modules[0].W.requires_grad_(False)      # the Fourier projection gets no gradient: frozen range of the fused pass
            opt = FusedAdam(net.parameters(), lr=2e-4, network=net)
            update = lambda: opt.step(max_norm=1.0)
        else:
            opt = torch.optim.Adam(net.parameters(), lr=2e-4)

            def update():
                torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
                opt.step()

        def backward():
            loss, _ = edm.loss_fn(net, x)
            loss = loss.mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            return loss

        def step():
            loss = backward()
            update()
            return loss

        def window():
            """ms from the end of the parameter VJP until the next forward could start: optimizer + weight push, synchronised on both sides"""
            backward()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            update()
            net._sync_params(x.device)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        return net, step, window

    def timed(step, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / max(n, 1), loss

    if a.path == "both":
        legs = {p: make(p) for p in ("torch", "fused")}
        for p in legs:
            for _ in range(a.warmup):
                legs[p][1]()
        ms = {p: [] for p in legs}
        win = {p: [] for p in legs}
        for _ in range(a.rounds):
            for p in legs:
                ms[p].append(timed(legs[p][1], a.steps)[0])
                win[p].append(float(np.median([legs[p][2]() for _ in range(3)])))
        out = {"B": a.B, "L": a.L, "nf": legs["torch"][0].nf, "gemm": a.gemm or "default", "steps_per_round": a.steps, "rounds": a.rounds,
               "n_params": legs["torch"][0]._n_params}
        for p in legs:
            out[p] = {"ms_per_step_rounds": [round(v, 2) for v in ms[p]], "ms_per_step": round(float(np.median(ms[p])), 2),
                      "spread_ms": round(max(ms[p]) - min(ms[p]), 2), "vjp_end_to_next_forward_ms": round(float(np.median(win[p])), 2)}
        print(json.dumps(out))
        return
    net, step, window = make(a.path)
    for _ in range(a.warmup):
        step()
    ms, loss = timed(step, a.steps)
    flops = wgrad_flops(net, a.B)
    # the weight push of one optimizer step on its own (NCSNppTime._sync_params -> buddy_ncsnpp_update_params)
    upd = []
    for _ in range(5):
        with torch.no_grad():
            next(iter(net.parameters())).mul_(1.0)      # bumps a _version: the next sync pushes every weight
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        net._sync_params(x.device)
        torch.cuda.synchronize()
        upd.append((time.perf_counter() - t1) * 1e3)
    print(json.dumps({"B": a.B, "L": a.L, "nf": net.nf, "gemm": a.gemm or "default", "path": a.path, "steps": a.steps, "ms_per_step": round(ms, 2),
                      "loss": float(loss.detach()), "wgrad_flops_per_step": flops, "update_params_ms": round(float(np.median(upd)), 2),
                      "n_params": net._n_params}))


if __name__ == "__main__":
    main()
