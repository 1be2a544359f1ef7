"""Blind DPS sampler step time (network fwd + VJP, likelihood, optimize_op, update) at B = 8 x 64 000 samples with the default losses, with a
non-default STFT loss family and with time-domain losses -- the cost of the loss kinds outside the default kernels.
usage: python tools/loss_step_time.py [steps] [warmup]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

PS = "tester.posterior_sampling"
CONFIGS = {
    "default": [],
    "stft": [f"{PS}.rec_loss.name=l2_stft_mag_sum", f"+{PS}.rec_loss.freq_weighting=sqrt", f"{PS}.rec_loss_params.name=l2_log_stft_sum",
             f"{PS}.RIR_noise_regularization.loss.name=l2_stft_sum"],
    "time": [f"{PS}.rec_loss.name=l2_sum", f"{PS}.rec_loss_params.name=l2_mean", f"{PS}.RIR_noise_regularization.loss.name=l2_sum"],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=20)
    ap.add_argument("warmup", nargs="?", type=int, default=3)
    a = ap.parse_args()
    ns = argparse.Namespace(T=201, length=64000, attention=None, gemm=None)
    net, out = None, {}
    for rnd in range(2):                    # two interleaved rounds: drift of the box shows as a spread between them
        for name, extra in CONFIGS.items():
            _, net, _, tester, _, y, op = bench.build_stack(ns, "cuda", 8, 0, net=net, extra=extra)
            run = bench.StepRunner(tester, y, op, "cuda")
            for _ in range(a.warmup):
                run.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                run.step()
            torch.cuda.synchronize()
            out.setdefault(name, []).append((time.perf_counter() - t0) / a.steps * 1e3)
    best = {k: min(v) for k, v in out.items()}
    print(json.dumps({"ms_per_step": {k: [round(x, 3) for x in v] for k, v in out.items()},
                      "vs_default": {k: round(best[k] / best["default"] - 1.0, 4) for k in best}}))


if __name__ == "__main__":
    main()
