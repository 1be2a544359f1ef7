"""Step time of the blind sampler with the default noise source (torch's generators: host draw, pinned copy on a side stream) against
`tester.noise.generator=philox` (drawn on the GPU, fused into the perturbation), at the headline shape B = 8 x 64 000, in alternating rounds in ONE
process (two stacks on the same prepared weights).  Two figures per round and source:

  step_ms  wall time per step, host clock around `steps` steps ending in a device synchronise
  host_ms  time the Python thread spends inside those step() calls before the synchronise: what the host pays to enqueue a step (the host runs
           ahead of the GPU, so this is below step_ms; it is the figure the noise source changes)

    python tools/seeded_step_time.py --out profiles/seeded_step_time.json
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--length", type=int, default=64000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bench import StepRunner
    from buddy_amd import _lib
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.synth import synth_clean, synth_rir, synth_state_dict
    from buddy_amd.testing.tester import Tester
    _lib.require_gpu()
    device = torch.device("cuda", 0)
    B, L = a.batch, a.length
    items = [(synth_clean(u, L), synth_rir(u, 8000), f"utt{u}.wav") for u in range(B)]
    base = None
    runners = {}
    for gen in ("torch", "philox"):
        args = compose(overrides=[f"tester.sampling_params.T={a.T}", "tester.posterior_sampling.warm_initialization.mode=reverb_scaled",
                                  f"tester.noise.generator={gen}", "+tester.sub_batches=1"])
        if base is None:
            base = instantiate(args.network)
            base.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(0, args.network.nf).items()})
            base = base.to(device).eval()
            net = base
        else:
            net = base.replica()
        t = Tester(args, net, instantiate(args.diff_params), test_set=None, device=device, in_training=True)
        torch.manual_seed(1234)
        noise = t.noise_factory([it[2] for it in items]) if gen == "philox" else None
        t.sampler.noise = noise
        _, y, op, _ = t.prepare_batch(items, blind=True, noise=noise)
        runners[gen] = StepRunner(t, y, op, device, blind=True)
    for r in runners.values():
        for _ in range(a.warmup):
            r.step()
    torch.cuda.synchronize()
    rows = []
    for rnd in range(a.rounds):
        for gen in ("torch", "philox") if rnd % 2 == 0 else ("philox", "torch"):
            r = runners[gen]
            r.step(); torch.cuda.synchronize()          # same starting condition for both: an empty queue after one step of this stack
            t0 = time.perf_counter()
            for _ in range(a.steps):
                r.step()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert torch.isfinite(r.x).all()
            rows.append(dict(round=rnd, generator=gen, step_ms=(t2 - t0) / a.steps * 1e3, host_ms=(t1 - t0) / a.steps * 1e3))
            print(f"round {rnd} {gen:6s} step {rows[-1]['step_ms']:.2f} ms, host {rows[-1]['host_ms']:.2f} ms", file=sys.stderr)
    res = dict(batch=B, length=L, T=a.T, steps=a.steps, warmup=a.warmup, rounds=rows)
    for gen in ("torch", "philox"):
        for k in ("step_ms", "host_ms"):
            v = sorted(r[k] for r in rows if r["generator"] == gen)
            res[f"{gen}_{k}"] = dict(min=v[0], median=0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2]), max=v[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
