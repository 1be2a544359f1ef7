#!/usr/bin/env python3
"""Training counterpart of test.py, with the command-line shape of the reference's train.py:

    python train.py --config-name=conf_VCTK.yaml model_dir=experiments/run dset.train.path=<VCTK/wav16> exp.batch_size=8 \\
        exp.optimizer.lr=1e-4 logging.save_interval=10000 +exp.max_iters=100000

without Hydra: `group=name` picks conf/<group>/<name>.yaml (tester, network, diff_params, exp, dset, logging), `a.b.c=value` overrides a
key.  The loss, the forward, every gradient and the optimizer step run in HIP on one MI355X (buddy_amd/training/); there is no CPU path."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from buddy_amd.config import compose_train  # noqa: E402
from buddy_amd.instantiate import instantiate  # noqa: E402
from buddy_amd.testing.tester import Tester  # noqa: E402

GROUPS = ("tester", "network", "diff_params", "exp", "dset", "logging")


def parse(argv):
    groups, overrides = {}, []
    for a in argv:
        if a.startswith("--config-name") or a.startswith("--config-path"):
            continue
        if "=" not in a:
            raise SystemExit(f"unrecognised argument {a!r}")
        k, v = a.split("=", 1)
        if k in GROUPS:
            groups[k] = v
        else:
            overrides.append(a)
    return groups, overrides


def _seed_worker(worker_id):
    import random
    import numpy as np
    seed = (torch.initial_seed() + worker_id) % 2 ** 32       # every loader worker draws its own files and offsets
    random.seed(seed)
    np.random.seed(seed)


def _main(args):
    if not torch.cuda.is_available():
        raise SystemExit("train.py needs an MI355X (no CPU fallback)")
    device = torch.device("cuda", int(args.get("gpu", 0)))
    torch.cuda.set_device(device)
    if not os.path.isabs(str(args.model_dir)):
        args.model_dir = os.path.join(ROOT, str(args.model_dir))
    os.makedirs(args.model_dir, exist_ok=True)
    args.exp.model_dir = args.model_dir

    train_set = instantiate(args.dset.train)
    nw = int(args.exp.num_workers)
    loader = torch.utils.data.DataLoader(train_set, batch_size=int(args.exp.batch_size), num_workers=nw, pin_memory=True,
                                         worker_init_fn=_seed_worker, prefetch_factor=20 if nw > 0 else None)
    test_set = instantiate(args.dset.test) if args.dset.test.get("path", None) and os.path.isdir(str(args.dset.test.path)) else None
    diff_params = instantiate(args.diff_params)
    network = instantiate(args.network).to(device)
    args.tester.sampling_params.same_as_training = True
    tester = Tester(args, network, diff_params, test_set=test_set, device=device, in_training=True)
    trainer = instantiate(args.exp.trainer, args, iter(loader), network, diff_params, tester, device)

    print()
    print("Training options:")
    print()
    print(f"Output directory:        {args.model_dir}")
    print(f"Network architecture:    {args.network._target_}")
    print(f"Dataset:    {args.dset.train._target_}")
    print(f"Diffusion parameterization:  {args.diff_params._target_}")
    print(f"Batch size:              {args.exp.batch_size}")
    print()
    trainer.training_loop()


def main(argv=None):
    groups, overrides = parse(sys.argv[1:] if argv is None else argv)
    args = compose_train(tester=groups.get("tester", "only_unconditional"), network=groups.get("network", "ncsnpp"),
                         diff_params=groups.get("diff_params", "edm_VCTK"), exp=groups.get("exp", "VCTK_16k_4s_time"),
                         dset=groups.get("dset", "vctk_16k_4s"), logging=groups.get("logging", "base_logging"), overrides=overrides)
    _main(args)


if __name__ == "__main__":
    main()
