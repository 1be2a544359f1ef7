#!/usr/bin/env python3
"""Training counterpart of test.py, with the command-line shape of the reference's train.py:

    python train.py --config-name=conf_VCTK.yaml model_dir=experiments/run dset.train.path=<VCTK/wav16> exp.batch_size=8 \\
        exp.optimizer.lr=1e-4 logging.save_interval=10000 +exp.max_iters=100000

without Hydra: `group=name` picks conf/<group>/<name>.yaml (tester, network, diff_params, exp, dset, logging), `a.b.c=value` overrides a
key.  The loss, the forward, every gradient and the optimizer step run in HIP on the MI355X (buddy_amd/training/); there is no CPU path.

Data-parallel: `+exp.gpus=N [+exp.backend=nccl|gloo]` starts N rank processes of this script (buddy_amd.dist.launch: fresh children, the
launching process never opens a GPU) and returns the first non-zero exit status; a torchrun-style launcher that sets RANK / WORLD_SIZE /
LOCAL_RANK works as well.  exp.batch_size stays the global batch; nccl (RCCL) wants one GPU per rank, gloo lets ranks share one for smoke
tests.  At most 16 ranks."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from buddy_amd import dist as bdist  # noqa: E402
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


def _rank_setup(args):
    """the device of this process and, in a job of several ranks, its placement and process group; returns (device, rank, world)"""
    rank, local_rank, world = bdist.env_rank_world()
    if world == 1:
        return torch.device("cuda", int(args.get("gpu", 0))), 0, 1
    backend = str(args.exp.get("backend", "nccl"))
    gpus = args.exp.get("gpus", None)
    if gpus is not None and int(gpus) != world:
        raise SystemExit(f"train.py: exp.gpus={gpus} but WORLD_SIZE={world}: launch one rank per GPU (python train.py +exp.gpus=N does it itself)")
    if world > bdist.MAX_RANKS:
        raise SystemExit(f"train.py: {world} ranks asked for, one node runs 1 to {bdist.MAX_RANKS}")
    if backend == "nccl" and world > torch.cuda.device_count():
        raise SystemExit(bdist.too_few_devices_message("train.py", world, torch.cuda.device_count()))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
    bdist.pin_rank(local_rank, local_world, torch.cuda.device_count())
    device = torch.device("cuda", bdist.device_index(local_rank))
    torch.cuda.set_device(device)
    bdist.rccl_env_defaults(log=(lambda m: print(m, file=sys.stderr)) if rank == 0 else None)
    bdist.init(backend=backend, device=device)
    return device, rank, world


def _main(args):
    if not torch.cuda.is_available():
        raise SystemExit("train.py needs an MI355X (no CPU fallback)")
    device, rank, world = _rank_setup(args)
    torch.cuda.set_device(device)
    if int(args.exp.batch_size) % world != 0:
        raise SystemExit(f"train.py: exp.batch_size={int(args.exp.batch_size)} is the global batch and must be a multiple of the {world} ranks")
    if not os.path.isabs(str(args.model_dir)):
        args.model_dir = os.path.join(ROOT, str(args.model_dir))
    os.makedirs(args.model_dir, exist_ok=True)
    args.exp.model_dir = args.model_dir

    if rank > 0:        # rank 0 draws what the single-process run draws; every other rank has its own files, offsets, sigmas and noise
        args.dset.train.seed = bdist.rank_seed(args.dset.train.get("seed", 0), rank)
    train_set = instantiate(args.dset.train)
    nw = int(args.exp.num_workers)
    gen = torch.Generator().manual_seed(bdist.rank_seed(args.exp.seed, rank)) if rank > 0 else None      # the base seed of the loader's workers
    loader = torch.utils.data.DataLoader(train_set, batch_size=int(args.exp.batch_size) // world, num_workers=nw, pin_memory=True,
                                         worker_init_fn=_seed_worker, prefetch_factor=20 if nw > 0 else None, generator=gen)
    test_set = instantiate(args.dset.test) if args.dset.test.get("path", None) and os.path.isdir(str(args.dset.test.path)) else None
    diff_params = instantiate(args.diff_params)
    network = instantiate(args.network).to(device)
    args.tester.sampling_params.same_as_training = True
    tester = Tester(args, network, diff_params, test_set=test_set, device=device, in_training=True)
    trainer = instantiate(args.exp.trainer, args, iter(loader), network, diff_params, tester, device)

    if rank == 0:
        print()
        print("Training options:")
        print()
        print(f"Output directory:        {args.model_dir}")
        print(f"Network architecture:    {args.network._target_}")
        print(f"Dataset:    {args.dset.train._target_}")
        print(f"Diffusion parameterization:  {args.diff_params._target_}")
        print(f"Batch size:              {args.exp.batch_size}" + (f" over {world} ranks" if world > 1 else ""))
        print()
    trainer.training_loop()
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def main(argv=None):
    groups, overrides = parse(sys.argv[1:] if argv is None else argv)
    args = compose_train(tester=groups.get("tester", "only_unconditional"), network=groups.get("network", "ncsnpp"),
                         diff_params=groups.get("diff_params", "edm_VCTK"), exp=groups.get("exp", "VCTK_16k_4s_time"),
                         dset=groups.get("dset", "vctk_16k_4s"), logging=groups.get("logging", "base_logging"), overrides=overrides)
    gpus = int(args.exp.get("gpus", 1) or 1)
    if gpus > 1 and "WORLD_SIZE" not in os.environ:
        # become the launcher: one fresh rank process per GPU with the same arguments; this process never opens a GPU
        try:
            raise SystemExit(bdist.launch(os.path.abspath(__file__), sys.argv[1:] if argv is None else argv, gpus, str(args.exp.get("backend", "nccl"))))
        except ValueError as e:
            raise SystemExit(str(e))
    _main(args)


if __name__ == "__main__":
    main()
