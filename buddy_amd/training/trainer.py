"""``Trainer`` -- same surface as the reference's ``training/trainer.py:21-336``: constructor ``(args, dset, network, diff_params, tester,
device)``, ``train_step``, ``update_ema``, ``training_loop``, ``state_dict`` / ``load_state_dict``, ``save_checkpoint``,
``resume_from_checkpoint``, ``get_batch``, ``heavy_logging``; checkpoints ``<model_dir>/<exp_name>-<it>.pt`` with the keys
``it, network, optimizer, ema, args``.

What differs is where the work runs.  The loss, the forward and every gradient are the HIP network's; clipping, the Adam update and the EMA
are ONE fused pass over flat buffers (``training/fused.py``), so between the end of the parameter VJP and the next forward the number of
launches does not depend on the number of parameter tensors.  ``train_step`` therefore already applies the EMA of its iteration, and the
``update_ema()`` that ``training_loop`` calls next (the reference's order) finds it done; ``update_ema()`` called on its own is one
EMA-only launch.

Logging: wandb, the torch profiler and the plots are not part of this package.  With ``args.logging.log`` the mean loss and the
per-sigma-bin errors (``process_loss_for_logging``) are appended as JSON lines to ``<model_dir>/train_log.jsonl`` every ``log_interval``
iterations.  The yaml keys ``lr_rampup_it``, ``scheduler_step_size`` and ``scheduler_gamma`` of the reference are read by nothing there and
by nothing here: the learning rate is constant.

Data parallelism: when ``torch.distributed`` is initialised (more than one rank, or a one-rank group forced for tests) the Trainer is one of W
replicas.  ``exp.batch_size`` stays the GLOBAL batch and every rank's loader yields ``batch_size // W`` utterances; the gradients are summed by
one all-reduce on the flat buffer and averaged inside the fused optimizer pass (``FusedAdam.attach_group``), so the step is the single-process
step on the global batch up to the rounding of that sum.  The replicas are made equal by a broadcast from rank 0 after construction and after
every resume, and are proved equal (``FusedAdam.check_replicas``: checksums of the weights, both moments and the EMA) then, before every
checkpoint, after every heavy log and every ``exp.replica_check_interval`` iterations (default: ``logging.log_interval``; 0: never).  Rank r
seeds its streams with ``dist.rank_seed(exp.seed, r)``; rank 0 writes the checkpoints (same keys, same name: a checkpoint of one world size
resumes at any other) and the logs, the latter from the per-utterance errors of the global batch.  Without a process group nothing of this
runs: same launches, same bits as before."""
from __future__ import annotations

import copy
import json
import os
import re
from glob import glob

import numpy as np
import torch

from .. import dist as bdist
from ..utils import training_utils as t_utils
from .fused import FusedAdam


def ema_factor(it, batch_size, ema_rampup, ema_rate):
    """The factor s of ``ema = ema * s + network * (1 - s)`` at iteration ``it`` (reference trainer.py:245-258):
    t = it * batch_size; clip(t / ema_rampup, 0, ema_rate) while t < ema_rampup, ema_rate from then on."""
    t = it * batch_size
    if t < ema_rampup:
        return float(np.clip(t / ema_rampup, 0.0, ema_rate))
    return float(ema_rate)


def make_optimizer(cfg, network):
    """The optimizer of ``args.exp.optimizer``.  The reference's yaml names torch's Adam as ``_target_``; the target is resolved by its last
    component, and Adam with default options is the fused HIP optimizer.  Anything else is refused: there is no per-tensor fallback."""
    kind = str(cfg["_target_"]).rpartition(".")[2]
    if kind not in ("Adam", "FusedAdam"):
        raise NotImplementedError(f"optimizer {cfg['_target_']!r}: the MI355X training loop has the fused Adam only")
    kw = {k: v for k, v in cfg.items() if k != "_target_"}
    unknown = sorted(set(kw) - {"lr", "betas", "eps"})
    if unknown:
        raise NotImplementedError(f"optimizer options {unknown} are not supported (lr, betas, eps)")
    if "betas" in kw:
        kw["betas"] = tuple(float(b) for b in kw["betas"])
    return FusedAdam(network.parameters(), network=network, **kw)


class Trainer:
    def __init__(self, args=None, dset=None, network=None, diff_params=None, tester=None, device="cpu"):
        assert args is not None, "args dictionary is None"
        assert dset is not None, "dset is None"
        assert network is not None, "network is None"
        assert diff_params is not None, "diff_params is None"
        assert device is not None, "device is None"
        self.args, self.dset, self.network, self.diff_params, self.device, self.tester = args, dset, network, diff_params, device, tester
        if self.tester is not None:
            self.tester.use_wandb = False
        if not any(p.requires_grad for p in network.parameters()):
            # NCSNppTime registers its parameters frozen (the sampler's default); the reference's are trainable except the Fourier W
            for (name, _, kind, _), p in zip(network._specs, network._params()):
                p.requires_grad_(kind != "fourier")
        self.world, self.rank, self._dp, self._constructed = 1, 0, False, False
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.world, self.rank, self._dp = torch.distributed.get_world_size(), torch.distributed.get_rank(), True
            if int(args.exp.batch_size) % self.world != 0:
                raise ValueError(f"exp.batch_size = {int(args.exp.batch_size)} is the global batch and must be a multiple of the {self.world} ranks")
        self.optimizer = make_optimizer(args.exp.optimizer, network)
        self.ema = copy.deepcopy(self.network).eval().requires_grad_(False)
        self.optimizer.attach_ema(self.ema)
        if self._dp:
            self.optimizer.attach_group(None, self.world, self.rank)
        torch.manual_seed(bdist.rank_seed(self.args.exp.seed, self.rank))
        self.total_params = sum(p.numel() for p in self.network.parameters() if p.requires_grad)
        print("total_params: ", self.total_params / 1e6, "M")
        self._ema_done_it = None        # the iteration whose EMA train_step has already applied
        self._log_rows = []

        self.latest_checkpoint = None
        resuming = False
        if self.args.exp.resume:
            ckpt = self.args.exp.get("resume_checkpoint", None)
            if ckpt not in (None, "None"):
                resuming = self.resume_from_checkpoint(checkpoint_path=ckpt)
            else:
                resuming = self.resume_from_checkpoint()
            if not resuming:
                print("Could not resume from checkpoint")
                print("training from scratch")
            else:
                print("Resuming from iteration {}".format(self.it))
        if not resuming:
            self.it = 0
            self.latest_checkpoint = None
            if tester is not None:
                self.tester.it = 0
        if self._dp:
            self.sync_replicas()
        self._constructed = True
        if self.args.logging.log:
            self.setup_logging_variables()

    # ---- data parallelism ---------------------------------------------------------------------------------------------------------
    def sync_replicas(self):
        """Every rank continues from rank 0's state -- weights, moments, EMA, step counters, iteration -- whatever each of them loaded, and
        the replicas are checked to be equal"""
        self.optimizer.broadcast_state(0)
        self.it = self.optimizer.broadcast_int(self.it, 0)
        if self.tester is not None:
            self.tester.it = self.it
        self.optimizer.check_replicas()

    def _replica_check_interval(self):
        v = self.args.exp.get("replica_check_interval", None)
        return int(self.args.logging.log_interval if v in (None, "None") else v)

    def setup_logging_variables(self):
        hp = self.args.diff_params.sde_hp
        self.sigma_bins = np.logspace(np.log10(hp.sigma_min), np.log10(hp.sigma_max), num=self.args.logging.num_sigma_bins, base=10)

    # ---- checkpoints --------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        return t_utils.load_state_dict(state_dict, network=self.network, ema=self.ema, optimizer=self.optimizer)

    def resume_from_checkpoint(self, checkpoint_path=None, checkpoint_id=None):
        """reference :110-169: an explicit path (as given, then under model_dir), else the newest ``<exp_name>-<it>.pt`` of model_dir.
        Data-parallel: every rank loads the file itself where it can see it, then all take rank 0's state (the construction does so itself;
        a call made later is followed by ``sync_replicas()`` here)."""
        ok = self._resume_from_checkpoint(checkpoint_path, checkpoint_id)
        if self._dp and self._constructed:
            self.sync_replicas()
        return ok

    def _resume_from_checkpoint(self, checkpoint_path=None, checkpoint_id=None):
        if checkpoint_path is not None:
            for path in (checkpoint_path, os.path.join(self.args.model_dir, checkpoint_path)):
                try:
                    checkpoint = torch.load(path, map_location=self.device, weights_only=False)
                    self.it = int(checkpoint.get("it", 0)) if isinstance(checkpoint, dict) else 0
                    return self.load_state_dict(checkpoint)
                except Exception as e:
                    print("Could not resume from checkpoint")
                    print(e)
                    self.it = 0
            print("training from scratch")
            return False
        try:
            if checkpoint_id is None:
                rx = re.compile(f"{re.escape(self.args.exp.exp_name)}-(\\d*)\\.pt")
                ids = [int(rx.search(w).groups()[0]) for w in glob(f"{self.args.model_dir}/{self.args.exp.exp_name}-*.pt")]
                checkpoint_id = max(ids)
            checkpoint = torch.load(f"{self.args.model_dir}/{self.args.exp.exp_name}-{checkpoint_id}.pt", map_location=self.device,
                                    weights_only=False)
            self.it = int(checkpoint.get("it", 0))
            self.load_state_dict(checkpoint)
            return True
        except Exception as e:
            print(e)
            return False

    def state_dict(self):
        return {"it": self.it, "network": self.network.state_dict(), "optimizer": self.optimizer.state_dict(), "ema": self.ema.state_dict(),
                "args": self.args}

    def save_checkpoint(self):
        """Data-parallel: the replicas are checked, rank 0 writes the one file, and every rank waits until it is there"""
        save_name = f"{self.args.model_dir}/{self.args.exp.exp_name}-{self.it}.pt"
        if self._dp:
            self.optimizer.check_replicas()
            try:
                if self.rank == 0:
                    self._write_checkpoint(save_name)
            finally:
                torch.distributed.barrier()
            self.latest_checkpoint = save_name
            return
        self._write_checkpoint(save_name)

    def _write_checkpoint(self, save_name):
        os.makedirs(self.args.model_dir, exist_ok=True)
        torch.save(self.state_dict(), save_name)
        print("saving", save_name)
        if self.args.logging.get("remove_old_checkpoints", False) and self.latest_checkpoint is not None:
            try:
                os.remove(self.latest_checkpoint)
                print("removed last checkpoint", self.latest_checkpoint)
            except OSError:
                print("could not remove last checkpoint", self.latest_checkpoint)
        self.latest_checkpoint = save_name

    # ---- logging ------------------------------------------------------------------------------------------------------------------
    def process_loss_for_logging(self, error, sigma):
        """mean loss and, per logarithmic sigma bin, the mean error of the first batch row that falls into it (reference :194-218)"""
        if self._dp:
            # the global batch: per-utterance mean errors and sigmas of every rank, in rank order (equal shares: the mean of the row means is
            # the global mean); every rank enters the gather, rank 0 keeps the row
            error, sigma = self.optimizer.gather_floats(torch.stack([error.detach().mean(dim=tuple(range(1, error.dim()))).float(),
                                                                     sigma.detach().reshape(-1).float()]))
            error = error[:, None]
            if self.rank != 0:
                return
        error = error.detach().cpu().numpy()
        sigma = sigma.detach().cpu().reshape(-1).numpy()
        row = {"it": int(self.it), "loss": float(error.mean())}
        for i, edge in enumerate(self.sigma_bins):
            mask = sigma <= edge if i == 0 else (sigma <= edge) & (sigma > self.sigma_bins[i - 1])
            if mask.sum() > 0:
                row["error_sigma_" + str(edge)] = float(error[np.where(mask)[0][0]].mean())
        self._log_rows.append(row)

    def easy_logging(self):
        """append the rows collected since the last call, and their mean loss, to <model_dir>/train_log.jsonl"""
        if not self._log_rows:
            return
        os.makedirs(self.args.model_dir, exist_ok=True)
        with open(os.path.join(self.args.model_dir, "train_log.jsonl"), "a") as f:
            for row in self._log_rows:
                f.write(json.dumps(row) + "\n")
            f.write(json.dumps({"it": int(self.it), "loss_mean": float(np.mean([r["loss"] for r in self._log_rows]))}) + "\n")
        self._log_rows = []

    def heavy_logging(self):
        """``tester.do_test`` on the latest checkpoint.  As in the reference, ``train.py`` gives Tester and Trainer the SAME network object, and
        ``Tester.load_checkpoint`` loads the EMA weights into it: every heavy log replaces the training weights by the EMA of the last saved
        checkpoint (in place, through the flat buffer; the handle is rebuilt).  Give the Tester a deep copy to keep the two apart.
        Data-parallel: the Tester runs on rank 0 only; afterwards every rank takes rank 0's weights, so all continue from the same ones --
        the EMA of the last checkpoint, as the single-process run does -- and the replicas are checked."""
        out = None
        if self.tester is not None and self.rank == 0:
            if self.latest_checkpoint is not None:
                self.tester.load_checkpoint(self.latest_checkpoint)
            out = self.tester.do_test(it=self.it)
        if self._dp:
            self.optimizer.broadcast_state(0, weights_only=True)
            self.optimizer.check_replicas()
        return out

    # ---- the step -----------------------------------------------------------------------------------------------------------------
    def get_batch(self):
        sample = next(self.dset)
        if self._dp and len(sample) != int(self.args.exp.batch_size) // self.world:
            raise ValueError(f"rank {self.rank}: the loader gave {len(sample)} utterances; exp.batch_size = {int(self.args.exp.batch_size)} is the "
                             f"global batch, each of the {self.world} ranks takes {int(self.args.exp.batch_size) // self.world}")
        return torch.as_tensor(sample).to(self.device).float()

    def _ema_s(self):
        e = self.args.exp
        return ema_factor(self.it, e.batch_size, e.ema_rampup, e.ema_rate)

    def train_step(self):
        """One training step (reference :225-243) with the EMA of this iteration fused into the optimizer pass; returns (error, sigma)"""
        self.optimizer.zero_grad()
        sample = self.get_batch()
        error, sigma = self.diff_params.loss_fn(self.network, sample, n=None)
        loss = error.mean()
        loss.backward()
        max_norm = float(self.args.exp.max_grad_norm) if self.args.exp.use_grad_clip else 0.0
        self.optimizer.step(max_norm=max_norm, ema_s=self._ema_s())
        self._ema_done_it = self.it
        self.last_loss = loss.detach()
        if self.args.logging.log:
            self.process_loss_for_logging(error, sigma)
        return error, sigma

    def update_ema(self):
        """EMA of the network weights (reference :245-258).  After a ``train_step`` of the same iteration it is already applied (fused);
        otherwise one EMA-only launch."""
        if self._ema_done_it == self.it:
            self._ema_done_it = None
            return
        self.optimizer.ema_update(self._ema_s())

    def training_loop(self):
        lg = self.args.logging
        rci = self._replica_check_interval() if self._dp else 0
        while True:
            self.train_step()
            self.update_ema()
            if self.it > 0 and self.it % lg.save_interval == 0 and lg.save_model:
                self.save_checkpoint()
            if self.it > 0 and self.it % lg.heavy_log_interval == 0 and lg.log:
                self.heavy_logging()
            if self.it > 0 and self.it % lg.log_interval == 0 and lg.log:
                self.easy_logging()
            if self._dp and rci > 0 and self.it > 0 and self.it % rci == 0:
                self.optimizer.check_replicas()
            self.it += 1
            if "max_iters" in self.args.exp.keys() and self.args.exp.max_iters is not None and self.it > self.args.exp.max_iters:
                break
