"""GPU: data-parallel training (buddy_amd/training with a process group) on TWO ranks that share the one GPU of the test box (gloo control
plane, collectives staged through the pinned host buffer; HIP compute), at the geometry of tests/golden/train_small.npz (nf = 32,
gemm = "fp32", L = 4096, global batch B = 2: rank r takes row r of every ``x``, ``noise`` and ``u``).

One two-rank run is shared by the tests that read it (the fixture ``two_ranks``): the six steps of the fixture with ``check_replicas()`` after
every step, a checkpoint after step 3, the flat buffers of both ranks gathered once at the end, then one ulp of drift on rank 1.  A second
two-rank run holds the refusal and the resume from a single-process checkpoint; a third child is the one-rank RCCL group.

Bounds: those tests/test_hip_trainer.py holds the single process to against the same fixture (recorded from the reference's Trainer in
float64): every stored norm, probe product and 1-D tensor of network and EMA within 1e-4 of the tensor's norm; the loss -- here the mean over
the ranks -- 1e-4 relative; the gradient norm before clipping -- here of the averaged gradient -- 5e-4.  Everything else is equality of bits:
at world size 2 the all-reduce is ONE commutative fp32 addition per element and every kernel is deterministic."""
import json
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_hip_trainer import GOLD, TOL, TOL_GRAD, Draws, build_net, compare, make_args

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOIN_TIMEOUT = 600


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


class RankDraws:
    """torch.rand / torch.randn inside loss_fn: row ``rank`` of the fixture's arrays, in the order the generator fed them to the reference"""

    def __init__(self, d, rank, start=0):
        self.noise, self.u, self.r, self.kr, self.kn = d["noise"], d["u"], rank, start, start

    def __enter__(self):
        self.orig = (torch.rand, torch.randn)

        def rand(*shape, **kw):
            self.kr += 1
            return torch.from_numpy(self.u[self.kr - 1][self.r:self.r + 1])

        def randn(*shape, **kw):
            self.kn += 1
            return torch.from_numpy(self.noise[self.kn - 1][self.r:self.r + 1])

        torch.rand, torch.randn = rand, randn
        return self

    def __exit__(self, *a):
        torch.rand, torch.randn = self.orig


def rank_batches(d, rank, start=0):
    return iter([torch.from_numpy(b[rank:rank + 1]) for b in d["x"][start:]])


def make_rank_trainer(d, model_dir, rank, start=0, rows=None, **exp):
    """a Trainer whose loader yields row ``rank`` of every fixture batch (``rows`` = "all": the whole batch, for a world of one)"""
    from buddy_amd.diff_params.edm import EDM
    from buddy_amd.training.trainer import Trainer
    args = make_args(d, model_dir, **exp)
    edm = EDM(args.diff_params.type, args.diff_params.sde_hp)
    dset = iter([torch.from_numpy(b) for b in d["x"][start:]]) if rows == "all" else rank_batches(d, rank, start)
    return Trainer(args, dset, build_net(d), edm, None, torch.device("cuda", 0))


def flats(opt):
    return [t.detach().clone() for t in (opt._p, opt._m, opt._v, opt._ema)]


def one_step(tr):
    tr.train_step()
    tr.update_ema()
    tr.it += 1


def spawn_ranks(fn, args, nprocs=2):
    """mp.spawn with a timeout on the join; an abnormal exit of a rank raises here, once"""
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + JOIN_TIMEOUT
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"the ranks did not finish within {JOIN_TIMEOUT} s")


def _init_rank(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from buddy_amd import dist as bd
    torch.cuda.set_device(0)
    bd.init(backend="gloo")


# ---- the shared two-rank run ---------------------------------------------------------------------------------------------------------------------
def _six_steps_worker(rank, world, port, out):
    import torch.distributed as dist
    from buddy_amd import _lib
    _init_rank(rank, world, port)
    d = np.load(GOLD)
    tr = make_rank_trainer(d, os.path.join(out, "ckpt"), rank)
    assert tr.world == 2 and tr.rank == rank and tr.optimizer._host is not None and tr.optimizer._host.is_pinned()
    host_ptr = tr.optimizer._host.data_ptr()
    res = {"losses": [], "norms": [], "checks": 0, "ms": []}
    with RankDraws(d, rank):
        for k in range(int(d["meta"][6])):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one_step(tr)
            torch.cuda.synchronize()
            res["ms"].append((time.perf_counter() - t0) * 1e3)
            res["losses"].append(float(tr.last_loss))
            res["norms"].append(tr.optimizer.grad_norm())
            tr.optimizer.check_replicas()
            res["checks"] += 1
            if tr.it == 3:
                tr.save_checkpoint()
                res["flat3"] = [t.cpu() for t in flats(tr.optimizer)]
    assert tr.optimizer._host.data_ptr() == host_ptr, "the staging buffer is allocated once"
    res["flat"] = [t.cpu() for t in flats(tr.optimizer)]
    res["steps"] = sorted({float(st["step"]) for st in tr.optimizer.state.values() if len(st)})
    if rank == 0:
        res["net"] = {k: v.cpu() for k, v in tr.network.state_dict().items()}
        res["ema"] = {k: v.cpu() for k, v in tr.ema.state_dict().items()}
    # what the all-reduce costs on this route (host-staged gloo, two ranks on one GPU): timed on the gradient buffer, after everything that reads it
    opt, ar = tr.optimizer, []
    for _ in range(3):
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt._all_reduce_sum(opt._g)
        torch.cuda.synchronize()
        ar.append((time.perf_counter() - t0) * 1e3)
    res["allreduce_ms"], res["n_params"] = ar, opt._n
    # drift: one ulp in one element of rank 1's first-moment buffer, a plain tensor write
    if rank == 1:
        i = opt._n // 2
        opt._m[i:i + 1] = torch.nextafter(opt._m[i:i + 1], torch.full_like(opt._m[i:i + 1], float("inf")))
    try:
        opt.check_replicas()
        res["drift"] = None
    except _lib.BuddyHipError as e:
        res["drift"] = str(e)
    torch.save(res, os.path.join(out, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ddp"))
    spawn_ranks(_six_steps_worker, (2, _free_port(), out))
    return out, [torch.load(os.path.join(out, f"rank{r}.pt"), weights_only=False) for r in (0, 1)]


class _SD:
    def __init__(self, sd):
        self.sd = sd

    def state_dict(self):
        return self.sd


def test_fixture_replay_on_two_ranks(two_ranks):
    _, (r0, r1) = two_ranks
    d = np.load(GOLD)
    assert list(d["clip_active"]) == [True, False, True, False, True, True]
    losses = [(a + b) / 2 for a, b in zip(r0["losses"], r1["losses"])]
    assert r0["norms"] == r1["norms"], "both ranks hold the same summed gradient"
    norms = r0["norms"]
    el = [abs(a - r) / abs(r) for a, r in zip(losses, d["loss"])]
    eg = [abs(a - r) / r for a, r in zip(norms, d["grad_norm"])]
    for k in range(len(losses)):
        print(f"two ranks step {k}: loss {losses[k]:.6f} vs {d['loss'][k]:.6f} rel {el[k]:.2e}; grad norm {norms[k]:.6f} vs {d['grad_norm'][k]:.6f} rel {eg[k]:.2e}")
    wn, we = compare("two ranks", _SD(r0["net"]), d, "net"), compare("two ranks", _SD(r0["ema"]), d, "ema")
    lines = ["six training steps on TWO ranks (gloo, one GPU), nf = 32 (tests/golden/train_small.npz), rank r = row r of the fixture's batch, against the fixture",
             f"network: worst error / tensor norm {wn[0]:.2e} ({wn[1]}); ema: {we[0]:.2e} ({we[1]})   [bound {TOL:g}]",
             f"loss (mean over ranks), worst relative {max(el):.2e}   [bound {TOL:g}]",
             f"gradient norm before clipping (averaged gradient), worst relative {max(eg):.2e}   [bound {TOL_GRAD:g}]",
             f"step wall time, ms, rank 0: {[round(v, 1) for v in r0['ms']]}",
             f"all-reduce of the {r0['n_params']} fp32 gradients, host-staged gloo smoke-test route (not an xGMI number), ms: "
             f"{[round(v, 2) for v in r0['allreduce_ms']]}"]
    print("\n".join(lines))
    rep = os.environ.get("DDP_ACCURACY_OUT")              # profiles/ddp_accuracy.txt is a copy of this report
    if rep:
        with open(rep, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert max(el) <= TOL, el
    assert max(eg) <= TOL_GRAD, eg
    for k, a in enumerate(norms):
        assert (a > float(d["hp"][1])) == bool(d["clip_active"][k]), f"step {k}: clipping differs from the reference run"
    assert wn[0] <= TOL, wn
    assert we[0] <= TOL, we


def test_replicas_agree_after_six_steps(two_ranks):
    _, (r0, r1) = two_ranks
    assert r0["checks"] == r1["checks"] == 6, "check_replicas() passed after every step on both ranks"
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq", "ema"), r0["flat"], r1["flat"]):
        assert torch.equal(a, b), name
    assert r0["steps"] == r1["steps"] == [6.0]
    assert not torch.equal(r0["flat"][0], r0["flat3"][0])


def test_two_ranks_equal_one_process_summing_the_two_gradients(two_ranks, tmp_path):
    """One process: rank 0's and rank 1's gradient one after the other from the same weights, their fp32 sum written into the gradient
    buffer, the scaled step with 1/2.  Three steps: equal bits with the two-rank run."""
    _, (r0, _) = two_ranks
    d = np.load(GOLD)
    tr = make_rank_trainer(d, str(tmp_path), 0)
    assert not tr._dp
    opt, edm = tr.optimizer, tr.diff_params
    max_norm = float(tr.args.exp.max_grad_norm)
    for it in range(3):
        grads = []
        for r in (0, 1):
            opt.zero_grad()
            with RankDraws(d, r, it):
                error, _ = edm.loss_fn(tr.network, torch.from_numpy(d["x"][it][r:r + 1]).cuda(), n=None)
            error.mean().backward()
            grads.append(opt._g.clone())
        opt._g.copy_(grads[0] + grads[1])
        opt.step(max_norm=max_norm, ema_s=tr._ema_s(), grad_scale=0.5)
        tr.it += 1
    torch.cuda.synchronize()
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq", "ema"), flats(opt), r0["flat3"]):
        assert torch.equal(a.cpu(), b), f"{name}: the two-rank run differs from its one-process emulation"


def test_checkpoint_of_two_ranks_resumes_in_one_process(two_ranks):
    out, (r0, _) = two_ranks
    path = os.path.join(out, "ckpt", "t-3.pt")
    assert os.path.exists(path) and [f for f in os.listdir(os.path.join(out, "ckpt")) if f.endswith(".pt")] == ["t-3.pt"], "rank 0 writes the one file"
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(ckpt.keys()) == ["args", "ema", "it", "network", "optimizer"] and ckpt["it"] == 3
    d = np.load(GOLD)
    tr = make_rank_trainer(d, os.path.join(out, "ckpt"), 0, rows="all", resume=True)
    assert not tr._dp and tr.it == 3
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq", "ema"), flats(tr.optimizer), r0["flat3"]):
        assert torch.equal(a.cpu(), b), name
    assert {float(st["step"]) for st in tr.optimizer.state.values() if len(st)} == {3.0}


def test_drift_of_one_ulp_is_caught_on_both_ranks(two_ranks):
    _, ranks = two_ranks
    for r, res in enumerate(ranks):
        msg = res["drift"]
        assert msg is not None, f"rank {r}: check_replicas() did not raise"
        assert "exp_avg differs from rank 0 on rank(s) [1]" in msg, msg
        assert "exp_avg_sq" not in msg and "param" not in msg and "ema" not in msg, msg


# ---- refusal, and a single-process checkpoint resumed on two ranks --------------------------------------------------------------------------------
def _resume_worker(rank, world, port, out):
    import torch.distributed as dist
    _init_rank(rank, world, port)
    d = np.load(GOLD)
    res = {}
    try:
        make_rank_trainer(d, os.path.join(out, "none"), rank, batch_size=3)
        res["refusal"] = None
    except ValueError as e:
        res["refusal"] = str(e)
    # only rank 0 sees the checkpoint: rank 1 looks into an empty directory and starts fresh, the broadcast makes the two equal
    tr = make_rank_trainer(d, os.path.join(out, "single" if rank == 0 else "empty"), rank, start=2, resume=True)
    res["it"] = tr.it
    res["flat_resumed"] = [t.cpu() for t in flats(tr.optimizer)]
    res["steps"] = sorted({float(st["step"]) for st in tr.optimizer.state.values() if len(st)})
    # the step after the resume also logs: every rank enters the gather of the per-utterance errors, rank 0 writes the row of the global batch
    tr.args.logging.log = True
    tr.setup_logging_variables()
    with RankDraws(d, rank, 2):
        one_step(tr)
    tr.easy_logging()
    tr.optimizer.check_replicas()
    res["loss"] = float(tr.last_loss)
    log = os.path.join(tr.args.model_dir, "train_log.jsonl")
    res["log"] = [json.loads(ln) for ln in open(log)] if os.path.exists(log) else None
    res["flat_next"] = [t.cpu() for t in flats(tr.optimizer)]
    torch.save(res, os.path.join(out, f"resume{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_refusal_and_single_process_checkpoint_resumed_on_two_ranks(tmp_path):
    from test_hip_trainer import make_trainer, _steps
    d = np.load(GOLD)
    out = str(tmp_path)
    os.makedirs(os.path.join(out, "empty"))
    single = make_trainer(d, os.path.join(out, "single"))
    _steps(single, d, 2, 0)
    single.save_checkpoint()
    torch.cuda.synchronize()
    want = [t.cpu() for t in flats(single.optimizer)]
    spawn_ranks(_resume_worker, (2, _free_port(), out))
    r0, r1 = (torch.load(os.path.join(out, f"resume{r}.pt"), weights_only=False) for r in (0, 1))
    for r, res in enumerate((r0, r1)):
        assert res["refusal"] is not None and "3" in res["refusal"] and "2" in res["refusal"], (r, res["refusal"])
        assert "batch_size = 3" in res["refusal"] and "2 ranks" in res["refusal"], res["refusal"]
        assert res["it"] == 2 and res["steps"] == [2.0]
    for name, a, b, c in zip(("p", "exp_avg", "exp_avg_sq", "ema"), r0["flat_resumed"], r1["flat_resumed"], want):
        assert torch.equal(a, b), f"{name}: the replicas differ after the resume"
        assert torch.equal(a, c), f"{name}: rank 0 differs from the single-process state"
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq", "ema"), r0["flat_next"], r1["flat_next"]):
        assert torch.equal(a, b), f"{name}: the replicas differ one step after the resume"
    assert not torch.equal(r0["flat_next"][0], r0["flat_resumed"][0])
    # the log: written by rank 0 alone, from the global batch (fp32 means of 4096 squared errors each: 1e-6 relative)
    assert r1["log"] is None and r0["log"] is not None and r0["log"][0]["it"] == 2
    mean = (r0["loss"] + r1["loss"]) / 2
    assert abs(r0["log"][0]["loss"] - mean) <= 1e-6 * abs(mean), (r0["log"], r0["loss"], r1["loss"])


# ---- one rank, RCCL: the device path of the collectives ---------------------------------------------------------------------------------------------
def _rccl_one_rank(port, out_path):
    """child process: two steps without a group, then the same two steps under a forced one-rank ``nccl`` group, whose all-reduce and broadcasts
    take the device buffers (no multi-rank test on a 1-GPU box can: RCCL wants one device per rank)"""
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    from buddy_amd import dist as bd
    torch.cuda.set_device(0)
    d = np.load(GOLD)

    def two_steps(tmp):
        tr = make_rank_trainer(d, tmp, 0, rows="all")
        with Draws(d):
            for _ in range(2):
                one_step(tr)
        torch.cuda.synchronize()
        return tr

    plain = two_steps(os.path.join(os.path.dirname(out_path), "plain"))
    assert not plain._dp
    bd.init(backend="nccl", device=torch.device("cuda", 0), force=True)
    assert dist.is_initialized() and dist.get_backend() == "nccl" and dist.get_world_size() == 1
    grouped = two_steps(os.path.join(os.path.dirname(out_path), "grouped"))
    assert grouped._dp and grouped.world == 1 and grouped.optimizer._device_coll and grouped.optimizer._host is None
    table = grouped.optimizer.check_replicas()
    same = all(bool(torch.equal(a, b)) for a, b in zip(flats(plain.optimizer), flats(grouped.optimizer)))
    norms = (plain.optimizer.grad_norm(), grouped.optimizer.grad_norm())
    dist.barrier()
    dist.destroy_process_group()
    json.dump({"same": same, "norms": norms, "rows": len(table)}, open(out_path, "w"))


def test_one_rank_rccl_group_keeps_the_bits(tmp_path):
    out = str(tmp_path / "rccl.json")
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_one_rank, args=(_free_port(), out))
    p.start(); p.join(JOIN_TIMEOUT)
    if p.is_alive():
        p.kill()
        pytest.fail("the one-rank RCCL child did not finish")
    assert p.exitcode == 0, f"RCCL one-rank child failed (exit {p.exitcode})"
    j = json.load(open(out))
    assert j["same"] and j["norms"][0] == j["norms"][1] and j["rows"] == 1, j
