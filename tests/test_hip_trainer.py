"""GPU: the training loop (buddy_amd/training) -- six steps replayed against the fixture recorded from the reference's Trainer in float64
(tests/golden/train_small.npz), the same steps through torch's Adam / clip_grad_norm_ / the reference's EMA loop, resume from a checkpoint
bit for bit, freshness of network and EMA after a step, sampling from a trained checkpoint, and the untouched default path.

Tolerances (the project's own, tests/test_hip_param_grads.py): loss 1e-4 relative; every stored norm, probe product and 1-D tensor of network
and EMA 1e-4 of the tensor's norm (test_short_training_run_vs_fp64 holds torch's Adam to both over five steps at the same learning rate);
the gradient norms before clipping 5e-4 (the parameter-gradient tolerance)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "train_small.npz")
PROBE_SEED = 5000           # tests/golden/make_golden_grads.py
TOL, TOL_GRAD = 1e-4, 5e-4


def probes(i, shape):
    return [np.random.RandomState(PROBE_SEED + 2 * i + j).standard_normal(shape).astype(np.float32) for j in (0, 1)]


def build_net(d):
    from buddy_amd.config import load_yaml, CONF_DIR, AttrDict
    from buddy_amd.networks.ncsnpp import NCSNppTime
    from buddy_amd.synth import synth_state_dict
    nf, n_fft, hop, L, B, seed, steps = (int(v) for v in d["meta"])
    cfg = load_yaml(os.path.join(CONF_DIR, "network", "ncsnpp.yaml"))
    cfg.pop("_target_")
    cfg.update(nf=nf, gemm="fp32", stft=AttrDict(n_fft=n_fft, hop_length=hop, center=True))
    net = NCSNppTime(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(seed, nf).items()})
    return net.cuda()


def make_args(d, model_dir, **exp):
    from buddy_amd.config import compose_train
    lr, max_norm, rate, rampup = (float(v) for v in d["hp"])
    nf, n_fft, hop, L, B, seed, steps = (int(v) for v in d["meta"])
    args = compose_train(overrides=[f"network.nf={nf}", f"exp.batch_size={B}", f"exp.optimizer.lr={lr}", f"exp.max_grad_norm={max_norm}",
                                    f"exp.ema_rate={rate}", f"exp.ema_rampup={rampup}", "exp.resume=false", "logging.log=false",
                                    "logging.save_model=false", f"exp.audio_len={L}", f"model_dir={model_dir}", "exp.exp_name=t"])
    for k, v in exp.items():
        args.exp[k] = v
    return args


class Draws:
    """torch.rand / torch.randn inside loss_fn: the fixture's arrays in the order the generator fed them to the reference"""

    def __init__(self, d, start=0):
        self.noise, self.u, self.kr, self.kn = d["noise"], d["u"], start, start

    def __enter__(self):
        self.orig = (torch.rand, torch.randn)

        def rand(*shape, **kw):
            self.kr += 1
            return torch.from_numpy(self.u[self.kr - 1])

        def randn(*shape, **kw):
            self.kn += 1
            return torch.from_numpy(self.noise[self.kn - 1])

        torch.rand, torch.randn = rand, randn
        return self

    def __exit__(self, *a):
        torch.rand, torch.randn = self.orig


def make_trainer(d, model_dir, net=None, start=0, **exp):
    from buddy_amd.diff_params.edm import EDM
    from buddy_amd.training.trainer import Trainer
    args = make_args(d, model_dir, **exp)
    net = build_net(d) if net is None else net
    edm = EDM(args.diff_params.type, args.diff_params.sde_hp)
    dset = iter([torch.from_numpy(b) for b in d["x"][start:]])
    return Trainer(args, dset, net, edm, None, torch.device("cuda", 0))


def compare(tag, module, d, key):
    """every stored norm, probe product and 1-D tensor of the fixture against ``module``; returns the worst error / tensor norm"""
    sd = module.state_dict()
    worst, over = (0.0, ""), []
    for i, n in enumerate(d["names"]):
        w = sd[str(n)].detach().cpu().double().numpy()
        ref_norm = float(d[f"{key}_norm"][i])
        a, b = probes(i, w.shape)
        # a probe product <w, p> with a standard-normal p has the scale ||w||: every error is measured against the tensor's norm
        errs = [abs(np.linalg.norm(w) - ref_norm), abs(float((w * a.astype(np.float64)).sum()) - float(d[f"{key}_probe0"][i])),
                abs(float((w * b.astype(np.float64)).sum()) - float(d[f"{key}_probe1"][i]))]
        if w.ndim == 1:
            errs.append(float(np.linalg.norm(w - d[f"{key}1d_{n}"])))
        e = max(errs) / (ref_norm + 1e-30)
        if e > TOL:
            over.append(f"{n} {e:.2e}" + (f" (difference {w - d[f'{key}1d_{n}']})" if w.ndim == 1 and w.size <= 4 else ""))
        if e > worst[0]:
            worst = (e, str(n))
    print(f"{tag}: worst {key} error / tensor norm {worst[0]:.2e} ({worst[1]}); above {TOL:g}: {over or 'none'}")
    return worst


def run_fused(d, tmp):
    tr = make_trainer(d, tmp)
    steps = int(d["meta"][6])
    losses, norms = [], []
    with Draws(d):
        for _ in range(steps):
            tr.train_step()
            losses.append(float(tr.last_loss))
            norms.append(tr.optimizer.grad_norm())
            tr.update_ema()
            tr.it += 1
    return tr, losses, norms


def run_torch(d):
    """the parent route: torch.optim.Adam, clip_grad_norm_ and the reference's EMA loop on a second copy of the network"""
    from buddy_amd.diff_params.edm import EDM
    from buddy_amd.training.trainer import ema_factor
    args = make_args(d, "unused")
    net = build_net(d)
    for (_, _, kind, _), p in zip(net._specs, net._params()):
        p.requires_grad_(kind != "fourier")
    edm = EDM(args.diff_params.type, args.diff_params.sde_hp)
    opt = torch.optim.Adam(net.parameters(), lr=args.exp.optimizer.lr, betas=tuple(args.exp.optimizer.betas), eps=args.exp.optimizer.eps)
    ema = copy.deepcopy(net).eval().requires_grad_(False)
    losses, norms = [], []
    with Draws(d):
        for it in range(int(d["meta"][6])):
            opt.zero_grad()
            error, _ = edm.loss_fn(net, torch.from_numpy(d["x"][it]).cuda(), n=None)
            loss = error.mean()
            loss.backward()
            norms.append(float(torch.nn.utils.clip_grad_norm_(net.parameters(), args.exp.max_grad_norm)))
            opt.step()
            losses.append(float(loss.detach()))
            s = ema_factor(it, args.exp.batch_size, args.exp.ema_rampup, args.exp.ema_rate)
            with torch.no_grad():
                for dst, src in zip(ema.parameters(), net.parameters()):
                    dst.copy_(dst * s + src * (1 - s))
    return net, ema, losses, norms


def gate(tag, d, losses, norms, net, ema):
    for k, (a, r) in enumerate(zip(losses, d["loss"])):
        e = abs(a - r) / abs(r)
        print(f"{tag} step {k}: loss {a:.6f} vs {r:.6f} rel {e:.2e}; grad norm {norms[k]:.6f} vs {d['grad_norm'][k]:.6f}")
    wn, we = compare(tag, net, d, "net"), compare(tag, ema, d, "ema")
    for k, (a, r) in enumerate(zip(losses, d["loss"])):
        assert abs(a - r) / abs(r) <= TOL, f"{tag} step {k}: loss {a} vs {r}"
    for k, (a, r) in enumerate(zip(norms, d["grad_norm"])):
        assert abs(a - r) / r <= TOL_GRAD, f"{tag} step {k}: gradient norm {a} vs {r}"
        assert (a > float(d["hp"][1])) == bool(d["clip_active"][k]), f"{tag} step {k}: clipping differs from the reference run"
    assert wn[0] <= TOL, f"{tag}: network {wn}"
    assert we[0] <= TOL, f"{tag}: EMA {we}"


def test_six_steps_vs_reference_fixture_and_parent_route(tmp_path):
    d = np.load(GOLD)
    assert d["clip_active"].any() and not d["clip_active"].all()
    tr, losses, norms = run_fused(d, str(tmp_path))
    net_t, ema_t, losses_t, norms_t = run_torch(d)
    # the difference between the two routes: reported, not gated (two fp32 orderings of Adam may step lr apart where a gradient is rounding noise)
    lines = ["six training steps, nf = 32 (tests/golden/train_small.npz): fused HIP step vs torch Adam + clip_grad_norm_ + EMA loop",
             "per tensor: ||a - b|| / ||b||; worst over the tensors"]
    for key, a, b in (("network", tr.network, net_t), ("ema", tr.ema, ema_t)):
        sa, sb = a.state_dict(), b.state_dict()
        worst = max(((float((sa[k].double() - sb[k].double()).norm() / (sb[k].double().norm() + 1e-30)), k) for k in sa), key=lambda t: t[0])
        mx = max(float((sa[k] - sb[k]).abs().max()) for k in sa)
        lines.append(f"{key}: worst relative difference {worst[0]:.3e} ({worst[1]}), largest absolute difference {mx:.3e} (lr = {float(d['hp'][0]):g})")
    lines.append("loss, per step, relative: " + " ".join(f"{abs(a - b) / abs(b):.2e}" for a, b in zip(losses, losses_t)))
    print("\n".join(lines))
    out = os.environ.get("TRAINER_ACCURACY_OUT")          # profiles/trainer_accuracy.txt is a copy of this report
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    # both routes are measured and printed before either is gated
    failures = []
    for tag, args in (("fused", (losses, norms, tr.network, tr.ema)), ("torch", (losses_t, norms_t, net_t, ema_t))):
        try:
            gate(tag, d, *args)
        except AssertionError as e:
            failures.append(str(e).splitlines()[0])
    assert not failures, failures


def _steps(tr, d, n, start):
    with Draws(d, start):
        for k in range(n):
            torch.manual_seed(100 + start + k)
            tr.train_step()
            tr.update_ema()
            tr.it += 1


def test_resume_is_bit_exact(tmp_path):
    d = np.load(GOLD)
    a = make_trainer(d, str(tmp_path / "a"))
    _steps(a, d, 4, 0)
    b = make_trainer(d, str(tmp_path / "b"))
    _steps(b, d, 2, 0)
    b.save_checkpoint()
    path = str(tmp_path / "b" / "t-2.pt")
    assert os.path.exists(path) and b.latest_checkpoint == path
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(ckpt.keys()) == ["args", "ema", "it", "network", "optimizer"] and ckpt["it"] == 2
    cpu_params = [torch.nn.Parameter(torch.zeros(p.shape), requires_grad=p.requires_grad) for p in b.network.parameters()]
    torch.optim.Adam(cpu_params).load_state_dict(ckpt["optimizer"])           # torch's own Adam accepts the optimizer state
    c = make_trainer(d, str(tmp_path / "b"), start=2, resume=True)
    assert c.it == 2
    _steps(c, d, 2, 2)
    assert c.it == a.it == 4
    for (k, x), y in zip(a.network.state_dict().items(), c.network.state_dict().values()):
        assert torch.equal(x, y), f"network {k}"
    for (k, x), y in zip(a.ema.state_dict().items(), c.ema.state_dict().values()):
        assert torch.equal(x, y), f"ema {k}"
    assert torch.equal(a.optimizer._m, c.optimizer._m) and torch.equal(a.optimizer._v, c.optimizer._v)
    sa, sc = a.optimizer.state_dict(), c.optimizer.state_dict()
    assert sa["param_groups"] == sc["param_groups"] and sa["state"].keys() == sc["state"].keys()
    assert all(float(sa["state"][i]["step"]) == float(sc["state"][i]["step"]) == 4.0 for i in sa["state"])


def test_freshness_of_network_and_ema_after_a_step(tmp_path):
    d = np.load(GOLD)
    tr = make_trainer(d, str(tmp_path))
    _steps(tr, d, 2, 0)
    L, B = int(d["meta"][3]), int(d["meta"][4])
    x = torch.from_numpy(d["x"][0]).cuda()[:, None]
    cn = torch.tensor([-0.7, -0.1], device="cuda")
    with torch.no_grad():
        for mod in (tr.network, tr.ema):
            y = mod(x, cn).clone()
            fresh = build_net(d)
            fresh.load_state_dict(mod.state_dict())
            assert torch.equal(y, fresh(x, cn)), "the forward after a fused step differs from a module that loaded the updated state_dict"
        assert not torch.equal(tr.network(x, cn), tr.ema(x, cn))
    # update_ema on its own (no train_step before it in this iteration): one EMA-only launch, visible in the next forward
    before = tr.ema.state_dict()["output_layer.bias"].clone()
    tr.update_ema()
    assert not torch.equal(before, tr.ema.state_dict()["output_layer.bias"])
    with torch.no_grad():
        fresh = build_net(d)
        fresh.load_state_dict(tr.ema.state_dict())
        assert torch.equal(tr.ema(x, cn), fresh(x, cn))
    # a gradient that is not the optimizer's view is refused, not gathered
    from buddy_amd import _lib
    tr.optimizer.zero_grad()
    with Draws(d, 2):
        error, _ = tr.diff_params.loss_fn(tr.network, tr.get_batch(), n=None)
    error.mean().backward()
    tr.network.output_layer.bias.grad = torch.zeros(2, device="cuda")
    with pytest.raises(_lib.BuddyHipError):
        tr.optimizer.step()


def test_sampling_from_a_trained_checkpoint(tmp_path):
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.synth import synth_clean, synth_rir
    from buddy_amd.testing.tester import Tester
    d = np.load(GOLD)
    tr = make_trainer(d, str(tmp_path))
    _steps(tr, d, 2, 0)
    tr.save_checkpoint()
    L = 8192
    args = compose(overrides=["network.nf=32", "tester.sampling_params.T=3", "tester.posterior_sampling.warm_initialization.mode=reverb_scaled",
                              "tester.posterior_sampling.blind_hp.op_updates_per_step=2"])
    net = build_net(d)
    t = Tester(args, net, instantiate(args.diff_params), test_set=None, device="cuda:0", in_training=True)
    assert t.load_checkpoint(tr.latest_checkpoint) is True and t.it == 2
    for (k, a), b in zip(net.state_dict().items(), tr.ema.state_dict().values()):
        assert torch.equal(a, b), f"the sampler must run on the EMA weights ({k})"
    item = (synth_clean(0, L), synth_rir(0, 1500), "u0.wav")
    _, yb, op, _ = t.prepare_batch([item], blind=True)
    pred = t.sampler.predict_conditional(yb, op, shape=(1, L), blind=True)
    assert tuple(pred.shape) == (1, L) and bool(torch.isfinite(pred).all())


def test_default_path_untouched_by_the_training_package():
    """no optimizer attached: forward and input-VJP are bit-identical before and after buddy_amd.training is imported (run in a fresh
    process each, so that 'before' really is before)"""
    import subprocess
    code = r'''
import sys, hashlib
sys.path.insert(0, %r)
import numpy as np, torch
if %d:
    import buddy_amd.training.trainer, buddy_amd.training.fused
sys.path.insert(0, %r)
from test_hip_trainer import build_net, GOLD
d = np.load(GOLD)
net = build_net(d).eval()
x = torch.from_numpy(d["x"][0]).cuda().requires_grad_(True)
y = net(x[:, None], torch.tensor([-0.7, -0.1], device="cuda"))
g, = torch.autograd.grad(y, x, torch.from_numpy(d["noise"][0]).cuda()[:, None])
assert net._flat is None and net._grad_flat is None
print("HASH", hashlib.sha256(y.detach().cpu().numpy().tobytes() + g.cpu().numpy().tobytes()).hexdigest())
'''
    hashes = []
    for with_training in (0, 1):
        r = subprocess.run([sys.executable, "-c", code % (ROOT, with_training, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        hashes.append([ln for ln in r.stdout.splitlines() if ln.startswith("HASH")][0])
    assert hashes[0] == hashes[1]
