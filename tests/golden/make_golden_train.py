#!/usr/bin/env python3
"""Golden fixture of a short training run, recorded from the *reference's* ``training/trainer.py`` ``Trainer`` on the CPU in float64 with
torch's own Adam, ``clip_grad_norm_`` and the reference's EMA loop (helpers and stubs of ``make_golden.py`` / ``make_golden_grads.py``).

Two things the reference's Trainer needs that the stubs do not give: ``hydra.utils.instantiate`` (for the optimizer) is pointed at the
repository's ``instantiate``; and ``utils.training_utils.profile`` returns cleanly only with ``logging.profiling.enabled`` true (its body
then fails on a name it never imports, lands in its own ``except`` and switches profiling off), so that is what the configuration says,
with ``logging.log`` and ``print_model_summary`` false.

Set-up: the small geometry of ``net_grads_small`` (nf = 32, STFT 126 / 32, L = 4096, seeded ``buddy_amd.synth`` weights, seed 41),
batch_size 2, lr 1e-4, clipping on with max_grad_norm 1, ema_rate 0.9, ema_rampup 6, six steps: steps 0-2 take the ramp branch of the EMA
(s = 0, 1/3, 2/3), steps 3-5 the constant one.  Batches, the noise and the uniform draws behind the sigmas are fixed float32 arrays from
RandomState(SEED), fed through ``dset`` and a patched ``torch.randn`` / ``torch.rand`` in the order ``loss_fn`` draws them (``rand(B)`` for
the sigmas, then ``randn((B, L))``), so a GPU run can replay them.

The batches are SCALED: at the data's natural level (0.05 x standard normal, sigma_data) the gradient norm before clipping is 0.049 .. 0.053
in all six steps and max_grad_norm = 1 never clips.  With unit-variance batches (X_STD = 1) the norms are 5.76, 0.126, 6.61, 0.985, 1.037,
1.99: steps 0, 2, 4, 5 clip, steps 1 and 3 do not (recorded in ``clip_active``); the two nearest to the threshold are 1.5 % and 3.7 % away
from it, thirty times the 5e-4 tolerance of the parameter gradients.

The file holds:
    x, noise, u           (6, B, L), (6, B, L), (6, B) float32 inputs
    loss, grad_norm       per step: the mean loss and the global gradient norm before clipping (float64)
    clip_active, ema_s    per step: whether clip_grad_norm_ scaled the gradient, and the EMA factor the reference used
    names                 parameter names in state-dict order
    net_norm / ema_norm, net_probe0/1 / ema_probe0/1   per tensor after step 6: its norm and <tensor, p_j> with the probes of
                          make_golden_grads.probes (index = position in ``names``)
    net1d_<name> / ema1d_<name>   every 1-D tensor in full (float64)
    meta (nf, n_fft, hop, L, B, seed, steps), hp (lr, max_grad_norm, ema_rate, ema_rampup)

Usage:  python tests/golden/make_golden_train.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the reference and the repository on sys.path, installs the stubs)
import make_golden_grads as mgg  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

SEED, STEPS, B, L = 9100, 6, 2, 4096
NF, NFFT, HOP, NET_SEED = 32, 126, 32, 41
LR, MAX_NORM, EMA_RATE, EMA_RAMPUP = 1e-4, 1.0, 0.9, 6
X_STD = 1.0        # standard deviation of the batches, see the docstring


def inputs():
    rs = np.random.RandomState(SEED)
    x = (X_STD * rs.standard_normal((STEPS, B, L))).astype(np.float32)
    noise = rs.standard_normal((STEPS, B, L)).astype(np.float32)
    u = rs.uniform(0.0, 1.0, size=(STEPS, B)).astype(np.float32)
    return x, noise, u


class Draws:
    """torch.rand / torch.randn inside the reference's loss_fn: the recorded arrays, in order"""

    def __init__(self, noise, u):
        self.noise, self.u, self.kr, self.kn = noise, u, 0, 0

    def __enter__(self):
        self.orig = (torch.rand, torch.randn)

        def rand(*shape, **kw):
            out = torch.from_numpy(self.u[self.kr]).double()
            assert tuple(out.shape) == tuple(np.ravel(shape)), shape
            self.kr += 1
            return out

        def randn(*shape, **kw):
            if len(shape) == 1 and not isinstance(shape[0], int):
                shape = tuple(shape[0])
            out = torch.from_numpy(self.noise[self.kn]).double()
            assert tuple(out.shape) == tuple(shape), shape
            self.kn += 1
            return out

        torch.rand, torch.randn = rand, randn
        return self

    def __exit__(self, *a):
        torch.rand, torch.randn = self.orig


def main():
    from buddy_amd.config import compose, to_attrdict
    from buddy_amd.instantiate import instantiate
    import hydra
    hydra.utils = sys.modules["hydra.utils"]
    hydra.utils.instantiate = instantiate
    import networks.ncsnpp as ref_ncsnpp
    ref_ncsnpp.torch = mgg._Torch64()
    from diff_params.edm import EDM
    from training.trainer import Trainer

    args = compose()
    args.exp = to_attrdict(dict(exp_name="golden", seed=1, batch_size=B, resume=False, resume_checkpoint="None", ema_rate=EMA_RATE,
                                ema_rampup=EMA_RAMPUP, use_grad_clip=True, max_grad_norm=MAX_NORM, audio_len=L, sample_rate=16000,
                                optimizer={"_target_": "torch.optim.Adam", "lr": LR, "betas": [0.9, 0.999], "eps": 1e-8}))
    args.logging = to_attrdict(dict(log=False, print_model_summary=False,
                                    profiling=dict(enabled=True, wait=1, warmup=1, active=1, repeat=1)))
    net = mg.build_ref_net(NF, NFFT, HOP, NET_SEED).double()
    names = list(net.state_dict().keys())
    edm = EDM(args.diff_params.type, args.diff_params.sde_hp)
    x, noise, u = inputs()
    dset = iter([torch.from_numpy(b).double() for b in x])
    trainer = Trainer(args, dset, net, edm, types.SimpleNamespace(), "cpu")
    assert isinstance(trainer.optimizer, torch.optim.Adam) and trainer.it == 0

    losses, norms, ema_s = [], [], []
    orig_clip, orig_loss = torch.nn.utils.clip_grad_norm_, edm.loss_fn

    def clip(params, max_norm, *a, **k):
        total = orig_clip(params, max_norm, *a, **k)
        norms.append(float(total))
        return total

    def loss_fn(*a, **k):
        error, sigma = orig_loss(*a, **k)
        losses.append(float(error.mean()))
        return error, sigma

    torch.nn.utils.clip_grad_norm_, edm.loss_fn = clip, loss_fn
    try:
        with Draws(noise, u) as d:
            for _ in range(STEPS):
                t = trainer.it * B
                ema_s.append(float(np.clip(t / EMA_RAMPUP, 0.0, EMA_RATE)) if t < EMA_RAMPUP else EMA_RATE)
                trainer.train_step()
                trainer.update_ema()
                trainer.it += 1
            assert d.kr == STEPS and d.kn == STEPS
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
    clip_active = np.array([n > MAX_NORM for n in norms])
    print("loss", losses)
    print("gradient norm before clipping", norms, "clip active", clip_active)
    assert clip_active.any(), "no step clips with these inputs: scale the batch"

    arrs = {}
    for tag, mod in (("net", trainer.network), ("ema", trainer.ema)):
        sd = mod.state_dict()
        assert list(sd.keys()) == names
        norm, p0, p1 = [], [], []
        for i, n in enumerate(names):
            w = sd[n].detach().double().numpy()
            a, b = mgg.probes(i, w.shape)
            norm.append(np.linalg.norm(w)); p0.append(float((w * a).sum())); p1.append(float((w * b).sum()))
            if w.ndim == 1:
                arrs[f"{tag}1d_{n}"] = w
        arrs[f"{tag}_norm"], arrs[f"{tag}_probe0"], arrs[f"{tag}_probe1"] = np.array(norm), np.array(p0), np.array(p1)
    mg.save("train_small", x=x, noise=noise, u=u, loss=np.array(losses), grad_norm=np.array(norms), clip_active=clip_active,
            ema_s=np.array(ema_s), names=np.array(names), meta=np.array([NF, NFFT, HOP, L, B, NET_SEED, STEPS]),
            hp=np.array([LR, MAX_NORM, EMA_RATE, EMA_RAMPUP]), **arrs)


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    torch.set_default_dtype(torch.float64)
    main()
