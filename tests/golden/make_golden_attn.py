#!/usr/bin/env python3
"""Golden fixtures of the NCSN++ attention sites (``attn_resolutions``), recorded from the *reference* on the CPU with the
helpers of ``make_golden.py`` (same stubs, same seeded ``buddy_amd.synth`` weights -- extended by the sites' parameters and
loaded into the reference with ``strict=True``, which pins the state-dict names; the list of names is stored as well).

    net_attn_lo     nf = 32, STFT 126 / 32, image_size 64, attn_resolutions (16,), 2 blocks: two down sites, one up site, C = 64
    net_attn_hi     the same with attn_resolutions (64, 32): levels 0 and 1 (C = 32 at T = 144 x 64 tokens: flash in ``auto``)
    net_full_attn   nf = 128, STFT 510 / 128, image_size 256, attn_resolutions (64, 32), L = 16000
    e2e_blind_attn  the blind sampler (as e2e_blind) on an nf = 32 network with network.attn_resolutions=[32], T = 5

Usage:  python tests/golden/make_golden_attn.py [--only NAME ...]
"""
import argparse
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the reference and the repository on sys.path, installs the stubs)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from buddy_amd.synth import attn_mask_of, synth_state_dict  # noqa: E402


def build_ref_net_attn(nf, n_fft, hop, seed, attn_resolutions, image_size, ch_mult=(1, 2, 2, 2), num_res_blocks=1):
    from networks.ncsnpp import NCSNppTime
    cfg = mg.load_yaml(os.path.join(mg.ROOT, "conf/network/ncsnpp.yaml"))
    cfg.pop("_target_")
    cfg.update(nf=nf, ch_mult=list(ch_mult), num_res_blocks=num_res_blocks, attn_resolutions=list(attn_resolutions), image_size=image_size,
               stft=mg.AttrDict(n_fft=n_fft, hop_length=hop, center=True))
    net = NCSNppTime(**cfg)
    mask = attn_mask_of(attn_resolutions, image_size, len(ch_mult))
    sd = synth_state_dict(seed, nf, tuple(ch_mult), num_res_blocks, attn_mask=mask)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.eval(), list(sd.keys())


def _net_attn_fixture(name, nf, n_fft, hop, L, B, seed, attn_resolutions, image_size, num_res_blocks=1):
    net, names = build_ref_net_attn(nf, n_fft, hop, seed, attn_resolutions, image_size, num_res_blocks=num_res_blocks)
    rs = np.random.RandomState(seed + 100)
    x = torch.from_numpy((0.5 * rs.standard_normal((B, 1, L))).astype(np.float32)).requires_grad_(True)
    cn = torch.from_numpy(rs.uniform(-2.0, 0.3, size=(B,)).astype(np.float32))
    cot = torch.from_numpy(rs.standard_normal((B, 1, L)).astype(np.float32))
    from networks.ncsnpp_utils import layerspp
    taps, hooks, kinds = {}, [], {}
    for i, mod in enumerate(net.all_modules):
        if isinstance(mod, (layerspp.ResnetBlockBigGANpp, layerspp.AttnBlockpp)):
            kinds[i] = "attn" if isinstance(mod, layerspp.AttnBlockpp) else "res"
            hooks.append(mod.register_forward_hook(lambda m, a, o, i=i: taps.__setitem__(i, o.detach())))
    y = net(x, cn)
    g, = torch.autograd.grad(y, x, cot)
    for h in hooks:
        h.remove()
    arrs = dict(x=x.detach(), cnoise=cn, cot=cot, y=y.detach(), vjp=g, meta=np.array([nf, n_fft, hop, L, B, seed]),
                ch_mult=np.array((1, 2, 2, 2)), num_res_blocks=np.array(num_res_blocks), attn_resolutions=np.array(attn_resolutions),
                image_size=np.array(image_size), names=np.array(names), attn_taps=np.array(sorted(i for i, k in kinds.items() if k == "attn")))
    for i, t in taps.items():
        arrs[f"tap{i}_mean"] = t.mean()
        arrs[f"tap{i}_absmax"] = t.abs().max()
        arrs[f"tap{i}_std"] = t.std()
    mg.save(name, **arrs)


def gen_net_attn():
    _net_attn_fixture("net_attn_lo", nf=32, n_fft=126, hop=32, L=4096, B=2, seed=31, attn_resolutions=(16,), image_size=64, num_res_blocks=2)
    _net_attn_fixture("net_attn_hi", nf=32, n_fft=126, hop=32, L=4096, B=2, seed=32, attn_resolutions=(64, 32), image_size=64, num_res_blocks=2)


def gen_net_full_attn():
    _net_attn_fixture("net_full_attn", nf=128, n_fft=510, hop=128, L=16000, B=1, seed=33, attn_resolutions=(64, 32), image_size=256)


def gen_e2e_blind_attn():
    """e2e_blind's sampler run (make_golden.gen_e2e_blind) with network.attn_resolutions=[32]: the network comes from the override"""
    orig = mg.build_ref_net

    def build(nf, n_fft, hop, seed, *a, **k):
        return build_ref_net_attn(nf, n_fft, hop, seed, attn_resolutions=(32,), image_size=256)[0]
    mg.build_ref_net = build
    try:
        mg._e2e("e2e_blind_attn", "blind_dereverberation_BUDDy", blind=True, T=5, order=1,
                overrides=["tester.posterior_sampling.warm_initialization.mode=reverb_scaled",
                           "tester.posterior_sampling.blind_hp.op_updates_per_step=3"])
    finally:
        mg.build_ref_net = orig


GENS = dict(net_attn=gen_net_attn, net_full_attn=gen_net_full_attn, e2e_blind_attn=gen_e2e_blind_attn)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    for k, fn in GENS.items():
        if a.only is None or k in a.only:
            print("==", k)
            fn()
