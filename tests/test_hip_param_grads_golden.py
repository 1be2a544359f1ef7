"""GPU: parameter gradients (buddy_ncsnpp_vjp_params through NCSNppTime.backward) against fixtures recorded from the reference
(tests/golden/make_golden_grads.py: float64 autograd of the reference network on the CPU) in every GEMM mode, the attention-site
configuration also with the flash attention core, and the nf = 128 network (N-tiled weight-gradient GEMMs: Cout up to 256).

Gates (the network tests' TOL = 5e-4): per parameter, |norm - ref| / ref and |<g, p_j> - ref_j| / ||g_ref|| (a standard-normal probe p_j gives
<g, p_j> of size ||g||); every 1-D gradient at max-abs-relative (the network tests' rel).  The key bias NIN_1.b of an attention block has an
exact gradient of 0 (softmax cancels a per-row shift): its values are measured against the norm of the same block's NIN_0.b gradient.  The
bias of a C -> 2 pyramid head is a sum over every pixel of the pyramid's gradient that cancels almost completely (~1e-3 of its terms survive):
it is measured against the norm of the same head's weight gradient.  These two are the only exceptions.  The Fourier W gets no gradient."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 5e-4
PROBE_SEED = 5000       # tests/golden/make_golden_grads.py


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def build(g, gemm, attention=None):
    from buddy_amd.config import AttrDict, CONF_DIR, load_yaml
    from buddy_amd.networks.ncsnpp import NCSNppTime
    from buddy_amd.synth import synth_state_dict
    nf, n_fft, hop, L, B, seed = [int(v) for v in g["meta"]]
    ch_mult, nrb = tuple(int(c) for c in g["ch_mult"]), int(g["num_res_blocks"])
    cfg = load_yaml(os.path.join(CONF_DIR, "network", "ncsnpp.yaml"))
    cfg.pop("_target_")
    cfg.update(nf=nf, gemm=gemm, attention=attention, ch_mult=list(ch_mult), num_res_blocks=nrb,
               attn_resolutions=[int(r) for r in g["attn_resolutions"]], image_size=int(g["image_size"]),
               stft=AttrDict(n_fft=n_fft, hop_length=hop, center=True))
    net = NCSNppTime(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(seed, nf, ch_mult, nrb, attn_mask=net.attn_mask).items()})
    return net.cuda()


_PROBES = {}


def probe_products(name, g_names, grads):
    """<g, p_j> for the fixture's probe rule, the probes drawn once per fixture"""
    out = {}
    for i, n in enumerate(g_names):
        if n not in grads:
            continue
        key = (name, n)
        if key not in _PROBES:
            shape = grads[n].shape
            _PROBES[key] = [torch.from_numpy(np.random.RandomState(PROBE_SEED + 2 * i + j).standard_normal(shape).astype(np.float32)).cuda()
                            for j in (0, 1)]
        out[n] = [float((grads[n].double() * p.double()).sum()) for p in _PROBES[key]]
    return out


@pytest.mark.parametrize("name,gemm,attention", [
    ("net_grads_small", "fp32", None), ("net_grads_small", "bf16x3", None), ("net_grads_small", "f16x2", None),
    ("net_grads_attn", "fp32", None), ("net_grads_attn", "bf16x3", None), ("net_grads_attn", "f16x2", None), ("net_grads_attn", "f16x2", "flash"),
    ("net_grads_full", "fp32", None), ("net_grads_full", "bf16x3", None), ("net_grads_full", "f16x2", None)])
def test_param_grads_vs_reference(golden, name, gemm, attention):
    g = golden(name)
    net = build(g, gemm, attention).requires_grad_(True)
    y = net(torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["cnoise"]).cuda())
    (y * torch.from_numpy(g["cot"]).cuda()).sum().backward()
    params = dict(net.named_parameters())
    assert params["all_modules.0.W"].grad is None, "the Fourier projection W must get no gradient"
    grads = {n: p.grad.detach() for n, p in params.items() if p.grad is not None}
    names = [str(n) for n in g["names"]]
    kept = [str(n) for n in g["grad_names"]]
    assert sorted(kept) == sorted(grads), "parameters with a gradient differ from the reference's"
    prods = probe_products(name, names, grads)
    ref_norm = dict(zip(kept, g["norm"]))
    bad, worst = [], (0.0, "")
    for i, n in enumerate(kept):
        scale = ref_norm[n]
        if n.endswith("NIN_1.b"):
            scale = ref_norm[n[:-len("NIN_1.b")] + "NIN_0.b"]
        if grads[n].shape == (2,) and n.startswith("all_modules."):        # a C -> 2 pyramid head's bias
            scale = max(scale, ref_norm[n[:-len("bias")] + "weight"])
        gn = float(grads[n].double().norm())
        errs = [abs(gn - ref_norm[n]) / scale] + [abs(prods[n][j] - float(g[f"probe{j}"][i])) / scale for j in (0, 1)]
        if grads[n].dim() == 1:
            r = g["g1d_" + n]
            errs.append(np.abs(grads[n].cpu().numpy() - r).max() / max(np.abs(r).max(), scale if scale != ref_norm[n] else 0.0))
        e = max(errs)
        if e > worst[0]:
            worst = (e, n)
        if e > TOL:
            bad.append((n, e))
    print(f"\n[{name} {gemm} {attention or 'auto'}] worst parameter: {worst[1]} {worst[0]:.2e}")
    assert not bad, f"parameter gradients off the reference (name, err): {sorted(bad, key=lambda t: -t[1])[:8]}"
