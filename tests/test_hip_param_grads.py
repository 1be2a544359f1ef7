"""GPU: parameter gradients of the hand-written NCSN++ (buddy_ncsnpp_vjp_params) against float64 autograd of the CPU oracle, their
determinism and batching, torch's accumulate semantics, freshness after an optimizer step (buddy_ncsnpp_update_params, replicas included)
and a short Adam run against a float64 CPU restatement of the same training step.

Tolerance (stated): max-abs error relative to the tensor's max-abs <= 5e-4 per parameter tensor, the network tests' TOL.  The weight gradients
themselves are exact fp32; the error comes from the output gradients the input-VJP forms on the way (the GEMM mode's arithmetic).  The biases of
the 2-channel pyramid heads are sums over every pixel of the pyramid's gradient, which cancel almost completely (every head's bias gets the same
sum, and the periodic Hann window's zero at sample 0 makes it ~0): they are measured against the scale of the same head's weight gradient.
The key bias NIN_1.b of an attention block has an exact gradient of 0: it is measured against the block's NIN_0.b gradient.  These two are the
only exceptions to the per-tensor gate."""
import copy
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 5e-4


def build(nf=32, n_fft=126, hop=32, seed=3, fir=False, gemm=None, ch_mult=(1, 2, 2, 2), num_res_blocks=1):
    from buddy_amd.config import load_yaml, CONF_DIR, AttrDict
    from buddy_amd.networks.ncsnpp import NCSNppTime
    from buddy_amd.synth import synth_state_dict
    cfg = load_yaml(os.path.join(CONF_DIR, "network", "ncsnpp.yaml"))
    cfg.pop("_target_")
    cfg.update(nf=nf, fir=fir, gemm=gemm, ch_mult=list(ch_mult), num_res_blocks=num_res_blocks,
               stft=AttrDict(n_fft=n_fft, hop_length=hop, center=True))
    net = NCSNppTime(**cfg)
    sd = synth_state_dict(seed, nf, tuple(ch_mult), num_res_blocks)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.cuda(), sd


def inputs(B, L, seed=0):
    rs = np.random.RandomState(seed)
    x = (0.1 * rs.standard_normal((B, L))).astype(np.float32)
    cn = (0.25 * np.log(rs.uniform(0.01, 5.0, B))).astype(np.float32)
    cot = rs.standard_normal((B, L)).astype(np.float32)
    return x, cn, cot


def gpu_grads(net, x, cn, cot):
    net.requires_grad_(True)
    net.zero_grad(set_to_none=True)
    y = net(torch.from_numpy(x).cuda(), torch.from_numpy(cn).cuda())
    (y * torch.from_numpy(cot).cuda()).sum().backward()
    torch.cuda.synchronize()
    return {n: (None if p.grad is None else p.grad.detach().cpu().double().numpy()) for n, p in net.named_parameters()}


def ref_grads(sd, x, cn, cot, n_fft, hop, ch_mult, num_res_blocks, fir, f64=True):
    import contextlib
    from oracle.ncsnpp_ref import ncsnpp_time
    from oracle.precision import fp64
    dt = torch.float64 if f64 else torch.float32
    with fp64() if f64 else contextlib.nullcontext():
        P = {k: torch.from_numpy(v).to(dt).requires_grad_(True) for k, v in sd.items()}
        y = ncsnpp_time(P, torch.from_numpy(x).to(dt), torch.from_numpy(cn).to(dt), n_fft, hop, tuple(ch_mult), num_res_blocks, fir=fir)
        (y * torch.from_numpy(cot).to(dt)).sum().backward()
    return {k: v.grad.double().numpy() for k, v in P.items()}


def kind_of(name, shape):
    if "GroupNorm" in name or (len(shape) == 1 and name.endswith(".weight")):
        return "GN"
    if name.endswith("bias") or name.endswith(".b"):
        return "bias"
    if "Dense_0" in name or name in ("all_modules.1.weight", "all_modules.2.weight"):
        return "Dense"
    if len(shape) == 4 and shape[2] == 3:
        return "3x3"
    return "1x1"


GEOMS = {
    "small": dict(ch_mult=(1, 2, 2, 2), num_res_blocks=1, fir=False),
    "small_fir": dict(ch_mult=(1, 2, 2, 2), num_res_blocks=1, fir=True),
    "cm12_rb2": dict(ch_mult=(1, 2), num_res_blocks=2, fir=False),
}


@pytest.mark.parametrize("gemm,geom", [("fp32", "small"), ("bf16x3", "small"), ("f16x2", "small"), ("f16x2", "small_fir"), ("f16x2", "cm12_rb2")])
def test_param_grads_vs_fp64(gemm, geom):
    g = GEOMS[geom]
    n_fft, hop, L, B = 126, 32, 4096, 2
    net, sd = build(gemm=gemm, **g)
    x, cn, cot = inputs(B, L)
    got = gpu_grads(net, x, cn, cot)
    ref = ref_grads(sd, x, cn, cot, n_fft, hop, g["ch_mult"], g["num_res_blocks"], g["fir"])
    assert got["all_modules.0.W"] is None, "the Fourier projection W must get no gradient"
    worst, bad, num, den = {}, [], 0.0, 0.0
    for name, r in ref.items():
        if name == "all_modules.0.W":
            continue
        a = got[name]
        assert a is not None and a.shape == r.shape, name
        scale = np.abs(r).max()
        if name.endswith("NIN_1.b"):
            # the key bias shifts every score of a query row by the same amount: softmax cancels it, its exact gradient is 0.  Measured against the
            # scale of the block's query-bias gradient instead
            scale = np.abs(ref[name[:-len("NIN_1.b")] + "NIN_0.b"]).max()
        if r.shape == (2,) and name.startswith("all_modules."):          # a C -> 2 pyramid head's bias (see the module docstring)
            scale = max(scale, np.abs(ref[name[:-len("bias")] + "weight"]).max())
        e = np.abs(a - r).max() / (scale + 1e-30)
        k = kind_of(name, r.shape)
        if e > worst.get(k, (0.0, ""))[0]:
            worst[k] = (e, name)
        if e > TOL:
            bad.append((name, e))
        num += float(((a - r) ** 2).sum()); den += float((r ** 2).sum())
    snr = 10 * math.log10(den / max(num, 1e-300))
    print(f"\n[{gemm} {geom}] gradient accuracy vs float64: {snr:.1f} dB; worst per kind: " +
          ", ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in sorted(worst.items())))
    assert not bad, f"parameter gradients off (name, rel): {sorted(bad, key=lambda t: -t[1])[:8]}"


def _lib_vjps(net, x, cn, cot, B, L):
    """(grad_x of buddy_ncsnpp_vjp, grad_x and flat grad_params of buddy_ncsnpp_vjp_params) after the same save = 2 forward"""
    from buddy_amd import _lib
    lib = _lib.require_gpu()
    h = net._get_handle()
    xd, cnd, cotd = (torch.from_numpy(v).cuda() for v in (x, cn, cot))
    y = torch.empty_like(xd)
    out = []
    for params in (False, True, True):
        _lib.check(lib.buddy_ncsnpp_forward(h, _lib.ptr(xd), _lib.ptr(cnd), None, None, None, _lib.ptr(y), B, L, 2, _lib.stream_ptr()))
        gx = torch.empty_like(xd)
        if params:
            gp = torch.empty(net._n_params, device="cuda")
            _lib.check(lib.buddy_ncsnpp_vjp_params(h, _lib.ptr(cotd), _lib.ptr(gx), _lib.ptr(gp), 0, _lib.stream_ptr()))
            out.append((gx.cpu().numpy(), gp.cpu().numpy()))
        else:
            _lib.check(lib.buddy_ncsnpp_vjp(h, _lib.ptr(cotd), _lib.ptr(gx), _lib.stream_ptr()))
            out.append((gx.cpu().numpy(), None))
    torch.cuda.synchronize()
    return out


def test_determinism_batching_and_accumulate():
    net, _ = build()
    B, L = 2, 4096
    x, cn, cot = inputs(B, L)
    (gx0, _), (gx1, gp1), (gx2, gp2) = _lib_vjps(net, x, cn, cot, B, L)
    assert np.array_equal(gx0, gx1), "grad_x of vjp_params differs from buddy_ncsnpp_vjp"
    assert np.array_equal(gp1, gp2), "two parameter VJPs are not bit-identical"
    assert np.array_equal(gx1, gx2)
    # accumulate = 1 adds into the buffer (here: onto the same gradient, so exactly twice it)
    from buddy_amd import _lib
    lib = _lib.require_gpu()
    xd, cnd, cotd = (torch.from_numpy(v).cuda() for v in (x, cn, cot))
    y = torch.empty_like(xd)
    gp = torch.from_numpy(gp1).cuda()
    _lib.check(lib.buddy_ncsnpp_forward(net._get_handle(), _lib.ptr(xd), _lib.ptr(cnd), None, None, None, _lib.ptr(y), B, L, 2, _lib.stream_ptr()))
    _lib.check(lib.buddy_ncsnpp_vjp_params(net._get_handle(), _lib.ptr(cotd), None, _lib.ptr(gp), 1, _lib.stream_ptr()))
    assert np.array_equal(gp.cpu().numpy(), 2 * gp1), "accumulate = 1 does not add into grad_params"
    # the Fourier W gets zero
    assert not gp1[net._offsets[0][0]:net._offsets[0][0] + net._offsets[0][1]].any()
    # B = 2 equals the sum of the two B = 1 gradients
    s = None
    for b in range(B):
        _, (_, gpb), _ = _lib_vjps(net, x[b:b + 1], cn[b:b + 1], cot[b:b + 1], 1, L)
        s = gpb.astype(np.float64) if s is None else s + gpb
    for (off, n), (name, *_) in zip(net._offsets, net._specs):
        r = s[off:off + n]
        e = np.abs(gp1[off:off + n] - r).max() / (np.abs(r).max() + 1e-30) if n else 0.0
        assert e < TOL, f"{name}: B = 2 vs sum of B = 1: {e}"
    # torch accumulate semantics: two backward passes add into .grad
    g1 = gpu_grads(net, x, cn, cot)
    y = net(torch.from_numpy(x).cuda(), torch.from_numpy(cn).cuda())
    (y * torch.from_numpy(cot).cuda()).sum().backward()
    for n, p in net.named_parameters():
        if g1[n] is None:
            assert p.grad is None
            continue
        assert np.allclose(p.grad.cpu().double().numpy(), 2 * g1[n], rtol=1e-6, atol=1e-6 * np.abs(g1[n]).max()), n


def test_freshness_after_adam_and_replicas():
    net, _ = build()
    B, L = 2, 4096
    x, cn, cot = inputs(B, L)
    xd, cnd = torch.from_numpy(x).cuda(), torch.from_numpy(cn).cuda()
    rep = net.replica()
    with torch.no_grad():
        y_rep0 = rep(xd, cnd).clone()                 # the replica's handle shares the store
    net.requires_grad_(True)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    y = net(xd, cnd)
    (y * torch.from_numpy(cot).cuda()).sum().backward()
    # a forward the replica saved before the update cannot be differentiated after it
    xr = xd.clone().requires_grad_(True)
    yr = rep(xr, cnd)
    opt.step()
    with torch.no_grad():
        y_new = net(xd, cnd).clone()
    fresh, _ = build()
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        y_fresh = fresh(xd, cnd)
    assert torch.equal(y_new, y_fresh), "the forward after Adam.step differs from a module that loaded the updated state_dict"
    assert not torch.equal(y_new, y_rep0)
    from buddy_amd import _lib
    with pytest.raises(_lib.BuddyHipError):
        yr.sum().backward()
    with torch.no_grad():
        y_rep1 = rep(xd, cnd)
    assert torch.equal(y_rep1, y_new), "a replica does not see the weights its parent pushed to the shared store"
    # EMA copy (reference trainer: deepcopy + in-place lerp) follows its own parameters
    ema = copy.deepcopy(net).requires_grad_(False)
    with torch.no_grad():
        assert torch.equal(ema(xd, cnd), y_new)
        for pe, pn in zip(ema.parameters(), net.parameters()):
            pe.copy_(pn.detach().lerp(pe, 0.5) * 0.999)
        y_ema = ema(xd, cnd).clone()
    fresh.load_state_dict(ema.state_dict())
    with torch.no_grad():
        assert torch.equal(y_ema, fresh(xd, cnd))


def test_short_training_run_vs_fp64():
    from types import SimpleNamespace
    from buddy_amd.diff_params.edm import EDM
    from oracle.ncsnpp_ref import ncsnpp_time
    g = GEOMS["small"]
    n_fft, hop, L, B = 126, 32, 4096, 2
    net, sd = build(gemm="fp32", **g)
    net.requires_grad_(True)
    edm = EDM("ve_karras", SimpleNamespace(sigma_data=0.05, sigma_min=1e-5, sigma_max=10, rho=10))
    rs = np.random.RandomState(7)
    x = (0.05 * rs.standard_normal((B, L))).astype(np.float32)
    n = rs.standard_normal((B, L)).astype(np.float32)
    t = np.array([0.02, 0.3], dtype=np.float32)
    P = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
    P["all_modules.0.W"].requires_grad_(False)
    ref_net = lambda inp, cnoise: ncsnpp_time(P, inp[:, 0], cnoise, n_fft, hop, g["ch_mult"], g["num_res_blocks"])[:, None]
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    opt_ref = torch.optim.Adam([v for v in P.values() if v.requires_grad], lr=1e-4)
    names = [k for k, _ in net.named_parameters()]
    for step in range(5):
        loss, _ = edm.loss_fn(net, torch.from_numpy(x).cuda(), torch.from_numpy(n).cuda(), t=torch.from_numpy(t))
        loss = loss.mean()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
        loss_r, _ = edm.loss_fn(ref_net, torch.from_numpy(x).double(), torch.from_numpy(n).double(), t=torch.from_numpy(t).double())
        loss_r = loss_r.mean()
        opt_ref.zero_grad()
        loss_r.backward()
        torch.nn.utils.clip_grad_norm_([v for v in P.values() if v.requires_grad], 1.0)
        opt_ref.step()
        el = abs(float(loss) - float(loss_r)) / abs(float(loss_r))
        assert el < 1e-4, f"step {step}: loss {float(loss)} vs {float(loss_r)}"
        sdn = dict(net.named_parameters())
        for k in names:
            a, r = sdn[k].detach().cpu().double(), P[k].detach()
            e = float((a - r).norm() / (r.norm() + 1e-30))
            assert e < 1e-4, f"step {step}: {k} differs by {e:.2e} (relative norm)"
