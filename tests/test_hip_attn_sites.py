"""GPU parity of the NCSN++ attention sites (``attn_resolutions``) against fixtures recorded from the reference
(tests/golden/make_golden_attn.py), and of the head-width-32 flash kernels they bring in against an fp64 restatement.
Tolerances are those of tests/test_hip_network.py: 5e-4 of the abs-max on output and input-VJP, 2e-3 on the per-module statistics."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 5e-4


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def build(g, gemm=None, attention=None):
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
    return net.cuda().eval()


def _check_net(g, net):
    x = torch.from_numpy(g["x"]).cuda().requires_grad_(True)
    y = net(x, torch.from_numpy(g["cnoise"]).cuda())
    bad, n = [], 0
    for k in sorted(g.files):
        if k.startswith("tap") and k.endswith("_absmax"):
            i = int(k[3:-7]); t = net.tap(i); n += 1
            if abs(float(t.abs().max()) - float(g[k])) > 2e-3 * float(g[k]) or abs(float(t.std()) - float(g[f"tap{i}_std"])) > 2e-3 * float(g[f"tap{i}_std"]):
                bad.append((i, float(t.abs().max()), float(g[k])))
    assert n >= 12 and not bad, f"per-module statistics off (idx, absmax, ref): {bad[:6]}"
    gx, = torch.autograd.grad(y, x, torch.from_numpy(g["cot"]).cuda())
    return rel(y.detach().cpu().numpy(), g["y"]), rel(gx.cpu().numpy(), g["vjp"])


@pytest.mark.parametrize("attention", ["auto", "matrix", "flash"])
@pytest.mark.parametrize("gemm", ["f16x2", "bf16x3", "fp32"])
@pytest.mark.parametrize("name", ["net_attn_lo", "net_attn_hi", "net_full_attn"])
def test_attention_sites_vs_golden(golden, name, gemm, attention):
    """every site of the reference's module list (taps at its module indices), forward and input-VJP, in every GEMM arithmetic and every fp32
    attention form.  net_attn_hi: level-0 sites at C = 32 over 144 x 64 tokens (flash C = 32 in auto; the T x T matrix, 340 MB per utterance, in
    matrix)."""
    g = golden(name)
    ey, eg = _check_net(g, build(g, gemm=gemm, attention=attention))
    print(name, gemm, attention, f"forward {ey:.2e} vjp {eg:.2e}")
    assert ey < TOL and eg < TOL


def test_attention_sites_f16_mode_full(golden):
    """the opt-in 16-bit attention at the full width (C = 256 sites + bottleneck): the bound of test_attention_modes_vs_golden (f16)"""
    g = golden("net_full_attn")
    ey, eg = _check_net(g, build(g, attention="f16"))
    print("net_full_attn f16", f"forward {ey:.2e} vjp {eg:.2e}")
    assert ey < 1e-3 and eg < 1e-3


def test_c32_sites_in_16bit_mode_run_fp32(golden):
    """a C = 32 site has no 16-bit kernel: in attention = bf16 it runs the fp32 flash kernels (the C = 64 sites and the bottleneck run bf16)"""
    g = golden("net_attn_hi")
    ey, eg = _check_net(g, build(g, attention="bf16"))
    print("net_attn_hi bf16", f"forward {ey:.2e} vjp {eg:.2e}")
    assert ey < 5e-3 and eg < 5e-3


def test_attention_sites_row_independence(golden):
    """row 0 of a B = 2 call equals the B = 1 call bit for bit (flash C = 32 split rule depends on T alone)"""
    g = golden("net_attn_hi")
    net = build(g, attention="auto")
    x = torch.from_numpy(g["x"]).cuda()
    cn = torch.from_numpy(g["cnoise"]).cuda()
    cot = torch.from_numpy(g["cot"]).cuda()
    out = []
    for xb, cb, gb in ((x, cn, cot), (x[:1], cn[:1], cot[:1])):
        xb = xb.clone().requires_grad_(True)
        y = net(xb, cb)
        gx, = torch.autograd.grad(y, xb, gb)
        out.append((y.detach()[0].cpu(), gx[0].cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_attention_site_without_flash_kernel_refused():
    """a site whose width has no flash kernel (C = 512) over more than 4096 tokens: argument error, no multi-GB matrix"""
    import ctypes as C
    from buddy_amd import _lib
    from buddy_amd.synth import module_specs
    lib = _lib.require_gpu()
    cm = (C.c_int * 2)(4, 4)
    specs = module_specs(128, (4, 4), 1, attn_mask=0b01)
    blob = np.zeros(sum(int(np.prod(s)) for _, s, *_ in specs), np.float32)
    h = C.c_void_p()
    _lib.check(lib.buddy_ncsnpp_create_attn(blob.ctypes.data, blob.size, 128, cm, 2, 1, 510, 128, 0b01, C.byref(h)))
    try:
        x = torch.zeros(1, 16000, device="cuda")
        y = torch.empty_like(x)
        cn = torch.zeros(1, device="cuda")
        rc = lib.buddy_ncsnpp_forward(h, x.data_ptr(), cn.data_ptr(), None, None, None, y.data_ptr(), 1, 16000, 0, torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and b"no flash kernel" in lib.buddy_last_error()
        # short input: 16 x 256 = 4096 tokens, the materialised form
        x = torch.zeros(1, 1920, device="cuda")
        y = torch.empty_like(x)
        _lib.check(lib.buddy_ncsnpp_forward(h, x.data_ptr(), cn.data_ptr(), None, None, None, y.data_ptr(), 1, 1920, 0, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    finally:
        lib.buddy_ncsnpp_destroy(h)


def _attn_ref64(q, k, v, dO, scale, chunk=2048):
    """fp64 attention and its three input gradients, query rows in chunks (no B x T x T tensor at T = 32768)"""
    B, T, Cc = q.shape
    qd, kd, vd, dd = (t.double() for t in (q, k, v, dO))
    O = torch.empty_like(qd); lse = torch.empty(B, T, dtype=torch.float64, device=q.device)
    dq = torch.empty_like(qd); dk = torch.zeros_like(qd); dv = torch.zeros_like(qd)
    for b in range(B):
        for i0 in range(0, T, chunk):
            s = qd[b, i0:i0 + chunk] @ kd[b].T * scale
            lse[b, i0:i0 + chunk] = torch.logsumexp(s, dim=-1)
            p = torch.exp(s - lse[b, i0:i0 + chunk, None])
            o = p @ vd[b]
            O[b, i0:i0 + chunk] = o
            dp = dd[b, i0:i0 + chunk] @ vd[b].T
            ds = p * (dp - (dd[b, i0:i0 + chunk] * o).sum(-1, keepdim=True)) * scale
            dq[b, i0:i0 + chunk] = ds @ kd[b]
            dk[b] += ds.T @ qd[b, i0:i0 + chunk]
            dv[b] += p.T @ dd[b, i0:i0 + chunk]
    return O, lse, dq, dk, dv


def _rel_t(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize("B,T", [(2, 144), (3, 1000), (2, 8256), (1, 32768)])
def test_flash_attention_c32_vs_fp64(B, T):
    """head width 32 (its own kernels: 2 waves x 32 rows, 64-key blocks) through buddy_flash_attention_{fwd,bwd}[_split]: the unsplit form, the
    count the network picks and two forced counts against the fp64 restatement; ragged T; bounds of the C in {64, 128, 256} kernels"""
    from buddy_amd import _lib
    lib = _lib.require_gpu()
    Cc = 32
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + T + 32)
    q, k, v, dO = (torch.randn(B, T, Cc, generator=g).cuda() for _ in range(4))
    q = q * 1.5
    scale = Cc ** -0.5
    ref = _attn_ref64(q, k, v, dO, scale)
    P = lambda t: None if t is None else t.data_ptr()                      # noqa: E731
    S = torch.cuda.current_stream().cuda_stream
    nb = (T + 31) // 32
    picked = lib.buddy_flash_attention_splits(B, T)
    counts = sorted({0, picked, 2, 3} - {1} if nb >= 3 else {0})
    results = {}
    for ns in counts:
        O = torch.empty_like(q); lse = torch.empty(B, T, device="cuda")
        dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        delta = torch.empty(B, T, device="cuda")
        if ns == 0:
            _lib.check(lib.buddy_flash_attention_fwd(P(q), P(k), P(v), P(O), P(lse), B, T, Cc, scale, 0, S))
            _lib.check(lib.buddy_flash_attention_bwd(P(q), P(k), P(v), P(O), P(dO), P(lse), P(delta), P(dq), P(dk), P(dv), B, T, Cc, scale, 0, S))
        else:
            ws = torch.empty(max(lib.buddy_flash_attention_workspace(B, T, Cc, ns), 1), device="cuda")
            _lib.check(lib.buddy_flash_attention_fwd_split(P(q), P(k), P(v), P(O), P(lse), B, T, Cc, scale, ns, P(ws), S))
            _lib.check(lib.buddy_flash_attention_bwd_split(P(q), P(k), P(v), P(O), P(dO), P(lse), P(delta), P(dq), P(dk), P(dv), B, T, Cc, scale, ns,
                                                           P(ws), S))
        torch.cuda.synchronize()
        results[ns] = (O, lse, dq, dk, dv)
        errs = dict(O=_rel_t(O, ref[0]), lse=float((lse.double() - ref[1]).abs().max()), dq=_rel_t(dq, ref[2]), dk=_rel_t(dk, ref[3]),
                    dv=_rel_t(dv, ref[4]))
        print((B, T, ns), {k_: f"{v_:.1e}" for k_, v_ in errs.items()})
        tf, tb = (1e-5, 2e-5) if T <= 8256 else (2e-5, 5e-5)          # fp32 sums over 32768 keys: measured up to 1.4e-5 / 2.0e-5
        assert errs["O"] < tf and errs["lse"] < 1e-4 and errs["dq"] < tb and errs["dk"] < tb and errs["dv"] < tb
    # the 16-bit entries have no C = 32 kernel
    assert lib.buddy_flash_attention16_workspace(B, T, Cc) == 0
    ws16 = torch.empty(16, device="cuda")
    O = torch.empty_like(q); lse = torch.empty(B, T, device="cuda")
    assert lib.buddy_flash_attention16_fwd(P(q), P(k), P(v), P(O), P(lse), B, T, Cc, scale, 2, P(ws16), S) != 0


def test_e2e_blind_attn_vs_reference_fixture(golden):
    """the blind sampler (product sampler, HIP operator) on a network with network.attn_resolutions=[32] against the reference's own run: the
    tolerance of test_blind_dps_vs_reference_fixture"""
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.synth import synth_state_dict
    from buddy_amd.testing.operators.subband_filtering import BlindSubbandFiltering
    from buddy_amd.utils.metrics import si_sdr
    from oracle.sampler_ref import NoiseStream
    g = golden("e2e_blind_attn")
    meta = [int(v) for v in g["meta"]]
    nf, L, T, order, seed = meta[:5]
    args = compose(tester="blind_dereverberation_BUDDy",
                   overrides=[f"tester.sampling_params.T={T}", f"tester.sampling_params.order={order}", f"network.nf={nf}", "network.attn_resolutions=[32]",
                              "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "tester.posterior_sampling.blind_hp.op_updates_per_step=3"])
    net = instantiate(args.network)
    assert net.attn_mask == 0b1000
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(seed, nf, attn_mask=net.attn_mask).items()})
    net = net.cuda().eval()
    edm = instantiate(args.diff_params)
    ns = [NoiseStream(meta[6])]
    smp = instantiate(args.tester.sampler, net, edm, args)
    op = BlindSubbandFiltering(args.tester.informed_dereverberation.op_hp, 16000, num_utts=1, noise=ns, device="cuda", length=L)
    smp.noise = ns
    op.update_H(use_noise=True)
    pred = smp.predict_conditional(torch.from_numpy(g["y"]).cuda(), op, shape=(1, L), blind=True)
    assert ns[0].k == int(g["n_draws"])
    p = pred.cpu().numpy()

    def sisdr(a, b):
        return float(si_sdr(torch.as_tensor(a).reshape(1, -1), torch.as_tensor(b).reshape(1, -1)))
    print(f"blind run with attention sites vs the reference: rel {rel(p, g['pred']):.2e}, SI-SDR {sisdr(p, g['pred']):.1f} dB")
    assert rel(p, g["pred"]) < 3e-3
    assert sisdr(p, g["pred"]) > 40.0
    assert abs(sisdr(p, g["clean"]) - sisdr(g["pred"], g["clean"])) < 0.1
    assert rel(op.params[0][0].detach().cpu().numpy(), g["decay"]) < 3e-2
    assert rel(op.params[1][0].detach().cpu().numpy(), g["weights"]) < 3e-2
    assert rel(smp.operator.get_time_RIR().detach().cpu().numpy(), g["est_rir"]) < 3e-2
