"""GPU parity of the hand-written NCSN++ (forward and input-VJP) through the C-ABI against
(a) golden fixtures recorded from the reference and (b) the CPU oracle on the same seeded inputs.
Tolerance (stated): relative-to-absmax 5e-4 on network outputs / VJPs in fp32 (the reference itself differs from
its own CPU re-run by ~1e-5 with different thread counts; 64 chained convs with K up to 4608 accumulate
summation-order round-off of ~1e-4)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 5e-4


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def build(nf, n_fft, hop, seed, fir=False, attention=None, gemm=None, ch_mult=(1, 2, 2, 2), num_res_blocks=1):
    from buddy_amd.config import load_yaml, CONF_DIR, AttrDict
    from buddy_amd.networks.ncsnpp import NCSNppTime
    from buddy_amd.synth import synth_state_dict
    cfg = load_yaml(os.path.join(CONF_DIR, "network", "ncsnpp.yaml"))
    cfg.pop("_target_")
    cfg.update(nf=nf, fir=fir, attention=attention, gemm=gemm, ch_mult=list(ch_mult), num_res_blocks=num_res_blocks,
               stft=AttrDict(n_fft=n_fft, hop_length=hop, center=True))
    net = NCSNppTime(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(seed, nf, tuple(ch_mult), num_res_blocks).items()})
    return net.cuda().eval()


@pytest.mark.parametrize("name", ["net_small", "net_full", "net_small_fir"])
def test_forward_vjp_vs_golden(golden, name):
    """net_small_fir: the same small network built with fir=True (FIR (1,3,3,1) resampling in the up / down blocks and both pyramids,
    reference up_or_down_sampling.py:195-257), fixture recorded through the reference's pure-PyTorch upfirdn2d."""
    g = golden(name)
    nf, n_fft, hop, L, B, seed = [int(v) for v in g["meta"]]
    net = build(nf, n_fft, hop, seed, fir=name.endswith("_fir"))
    x = torch.from_numpy(g["x"]).cuda().requires_grad_(True)
    y = net(x, torch.from_numpy(g["cnoise"]).cuda())
    report = []
    for k in sorted(g.files):
        if k.startswith("tap") and k.endswith("_absmax"):
            i = int(k[3:-7])
            t = net.tap(i)
            report.append((i, float(t.abs().max()), float(g[k]), float(t.std()), float(g[f"tap{i}_std"])))
    bad = [r for r in report if abs(r[1] - r[2]) > 2e-3 * r[2] or abs(r[3] - r[4]) > 2e-3 * r[4]]
    assert not bad, f"per-module statistics off (idx, absmax, ref, std, ref): {bad[:6]}"
    e = rel(y.detach().cpu().numpy(), g["y"])
    assert e < TOL, f"forward rel err {e}"
    gx, = torch.autograd.grad(y, x, torch.from_numpy(g["cot"]).cuda())
    e = rel(gx.cpu().numpy(), g["vjp"])
    assert e < TOL, f"vjp rel err {e}"


@pytest.mark.parametrize("attention", ["matrix", "flash"])
@pytest.mark.parametrize("gemm", ["f16x2", "bf16x3", "fp32"])
@pytest.mark.parametrize("name", ["net_cm12_rb2", "net_cm1122_rb1"])
def test_architecture_family_vs_golden(golden, name, gemm, attention):
    """The constructor is parametric (reference networks/ncsnpp.py:50-52,184-270: ch_mult, num_res_blocks, nf); csrc/net.hip builds the module list
    for any level / block count.  Two members besides the shipped (1, 2, 2, 2) / 1 block, recorded from the reference: forward, input-VJP and the
    per-module statistics, in both GEMM arithmetics and both fp32 attention forms."""
    g = golden(name)
    nf, n_fft, hop, L, B, seed = [int(v) for v in g["meta"]]
    ch_mult, nrb = tuple(int(c) for c in g["ch_mult"]), int(g["num_res_blocks"])
    net = build(nf, n_fft, hop, seed, gemm=gemm, attention=attention, ch_mult=ch_mult, num_res_blocks=nrb)
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
    ey, eg = rel(y.detach().cpu().numpy(), g["y"]), rel(gx.cpu().numpy(), g["vjp"])
    print(name, gemm, attention, f"forward {ey:.2e} vjp {eg:.2e}")
    assert ey < TOL and eg < TOL


@pytest.mark.parametrize("attention,tol", [("matrix", TOL), ("flash", TOL), ("f16", 1e-3), ("bf16", 5e-3)])
def test_attention_modes_vs_golden(golden, attention, tol):
    """NCSNppTime(attention=...): the materialised form and the online-softmax kernels hold the fp32 tolerance; the opt-in 16-bit-operand
    variants are stated at 1e-3 (f16) / 5e-3 (bf16) of the output peak on the full-width fixture (one attention block in a 36-module network)."""
    g = golden("net_full")
    nf, n_fft, hop, L, B, seed = [int(v) for v in g["meta"]]
    net = build(nf, n_fft, hop, seed, attention=attention)
    x = torch.from_numpy(g["x"]).cuda().requires_grad_(True)
    y = net(x, torch.from_numpy(g["cnoise"]).cuda())
    gx, = torch.autograd.grad(y, x, torch.from_numpy(g["cot"]).cuda())
    ey, eg = rel(y.detach().cpu().numpy(), g["y"]), rel(gx.cpu().numpy(), g["vjp"])
    print(attention, f"forward {ey:.2e} vjp {eg:.2e}")
    assert ey < tol and eg < tol


def test_forward_vjp_vs_oracle_batched_fused_edm():
    """B=3 with different sigmas; EDM scalars folded into the kernels vs oracle EDM denoiser."""
    from oracle import ncsnpp_ref
    from oracle.sampler_ref import EDMRef
    from buddy_amd.config import AttrDict
    from buddy_amd.synth import synth_state_dict
    nf, L, B, seed = 32, 6000, 3, 11
    net = build(nf, 510, 128, seed)
    P = ncsnpp_ref.to_torch(synth_state_dict(seed, nf))
    rs = np.random.RandomState(0)
    x = torch.from_numpy((0.3 * rs.standard_normal((B, L))).astype(np.float32))
    cot = torch.from_numpy(rs.standard_normal((B, L)).astype(np.float32))
    sig = torch.tensor([0.4, 0.02, 0.003])
    edm = EDMRef(AttrDict(sigma_data=0.05))
    xr = x.clone().requires_grad_(True)
    ys = []
    for b in range(B):
        f = lambda z, cn: ncsnpp_ref.ncsnpp_time(P, z, cn, 510, 128)
        ys.append(edm.denoiser(xr[b:b + 1, None], f, sig[b])[:, 0])
    yr = torch.cat(ys)
    gr, = torch.autograd.grad(yr, xr, cot)
    xg = x.cuda().requires_grad_(True)
    s = sig.cuda()
    y = net.denoise_fused(xg, edm.cnoise(s), edm.cin(s), edm.cskip(s), edm.cout(s))
    gx, = torch.autograd.grad(y, xg, cot.cuda())
    assert rel(y.detach().cpu().numpy(), yr.detach().numpy()) < TOL
    assert rel(gx.cpu().numpy(), gr.numpy()) < TOL


@pytest.mark.parametrize("nf,ch_mult,L", [(128, (1, 3), 1000), (256, (1, 2), 1000), (128, (3, 3), 500)])
def test_wide_levels_vs_oracle(nf, ch_mult, L):
    """Level widths of 384 and 512 channels (96 and 128 channel quads: no power of two of at most 64): forward and input-VJP against the float64
    oracle on synth weights; n_fft = 126, hop = 32, B = 2, the default attention.  With (1, 3) and (1, 2) the wide level is the last one: its
    pyramid head runs the 3 x 3 Cin -> 2 convolution at 384 / 512 channels, its bottleneck attention the materialised form.  The Combine of the
    input pyramid sits between two levels and has the width of the upper one, so (3, 3) is the network whose input-VJP runs the one-tap Cin -> 2
    convolution at 384 channels (L = 500: 16 frames)."""
    from oracle import ncsnpp_ref
    from oracle.precision import fp64
    from buddy_amd.synth import synth_state_dict
    n_fft, hop, B, seed = 126, 32, 2, 21
    net = build(nf, n_fft, hop, seed, ch_mult=ch_mult)
    sd = synth_state_dict(seed, nf, tuple(ch_mult), 1)
    rs = np.random.RandomState(nf)
    x = (0.3 * rs.standard_normal((B, L))).astype(np.float32)
    cot = rs.standard_normal((B, L)).astype(np.float32)
    cn = np.array([-0.8, -0.2], dtype=np.float32)
    with fp64():
        Pr = ncsnpp_ref.to_torch(sd)
        xr = torch.from_numpy(x).double().requires_grad_(True)
        yr = ncsnpp_ref.ncsnpp_time(Pr, xr, torch.from_numpy(cn).double(), n_fft, hop, tuple(ch_mult), 1)
        gr, = torch.autograd.grad(yr, xr, torch.from_numpy(cot).double())
    xg = torch.from_numpy(x).cuda().requires_grad_(True)
    y = net(xg, torch.from_numpy(cn).cuda())
    gx, = torch.autograd.grad(y, xg, torch.from_numpy(cot).cuda())
    ey, eg = rel(y.detach().cpu().numpy(), yr.detach().numpy()), rel(gx.cpu().numpy(), gr.numpy())
    print(f"wide levels nf={nf} ch_mult={ch_mult}: forward {ey:.2e} vjp {eg:.2e}")
    assert ey < TOL and eg < TOL


def test_batch_independence_and_determinism():
    """per-utterance semantics: row b of a batched call equals the B=1 call bit-for-bit; repeated calls are bit-identical."""
    net = build(32, 510, 128, 2)
    rs = np.random.RandomState(1)
    x = torch.from_numpy((0.3 * rs.standard_normal((4, 8192))).astype(np.float32)).cuda()
    cn = torch.tensor([-1.0, -0.5, 0.1, -2.0], device="cuda")
    with torch.no_grad():
        y = net(x, cn)
        y2 = net(x, cn)
        y1 = torch.cat([net(x[b:b + 1], cn[b:b + 1]) for b in range(4)])
    assert torch.equal(y, y2)
    assert torch.equal(y, y1)


def test_f16x2_utterance_does_not_depend_on_its_batch():
    """Full width (the f16x2 batched GEMMs run: 128 / 256 channels), utterances FOUR DECADES apart in level in one batch: the power-of-two scale of the
    transformed inputs is per utterance (abs-max collected by the input transform), so row b of the batched forward + VJP equals the B = 1 call bit for bit,
    whatever shares the batch; and the quiet utterance keeps its accuracy (against the fp32-MFMA handle, relative to ITS abs-max)."""
    net = build(128, 510, 128, 3)
    assert net.get_option("gemm") == 2                      # the library default
    ref = build(128, 510, 128, 3, gemm="fp32")
    rs = np.random.RandomState(4)
    x = torch.from_numpy((0.3 * rs.standard_normal((3, 16000))).astype(np.float32))
    x[1] *= 1e-2; x[2] *= 1e2
    cot = torch.from_numpy(rs.standard_normal((3, 16000)).astype(np.float32)).cuda()
    cn = torch.tensor([-1.0, -0.5, 0.1], device="cuda")
    def run(n, xs, cs, ct):
        xg = xs.cuda().requires_grad_(True)
        y = n(xg, cs)
        g, = torch.autograd.grad(y, xg, ct)
        return y.detach(), g
    y, g = run(net, x, cn, cot)
    for b in range(3):
        y1, g1 = run(net, x[b:b + 1], cn[b:b + 1], cot[b:b + 1])
        assert torch.equal(y[b:b + 1], y1) and torch.equal(g[b:b + 1], g1), b
    alt = net.replica()
    alt.set_option("wgemm_rt", 1)                           # the 32-row-per-wave kernel: another tiling of the same sums in the same order
    ya, ga = run(alt, x, cn, cot)
    assert torch.equal(y, ya) and torch.equal(g, ga)
    yr, gr = run(ref, x, cn, cot)
    for b in range(3):
        ey, eg = rel(y[b].cpu().numpy(), yr[b].cpu().numpy()), rel(g[b].cpu().numpy(), gr[b].cpu().numpy())
        print(f"utterance {b} (level {float(x[b].abs().max()):.1e}): f16x2 vs fp32 MFMA forward {ey:.2e} vjp {eg:.2e}")
        assert ey < TOL and eg < TOL


@pytest.mark.parametrize("gemm", ["f16x2", "bf16x3", "fp32"])
def test_gemm_modes_vs_golden(golden, gemm):
    """NCSNppTime(gemm=...): the Winograd-domain GEMMs in f16x2 arithmetic (default: two-term f16 split of power-of-two-scaled operands, three f16 MFMA
    products), in bf16x3 arithmetic (exact three-way bf16 split, six bf16 MFMA products) and on
    the fp32 MFMA hold the SAME tolerance against the full-width reference fixture; both errors are printed side by side."""
    g = golden("net_full")
    nf, n_fft, hop, L, B, seed = [int(v) for v in g["meta"]]
    net = build(nf, n_fft, hop, seed, gemm=gemm)
    x = torch.from_numpy(g["x"]).cuda().requires_grad_(True)
    y = net(x, torch.from_numpy(g["cnoise"]).cuda())
    gx, = torch.autograd.grad(y, x, torch.from_numpy(g["cot"]).cuda())
    ey, eg = rel(y.detach().cpu().numpy(), g["y"]), rel(gx.cpu().numpy(), g["vjp"])
    print(f"gemm={gemm}: forward {ey:.2e} vjp {eg:.2e}")
    assert ey < TOL and eg < TOL


@pytest.mark.parametrize("gemm", ["f16x2", "bf16x3", "fp32"])
def test_full_size_vs_reference_fixture(golden, gemm):
    """SURVEY 8(c).3 / VERDICT r5 item 3: the FULL size against the reference itself (not only against the oracle): nf = 128, STFT 510 / 128,
    L = 64 000 = BASELINE configs[1]'s utterance (reference networks/ncsnpp.py:281-449, :498-506) -- forward, input-VJP and the per-module statistics,
    in all three GEMM arithmetics at the SAME 5e-4 bound; then the B = 2 fixture whose row 0 is that utterance: both rows against the reference's
    batched run, and row 0 bit-identical to the B = 1 call (an utterance's result does not depend on its batch)."""
    g = golden("net_full_64000")
    nf, n_fft, hop, L, B, seed = [int(v) for v in g["meta"]]
    assert (nf, L, B) == (128, 64000, 1)
    net = build(nf, n_fft, hop, seed, gemm=gemm)
    x = torch.from_numpy(g["x"]).cuda().requires_grad_(True)
    y = net(x, torch.from_numpy(g["cnoise"]).cuda())
    bad, n = [], 0
    for k in sorted(g.files):
        if k.startswith("tap") and k.endswith("_absmax"):
            i = int(k[3:-7]); t = net.tap(i); n += 1
            if abs(float(t.abs().max()) - float(g[k])) > 2e-3 * float(g[k]) or abs(float(t.std()) - float(g[f"tap{i}_std"])) > 2e-3 * float(g[f"tap{i}_std"]):
                bad.append((i, float(t.abs().max()), float(g[k])))
    assert n >= 18 and not bad, f"per-module statistics off (idx, absmax, ref): {bad[:6]}"
    gx, = torch.autograd.grad(y, x, torch.from_numpy(g["cot"]).cuda())
    ey, eg = rel(y.detach().cpu().numpy(), g["y"]), rel(gx.cpu().numpy(), g["vjp"])
    g2 = golden("net_full_64000_B2")
    assert np.array_equal(g2["x"][0], g["x"][0]) and g2["x"].shape[0] == 2
    x2 = torch.from_numpy(g2["x"]).cuda().requires_grad_(True)
    y2 = net(x2, torch.from_numpy(g2["cnoise"]).cuda())
    gx2, = torch.autograd.grad(y2, x2, torch.from_numpy(g2["cot"]).cuda())
    ey2, eg2 = rel(y2.detach().cpu().numpy(), g2["y"]), rel(gx2.cpu().numpy(), g2["vjp"])
    print(f"L = 64000 vs the reference, gemm={gemm}: B=1 forward {ey:.2e} vjp {eg:.2e}; B=2 forward {ey2:.2e} vjp {eg2:.2e}")
    assert ey < TOL and eg < TOL and ey2 < TOL and eg2 < TOL
    assert torch.equal(y2[0].detach(), y[0].detach()) and torch.equal(gx2[0], gx[0]), "row 0 of the batch differs from its B = 1 run"


def test_cold_start_budget_and_shared_replica():
    """a network handle must be cheap.  Full-width network (111 MB of parameters): buddy_ncsnpp_create + the first forward
    (which prepares, on the GPU, the ONE operand form each 3x3 convolution uses for this workload) under 1.5 s of wall time here (measured
    ~0.3 s; the bound leaves room for a cold driver), prepared weights < 1.3 GB for a forward-only handle and < 2.6 GB with the data-gradient
    forms of the VJP (round 3: 5.7 GB and ~7 s per handle); a replica shares all of it (no new bytes, no new forms) and returns the parent's
    output bit for bit."""
    import time
    net = build(128, 510, 128, 0)
    B, L = 2, 64000
    rs = np.random.RandomState(5)
    x = torch.from_numpy((0.3 * rs.standard_normal((B, L))).astype(np.float32)).cuda()
    cn = torch.tensor([-0.7, -0.1], device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        y = net(x, cn)
    torch.cuda.synchronize()
    cold = time.perf_counter() - t0
    wb = net.weight_bytes()
    assert cold < 1.5, f"handle creation + first forward took {cold:.2f} s"
    assert wb["conv3_forms"] < 1.3e9, wb
    n_fwd = wb["conv3_form_count"]
    xg = x.clone().requires_grad_(True)
    yg = net(xg, cn)
    g, = torch.autograd.grad(yg, xg, torch.ones_like(yg))
    torch.cuda.synchronize()
    wb2 = net.weight_bytes()
    assert wb2["conv3_forms"] < 2.6e9 and wb2["conv3_form_count"] <= 2 * n_fwd, wb2
    t0 = time.perf_counter()
    rep = net.replica()
    with torch.no_grad():
        yr = rep(x, cn)
    torch.cuda.synchronize()
    warm = time.perf_counter() - t0
    wb3 = rep.weight_bytes()
    assert wb3 == wb2, (wb2, wb3)
    assert torch.equal(yr, y)
    assert warm < 0.5, f"replica + its first forward took {warm:.2f} s"
    print(f"cold start {cold * 1e3:.0f} ms, replica first forward {warm * 1e3:.0f} ms, weight store {wb2}")


def test_round6_kernel_forms_equal_their_predecessors():
    """Round 6's kernel forms against the ones they replaced, full-width network, forward and input-VJP, two handles of the same weights in one process:
    the 1x1 / NIN / skip-path GEMMs in f16x2 with the running per-row scale (gen_f16x2, its 64-row and two-column-block forms gen_rows / gen_cp; predecessor:
    the exact bf16x3 split), non-temporal loads in the skip-path epilogue (gnb_nt) and the strip form of the C -> 2 convolutions (c2out_tiled = 2;
    predecessor 1).  Same function, other summation orders / a 2^-22 instead of a 2^-24 operand split in the 6 % of the FLOPs that are 1x1: 2e-5 of the
    abs-max (each side holds 5e-4 against the reference fixtures); the 32-row-only f16x2 form against the size-selected forms: bit-identical."""
    net = build(128, 510, 128, 0)
    old = net.replica().set_option("gen_f16x2", 0).set_option("gnb_nt", 0).set_option("c2out_tiled", 1)
    rows32 = net.replica().set_option("gen_rows", 32).set_option("gen_cp", 0)
    rs = np.random.RandomState(12)
    L, B = 32768, 2
    cn = torch.tensor([-0.3, -1.2]).cuda()
    cot = torch.from_numpy(rs.standard_normal((B, L)).astype(np.float32)).cuda()
    x0 = torch.from_numpy((0.3 * rs.standard_normal((B, L))).astype(np.float32)).cuda()
    outs = {}
    for tag, n in (("new", net), ("old", old), ("rows32", rows32)):
        x = x0.clone().requires_grad_(True)
        y = n(x, cn)
        g, = torch.autograd.grad(y, x, cot)
        outs[tag] = (y.detach().cpu().numpy(), g.cpu().numpy())
    ey, eg = rel(outs["new"][0], outs["old"][0]), rel(outs["new"][1], outs["old"][1])
    print(f"round-6 forms vs their predecessors: forward {ey:.2e}, vjp {eg:.2e}")
    assert not np.array_equal(outs["new"][1], outs["old"][1]), "the options did not change the path"
    assert ey < 2e-5 and eg < 2e-5, (ey, eg)
    # the three tilings of the f16x2 general form run the same per-row arithmetic in the same order (a row's scale depends on the row alone): bit-identical
    assert rows32.get_option("gen_rows") == 32 and rows32.get_option("gen_cp") == 0 and net.get_option("gen_rows") == 0
    assert np.array_equal(outs["new"][0], outs["rows32"][0]) and np.array_equal(outs["new"][1], outs["rows32"][1])


def test_fused_round4_paths_equal_plain_paths():
    """The two structural fusions of round 4 -- the up blocks' Conv_0 in sub-pixel form (option upconv) and the skip path's 1x1 data-gradient GEMM with
    the GroupNorm_0 backward apply as its epilogue (option c2_fuse) -- against the plain paths (three-pass convolution on the materialised upsampled
    tensor; separate GEMM and apply launches), full-width network, forward and input-VJP.  Both run IN ONE PROCESS on two handles of the same weights
    (per-handle options, round 5: buddy_ncsnpp_set_option).  Both sides are fp32 evaluations of the same function in a different summation order:
    2e-5 of the abs-max (each holds 5e-4 against the reference fixtures).  Unknown keys / values are refused."""
    from buddy_amd import _lib
    net = build(128, 510, 128, 0)
    plain = net.replica().set_option("upconv", 0).set_option("c2_fuse", 0)
    rs = np.random.RandomState(11)
    L, B = 32768, 2
    cn = torch.tensor([-0.3, -1.2]).cuda()
    cot = torch.from_numpy(rs.standard_normal((B, L)).astype(np.float32)).cuda()
    x0 = torch.from_numpy((0.3 * rs.standard_normal((B, L))).astype(np.float32)).cuda()
    outs = {}
    for tag, n in (("fused", net), ("plain", plain), ("fused_again", net)):       # interleaved: the handles do not disturb each other
        x = x0.clone().requires_grad_(True)
        y = n(x, cn)
        g, = torch.autograd.grad(y, x, cot)
        outs[tag] = (y.detach().cpu().numpy(), g.cpu().numpy())
    assert net.get_option("upconv") == 1 and plain.get_option("upconv") == 0 and plain.get_option("c2_fuse") == 0
    assert np.array_equal(outs["fused"][0], outs["fused_again"][0]) and np.array_equal(outs["fused"][1], outs["fused_again"][1])
    ey, eg = rel(outs["fused"][0], outs["plain"][0]), rel(outs["fused"][1], outs["plain"][1])
    print(f"fused vs plain round-4 paths: forward {ey:.2e}, vjp {eg:.2e}")
    assert not np.array_equal(outs["fused"][1], outs["plain"][1]), "the options did not change the path"
    assert ey < 2e-5 and eg < 2e-5
    with pytest.raises(_lib.BuddyHipError):
        net.set_option("upconvv", 0)
    with pytest.raises(_lib.BuddyHipError):
        net.set_option("attention", 9)
    # a rejected entry is not remembered: a replica made afterwards (which replays the module's options onto its new handle) still builds and runs
    assert "upconvv" not in net._options and net._options.get("attention") != 9
    with torch.no_grad():
        assert torch.isfinite(net.replica()(x0, cn)).all()
    # an option change between a saved forward and its VJP drops the tape (the closures were recorded for the old kernels / workspaces): the VJP
    # reports a state error instead of launching against a stale arena
    x = x0.clone().requires_grad_(True)
    y = net(x, cn)
    net.set_option("gemm", 1)
    with pytest.raises(_lib.BuddyHipError, match="saved forward"):
        torch.autograd.grad(y, x, cot)
    net.set_option("gemm", 2)
    x = x0.clone().requires_grad_(True)
    g2, = torch.autograd.grad(net(x, cn), x, cot)
    assert np.array_equal(g2.cpu().numpy(), outs["fused"][1])
