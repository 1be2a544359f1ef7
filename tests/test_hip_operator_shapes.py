"""GPU: the hand-written blind operator (csrc/operator.hip) against the float64 arbiter (tests/_operator_ref.py: the torch restatement under
oracle.precision.fp64() on the CPU, fed the HIP handle's own parameters and the same noise draws) at the shapes where its index arithmetic
changes path -- short, ragged, tile-exact, L == Lr, L > Lr and past the 8192-workgroup cap of the element-wise kernels.  The existing parity
tests run at four (U, L) pairs with U*T even and compare fp32 with fp32 at 2e-4 .. 5e-3; here every quantity is held to
max(golden-test bound of its class, 4 x the fp32 CPU restatement's own recorded error) -- _operator_ref.bound -- which
tests/test_operator_ref_host.py shows the restatement itself meets.  Errors are fractions of abs-max; phase-bearing quantities are compared as
complex numbers, never as angles (angles of near-zero bins and +-pi wraps are ill-conditioned)."""
import numpy as np
import pytest
import torch

import _operator_ref as R

pytestmark = pytest.mark.gpu

ALL = list(R.SHAPES)
NOT_GRID_CAP = [s for s in ALL if s != "grid_cap"]
_CTX = {}


class Ctx:
    """One shape: the HIP handle with H rebuilt from its own parameters, and the arbiter case fed exactly those parameters."""

    def __init__(self, shape_id):
        from buddy_amd.testing.operators.subband_filtering import BlindSubbandFiltering
        self.id = shape_id
        self.U, self.L = R.SHAPES[shape_id]
        self.args = R.config(3)
        self.ps = self.args.tester.posterior_sampling
        self.ns = R.streams(self.U, 0)
        self.op = BlindSubbandFiltering(self.args.tester.informed_dereverberation.op_hp, R.SR, num_utts=self.U, noise=self.ns, device="cuda", length=self.L)
        assert [n.k for n in self.ns] == [2] * self.U                   # the phases, then update_H(use_noise=True)
        assert self.op.length_rir + 1024 == R.LR_LEN
        self.params = tuple(t.clone() for t in self.op._get())          # buddy_blindop_get_params: not drawn twice
        self.op.update_H()                                              # H = cons(A e^{j phases}) of exactly these numbers, as the arbiter builds it
        self.case = R.Case(shape_id, *(t.cpu().numpy() for t in self.params), fp64=True)
        c = self.case
        self.x, self.y, self.xd, self.w = (torch.from_numpy(a.copy()).cuda() for a in (c.x, c.y, c.xd, c.w))
        self.noise = torch.from_numpy(c.noise).cuda().contiguous()
        self.op.hip_bind(self.y, self.ps)

    def restore(self):
        self.op.set_params(*self.params, reset_adam=True)
        self.op.update_H()
        for n in self.ns:
            n.k = 2


def ctx(shape_id):
    if shape_id not in _CTX:
        _CTX[shape_id] = Ctx(shape_id)
    return _CTX[shape_id]


def check(shape_id, got, ref):
    """every figure is printed before anything is asserted"""
    errs = {k: R.rel(got[k], ref[k]) for k in ref}
    for k, v in errs.items():
        print(f"HIPERR {shape_id} {k} {v:.3e} bound {R.bound(shape_id, k):.1e}")
    bad = {k: (v, R.bound(shape_id, k)) for k, v in errs.items() if not v < R.bound(shape_id, k)}
    assert not bad, (shape_id, bad)


def cplx(t):
    return torch.view_as_complex(t.contiguous())


def _lib():
    from buddy_amd import _lib as L
    return L, L.load()


# ---------------------------------------------------------------- the HIP side of each section, named like the arbiter's answers
def hip_forward(c):
    op = c.op
    rir = op.get_time_RIR().reshape(c.U, -1)
    return {"A": op.design_filter(), "H": op.H, "stft_x": op.apply_stft(c.x), "stft_rir": op.apply_stft(rir), "deg": op.degradation(c.x), "rir": rir}


def hip_vjp_x(c):
    L, lib = _lib()
    gx = torch.empty_like(c.x)
    L.check(lib.buddy_blindop_degrade_vjp(c.op._h, L.ptr(c.x.contiguous()), L.ptr(c.w.contiguous()), L.ptr(gx), None, L.stream_ptr()))
    torch.cuda.synchronize()
    return {"vjp_x": gx}


def hip_adjoints(c):
    """the library entries themselves: stft / stft_adjoint at both lengths, degrade_vjp, time_rir_vjp"""
    L, lib = _lib()
    op, U, h, s = c.op, c.U, c.op._h, L.stream_ptr()
    cs = c.case
    w_rir = torch.from_numpy(cs.w_rir).cuda()
    rir = op.get_time_RIR().reshape(U, -1).contiguous()
    out, fwd = {}, {}
    for key, sig, W in (("x", c.x.contiguous(), torch.from_numpy(cs.W_x).cuda()), ("rir", rir, torch.from_numpy(cs.W_rir).cuda())):
        n = int(sig.shape[-1])
        X = torch.empty_like(W)
        g = torch.empty(U, n, device="cuda")
        L.check(lib.buddy_blindop_stft(h, L.ptr(sig), n, L.ptr(X), s))
        L.check(lib.buddy_blindop_stft_adjoint(h, L.ptr(W.contiguous()), n, L.ptr(g), s))
        out["adj_stft_" + key], fwd["stft_" + key] = g, cplx(X)
    gx = torch.empty_like(c.x)
    gH = torch.empty(U, 513, op.Nf, 2, device="cuda"); gH2 = torch.empty_like(gH)
    L.check(lib.buddy_blindop_degrade_vjp(h, L.ptr(c.x.contiguous()), L.ptr(c.w.contiguous()), L.ptr(gx), L.ptr(gH), s))
    L.check(lib.buddy_blindop_time_rir_vjp(h, L.ptr(w_rir.contiguous()), L.ptr(gH2), s))
    torch.cuda.synchronize()
    out.update(vjp_x=gx, vjp_H=cplx(gH), vjp_rir_H=cplx(gH2))
    fwd.update(deg=op.degradation(c.x), rir=rir, H=op.H)
    return out, fwd


def hip_likelihood(c):
    xd = c.xd.clone().requires_grad_(True)
    rec = c.op.hip_rec_loss(xd)
    g, = torch.autograd.grad(rec, xd)
    return {"l_lik": c.op.last_rec_per_utt, "g_x": g}


def hip_param_grads(c, op=None, xd=None, noise=None, with_noise=True):
    L, lib = _lib()
    op = c.op if op is None else op
    xd = c.xd if xd is None else xd
    noise = c.noise if noise is None else noise
    U = op.U
    gd = torch.empty(U, op.num_exponentials, op.num_bands, device="cuda"); gw = torch.empty_like(gd)
    gp = torch.empty(U, 513, op.Nf, device="cuda"); ls = torch.zeros(2 * U, device="cuda")
    L.check(lib.buddy_blindop_param_grads(op._h, L.ptr(xd.contiguous()), L.ptr(noise.contiguous()) if with_noise else None, R.T_OP if with_noise else 0.0,
                                          op.w_rec_params, op.w_reg if with_noise else 0.0, L.ptr(gd), L.ptr(gw), L.ptr(gp), L.ptr(ls), L.stream_ptr()))
    torch.cuda.synchronize()
    out = {"l_rec": ls[:U].clone(), "g_decay": gd, "g_weights": gw, "g_phases": gp}
    if with_noise:
        out["l_reg"] = ls[U:].clone()
    return out


def hip_loss(c):
    from buddy_amd.utils.losses import get_loss
    out = {}
    for nm, fw in R.LOSS_EDGE_BLOCKS:
        a = (0.8 * c.x).requires_grad_(True); b = (0.9 * c.y).requires_grad_(True)
        v = get_loss(R.loss_block(nm, fw, R.LOSS_WEIGHT), c.op)(a, b)
        ga, gb = torch.autograd.grad(v, (a, b))
        out.update({f"loss.{nm}.{fw}.value": c.op.last_loss_per_utt.clone(), f"loss.{nm}.{fw}.g_a": ga, f"loss.{nm}.{fw}.g_b": gb})
    return out


def hip_loop(c):
    op = c.op
    c.restore()
    try:
        op.hip_optimize(c.xd, R.T_LOOP)
        assert [n.k for n in c.ns] == [5] * c.U                         # one regulariser draw per iteration and row
        st, step = op.adam_state()
        assert step == 3
        d, w, p = op._get()
        A = op.design_filter()
        op.update_H()
        out = {"loop_decay": d, "loop_weights": w, "loop_A": A, "loop_H": op.H, "loop_rir": op.get_time_RIR().reshape(c.U, -1),
               "loop_Aejphi": R.a_ejphi(A, p)}
        for nm in ("decay", "weights", "phases"):
            out["loop_m_" + nm], out["loop_v_" + nm] = st[nm][0].clone(), st[nm][1].clone()
        torch.cuda.synchronize()
        return out
    finally:
        c.restore()


def hip_section(c, name):
    if name == "forward":
        return hip_forward(c)
    if name == "adjoints":
        return hip_adjoints(c)[0]
    if name == "vjp_x":
        return hip_vjp_x(c)
    if name == "likelihood":
        return hip_likelihood(c)
    if name == "param_grads":
        return hip_param_grads(c)
    if name == "param_grads_only":
        return {"only_" + k: v for k, v in hip_param_grads(c, with_noise=False).items()}
    if name == "loss":
        return hip_loss(c)
    if name == "loop":
        return hip_loop(c)
    raise KeyError(name)


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("shape_id", ALL)
def test_forward_pieces(shape_id):
    """(a) design_filter, H, apply_stft of the signal and of the time-RIR, degradation, get_time_RIR"""
    c = ctx(shape_id)
    check(shape_id, hip_forward(c), c.case.section("forward"))


def _row_dot(a, b):
    a, b = R.to_np(a), R.to_np(b)
    return (a.conj() * b).real.reshape(a.shape[0], -1).sum(1)


def _norm2(a):
    a = R.to_np(a)
    return np.sqrt((np.abs(a) ** 2).reshape(a.shape[0], -1).sum(1))


def _absmax(a):
    a = R.to_np(a)
    return np.abs(a).reshape(a.shape[0], -1).max(1)


@pytest.mark.parametrize("shape_id", NOT_GRID_CAP)
def test_adjoints(shape_id):
    """(b) buddy_blindop_stft / _stft_adjoint at both lengths, _degrade_vjp, _time_rir_vjp: the vjp outputs against the arbiter's autograd, and
    the dot-product identity <w, A x> == <A^T w, x> per row with random cotangents, the sums accumulated in float64.

    Bound of the identity: either side is the dot product of a float32-exact vector with an output whose element-wise error is held to
    eps * abs-max by the tests above (eps = the golden bound of the forward piece; the adjoint runs the same arithmetic transposed), and
    independent element errors add in quadrature: |lhs - rhs| <= eps (max|A x| |w|_2 + max|A^T w| |x|_2)."""
    c = ctx(shape_id)
    got, fwd = hip_adjoints(c)
    cs = c.case
    W_x, W_rir = cs.W_x[..., 0] + 1j * cs.W_x[..., 1], cs.W_rir[..., 0] + 1j * cs.W_rir[..., 1]
    pairs = (("stft x", "stft", fwd["stft_x"], W_x, got["adj_stft_x"], c.x), ("stft rir", "stft", fwd["stft_rir"], W_rir, got["adj_stft_rir"], fwd["rir"]),
             ("degrade x", "filter", fwd["deg"], c.w, got["vjp_x"], c.x), ("degrade H", "filter", fwd["deg"], c.w, got["vjp_H"], fwd["H"]),
             ("time_rir H", "filter", fwd["rir"], cs.w_rir, got["vjp_rir_H"], fwd["H"]))
    fails = []
    for name, cls, Ax, w, ATw, x in pairs:
        lhs, rhs = _row_dot(w, Ax), _row_dot(ATw, x)
        tol = R.GOLDEN_BOUND[cls] * (_absmax(Ax) * _norm2(w) + _absmax(ATw) * _norm2(x))
        print(f"HIPADJ {shape_id} {name} max|lhs-rhs|/tol {np.max(np.abs(lhs - rhs) / tol):.3e}")
        if not np.all(np.abs(lhs - rhs) <= tol):
            fails.append((name, lhs, rhs, tol))
    check(shape_id, got, cs.section("adjoints"))
    assert not fails, fails


@pytest.mark.parametrize("shape_id", ALL)
def test_likelihood_and_parameter_gradients(shape_id):
    """(c) hip_rec_loss with torch.autograd.grad; buddy_blindop_param_grads with the regulariser and with noise = NULL (the path that does not
    share its launches with the regulariser chain): per-utterance loss values and the three parameter gradients.  grid_cap: the likelihood
    and the g_x of (b) only -- it is there for the second grid-stride trip."""
    c = ctx(shape_id)
    for sec in R.sections(shape_id):
        if sec in ("vjp_x", "likelihood", "param_grads", "param_grads_only"):
            check(shape_id, hip_section(c, sec), c.case.section(sec))


@pytest.mark.parametrize("shape_id", R.LOSS_SHAPES)
def test_loss_family_at_the_edges(shape_id):
    """(d) the callable loss (slot 3) with fewer elements than threads and with a second tile of one frame: the shipped l2_comp_stft_summean
    (comp_loss_kernel), a weighted spectral kind (spec_loss_kernel, the sqrt weighting of tests/test_hip_loss_family.py) and l2_mean
    (td_loss_kernel); per-utterance values and the gradient w.r.t. both arguments"""
    c = ctx(shape_id)
    check(shape_id, hip_loss(c), c.case.section("loss"))
    # the callable leaves the fused slots as bound: the likelihood is unchanged afterwards
    check(shape_id, hip_likelihood(c), c.case.section("likelihood"))


@pytest.mark.parametrize("shape_id", R.LOOP_SHAPES)
def test_captured_loop(shape_id):
    """(e) hip_optimize, three iterations of the captured graph, against three float64 iterations of the restatement's optimize_op (torch's
    Adam): what the parameters produce -- decay, weights, A e^{j phi}, and H / the time-RIR after a final update_H -- and the Adam moments.
    2e-3 through iteration 3 as in tests/test_hip_operator_golden.py (the algorithm's own fp32 sensitivity, measured there), or 4 x the fp32
    restatement's own error where that is larger: A e^{j phi} at sub_hop (6.4e-3) and odd (3.5e-3), where most bins sit at the magnitude floor
    and Adam turns the round-off of their phase gradients into +-lr steps."""
    c = ctx(shape_id)
    check(shape_id, hip_loop(c), c.case.section("loop"))


@pytest.mark.parametrize("shape_id", R.ROW_SHAPES)
def test_rows_are_independent(shape_id):
    """(f) every row again in a num_utts = 1 handle with the same parameters and noise: bit-identical forward pieces and gradients (every kernel
    is element-wise or reduces per row in a fixed order)"""
    from buddy_amd.testing.operators.subband_filtering import BlindSubbandFiltering
    from oracle.sampler_ref import NoiseStream
    c = ctx(shape_id)
    c.restore()
    whole = {**hip_forward(c), **hip_likelihood(c), **hip_param_grads(c)}
    whole.update({"only_" + k: v for k, v in hip_param_grads(c, with_noise=False).items()})
    diff = []
    for u in range(c.U):
        one = BlindSubbandFiltering(c.args.tester.informed_dereverberation.op_hp, R.SR, num_utts=1, noise=[NoiseStream(900 + u)], device="cuda", length=c.L)
        one.set_params(*(t[u:u + 1].clone() for t in c.params), reset_adam=True)
        one.update_H()
        one.hip_bind(c.y[u:u + 1].clone(), c.ps)
        x1, xd1 = c.x[u:u + 1].clone(), c.xd[u:u + 1].clone()
        rir = one.get_time_RIR().reshape(1, -1)
        row = {"A": one.design_filter(), "H": one.H, "stft_x": one.apply_stft(x1), "stft_rir": one.apply_stft(rir), "deg": one.degradation(x1), "rir": rir}
        xg = xd1.clone().requires_grad_(True)
        g, = torch.autograd.grad(one.hip_rec_loss(xg), xg)
        row.update(l_lik=one.last_rec_per_utt, g_x=g)
        row.update(hip_param_grads(c, one, xd1, c.noise[u:u + 1].clone()))
        row.update({"only_" + k: v for k, v in hip_param_grads(c, one, xd1, with_noise=False).items()})
        assert set(row) == set(whole)
        for k, v in row.items():
            if not torch.equal(v, whole[k][u:u + 1]):
                diff.append((u, k, R.rel(v, whole[k][u:u + 1])))
    print(f"HIPROW {shape_id} not bit-identical: {diff}")
    assert not diff, diff
