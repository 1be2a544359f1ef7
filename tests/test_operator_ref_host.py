"""CPU: the float64 arbiter of the blind operator tests (tests/_operator_ref.py) held to account before the HIP operator is measured against it
(tests/test_hip_operator_shapes.py): it is self-adjoint-consistent in float64, its own fp32 form stays inside the bounds the GPU tests use at
every shape of their table, and it reproduces the vectors recorded from the reference (tests/golden/ops.npz)."""
import numpy as np
import pytest
import torch

import _operator_ref as R

torch.set_num_threads(8)


def _row_dot(a, b):
    """real inner product per row, complex arrays as (Re, Im) pairs, accumulated in float64"""
    a, b = np.asarray(a), np.asarray(b)
    return (a.conj() * b).real.reshape(a.shape[0], -1).sum(1)


@pytest.mark.parametrize("shape_id", ["sub_hop", "odd"])
def test_arbiter_adjoint_identity_in_float64(shape_id):
    """<w, A x> == <A^T w, x> for degradation (linear in x and in H) and get_time_RIR (linear in H) with the arbiter's own autograd: a broken
    reference must not pass as a tight one.  1e-12 of |w| |A x| per row."""
    c64, _ = R.host_pair(shape_id)
    f, a = c64.forward(), c64.adjoints()
    norm = lambda v: np.sqrt((np.abs(np.asarray(v, dtype=np.complex128)) ** 2).reshape(v.shape[0], -1).sum(1))
    pairs = (("x", f["deg"], c64.w, a["vjp_x"], c64.x), ("H", f["deg"], c64.w, a["vjp_H"], f["H"]), ("rir H", f["rir"], c64.w_rir, a["vjp_rir_H"], f["H"]),
             ("stft x", f["stft_x"], c64.W_x[..., 0] + 1j * c64.W_x[..., 1], a["adj_stft_x"], c64.x),
             ("stft rir", f["stft_rir"], c64.W_rir[..., 0] + 1j * c64.W_rir[..., 1], a["adj_stft_rir"], f["rir"]))
    for name, Ax, w, ATw, x in pairs:
        lhs, rhs = _row_dot(w, Ax), _row_dot(ATw, x)
        scale = norm(np.asarray(w)) * norm(Ax)
        assert np.all(np.abs(lhs - rhs) < 1e-12 * scale), (shape_id, name, lhs, rhs)


@pytest.mark.parametrize("shape_id", list(R.SHAPES))
def test_fp32_restatement_stays_inside_the_gpu_bounds(shape_id):
    """The condition that the reference alone stays inside the bound: the same calls with the default dtype at float32 against the float64
    arbiter, every quantity the GPU test of this shape compares, within max(golden bound, 4 x the recorded fp32 error) -- the golden bound
    wherever 4 x the recorded error is below it (everything but the phases after three Adam steps at sub_hop and odd)."""
    c64, c32 = R.host_pair(shape_id)
    err = R.errors(c64, c32)
    assert set(err) == set(R.fp32_err()["errors"][shape_id]), "the recorded table lists other quantities: run tests/_operator_ref.py again"
    print(shape_id, "arbiter %.1f s" % sum(c64.seconds.values()), {k: f"{v:.1e}" for k, v in err.items()})
    bad = {k: (v, R.bound(shape_id, k)) for k, v in err.items() if not v < R.bound(shape_id, k)}
    assert not bad, (shape_id, bad)


def test_bounds_are_the_golden_ones_where_the_restatement_allows():
    """4 x the recorded fp32 error exceeds the golden bound only for A e^{j phi} after the three Adam steps (scale-free updates turn round-off
    of the phase gradients of near-floor bins into +-lr steps: tests/test_hip_operator_golden.py::test_optimize_op_vs_reference)."""
    wider = {(s, k) for s, e in R.fp32_err()["errors"].items() for k in e if R.bound(s, k) > R.GOLDEN_BOUND[R.klass(k)]}
    assert wider <= {("sub_hop", "loop_Aejphi"), ("odd", "loop_Aejphi")}, wider


def test_arbiter_reproduces_the_reference_fixture(golden):
    """tests/golden/ops.npz (recorded from the reference, U = 1) at the tolerances tests/test_oracle_golden.py holds the oracle to: once through
    the noise streams (the constructor's two draws, update_H(use_noise=True), the regulariser's draw: the draw order), once with the recorded
    phases injected (the parameter injection the GPU tests rely on)."""
    from buddy_amd.config import compose
    from oracle.sampler_ref import NoiseStream
    g = golden("ops")
    args = compose()
    x, y = g["x"][None], g["y_rir"]
    ns = NoiseStream(11)
    arb = R.Arbiter(args, 1, [ns], fp64=True)
    f = arb.forward(x)
    assert R.rel(f["A"][0], g["blind_A"]) < 1e-5
    assert R.rel(np.stack([f["H"][0].real, f["H"][0].imag], -1), g["blind_H"]) < 1e-4
    assert R.rel(f["deg"], g["blind_deg"].reshape(1, -1)) < 1e-4
    assert R.rel(f["rir"][0], g["blind_rir"].reshape(-1)) < 1e-4
    assert R.rel(np.stack([f["stft_x"].real, f["stft_x"].imag], -1), g["blind_stft_x"].reshape(f["stft_x"].shape + (2,))) < 1e-5
    assert ns.k == 3
    n = ns.randn((arb.Lr,)).numpy()[None]

    def check(p):
        assert abs(float(p["l_rec"][0]) - float(g["blind_l_rec"])) < 1e-4 * abs(float(g["blind_l_rec"]))
        assert abs(float(p["l_reg"][0]) - float(g["blind_l_reg"])) < 1e-4 * abs(float(g["blind_l_reg"]))
        assert R.rel(p["g_decay"][0], g["blind_g_decay"].reshape(p["g_decay"][0].shape)) < 2e-3
        assert R.rel(p["g_weights"][0], g["blind_g_weights"].reshape(p["g_weights"][0].shape)) < 2e-3
        assert R.rel(p["g_phases"][0], g["blind_g_phases"].reshape(p["g_phases"][0].shape)) < 2e-3

    check(arb.param_grads(x, y, n, 0.005))
    decay, weights, _ = R.initial_params(args, 1)
    inj = R.Arbiter(args, 1, R.streams(1), decay, weights, g["blind_phases"].reshape(1, 513, -1), fp64=True)
    check(inj.param_grads(x, y, n, 0.005))
