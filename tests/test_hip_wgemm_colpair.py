"""The two-column-block form of the batched f16x2 Winograd-domain GEMM (wgemm_f16x2_kernel<2>, option wgemm_cb / BUDDY_WGEMM_CB; csrc/wgemm.hip) against
the one-block forms: every output sums the same products in the same order, so the M arrays are the same BITS, and both hold the float64 bound of
tests/test_hip_kernels.py::test_winograd_domain_gemm_f16x2 (8e-5 of an utterance's abs-max, 2e-3 of the worst row's).

The process default of the option comes from the environment, so each form runs in a fresh child process (this file as a script): BUDDY_WGEMM_CB=2 (the new
form wherever Cout >= 256) and BUDDY_WGEMM_CB=1 (never: wgemm_f16x2_rt2_kernel at these shapes).  Two children, started together, each under its own timeout,
compute every case once; the tests compare what they wrote.

Shapes: tiles = 333 in three utterances of 111 (a ragged last row block, row blocks and waves that straddle an utterance boundary), utterances scaled by 1,
2^-9 and 2^7 (a wrong per-row scale shows), Cout 256 / 384 / 512 (one pair, a pair plus a single block, two pairs), positions 8 (folded 1-D grid) and 3
(grid.z).  Cin: the f16x2 entry points take multiples of 64 only (an even number of K-stages: buddy_wgemm_f16x2_packed_bytes is 0 otherwise, as
test_hip_kernels.py asserts), so Cin = 32 and 96 must be REFUSED with BUDDY_ERR_ARG under either form and leave M untouched; the peeled loop's edge cases at
supported sizes are Cin = 64 (only the two peeled stages), 192 (an odd stage-pair count) and 256."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILES, TPU = 333, 111
COUTS, CINS, POSITIONS = (256, 384, 512), (32, 96, 256, 64, 192), (8, 3)
CASES = [(co, ci, p) for co in COUTS for ci in CINS for p in POSITIONS]
LEVELS = (1.0, 2.0 ** -9, 2.0 ** 7)


def key(case):
    return "c%d_k%d_p%d" % case


def inputs(case):
    """seeded V (positions, tiles, Cin) with the utterances' levels applied, and U (positions, Cout, Cin); float32 numpy"""
    Cout, Cin, P_ = case
    rs = np.random.RandomState(Cout + 7 * Cin + P_)
    level = np.repeat(np.asarray(LEVELS, dtype=np.float32), TPU)[None, :, None]
    V = rs.standard_normal((P_, TILES, Cin)).astype(np.float32) * np.exp(2.0 * rs.standard_normal((P_, TILES, 1))).astype(np.float32) * level
    U = rs.standard_normal((P_, Cout, Cin)).astype(np.float32) * np.exp(1.5 * rs.standard_normal((P_, 1, Cin))).astype(np.float32) * np.float32(1e-2)
    return V, U


def child(out_path):
    """every case through buddy_wgemm_f16x2_pack_weights + buddy_gemm_winograd_domain_f16x2 under this process's BUDDY_WGEMM_CB; M arrays (or the refusal) -> npz"""
    import torch
    from buddy_amd import _lib
    lib = _lib.require_gpu()
    S = lambda: torch.cuda.current_stream().cuda_stream
    out = {}
    for case in CASES:
        Cout, Cin, P_ = case
        Vn, Un = inputs(case)
        V, U = torch.from_numpy(Vn).cuda(), torch.from_numpy(Un).cuda()
        M = torch.full((P_, TILES, Cout), 7.0, device="cuda")
        vmax = torch.empty(len(LEVELS), 64, 32, dtype=torch.int32, device="cuda")
        _lib.check(lib.buddy_abs_max_bits(V.data_ptr(), P_, len(LEVELS), TPU * Cin, vmax.data_ptr(), S()))
        nbytes = int(lib.buddy_wgemm_f16x2_packed_bytes(P_, Cout, Cin))
        if nbytes == 0:                                       # an unsupported K: both entry points refuse, nothing is launched
            U2 = torch.zeros(P_ * Cout * Cin + 128, dtype=torch.int32, device="cuda")
            rc_pack = lib.buddy_wgemm_f16x2_pack_weights(U.data_ptr(), U2.data_ptr(), P_, Cout, Cin, S())
            rc_gemm = lib.buddy_gemm_winograd_domain_f16x2(V.data_ptr(), U2.data_ptr(), M.data_ptr(), TILES, Cout, Cin, P_, vmax.data_ptr(), TPU, S())
            torch.cuda.synchronize()
            out[key(case) + "_rc"] = np.asarray([rc_pack, rc_gemm])
        else:
            U2 = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
            _lib.check(lib.buddy_wgemm_f16x2_pack_weights(U.data_ptr(), U2.data_ptr(), P_, Cout, Cin, S()))
            _lib.check(lib.buddy_gemm_winograd_domain_f16x2(V.data_ptr(), U2.data_ptr(), M.data_ptr(), TILES, Cout, Cin, P_, vmax.data_ptr(), TPU, S()))
            torch.cuda.synchronize()
        out[key(case)] = M.cpu().numpy()
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """{BUDDY_WGEMM_CB value: npz of all cases}: the two children run side by side, each under its own timeout"""
    d = tmp_path_factory.mktemp("colpair")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = {}
    for cb in ("2", "1"):
        env = dict(os.environ, BUDDY_WGEMM_CB=cb, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        procs[cb] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(d / f"cb{cb}.npz")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    res = {}
    for cb, pr in procs.items():
        try:
            log, _ = pr.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            raise
        assert pr.returncode == 0, f"BUDDY_WGEMM_CB={cb}: exit {pr.returncode}\n{log.decode(errors='replace')[-2000:]}"
        res[cb] = np.load(str(d / f"cb{cb}.npz"))
    return res


@pytest.mark.parametrize("case", CASES, ids=key)
def test_colpair_equals_one_block_forms_and_float64(forms, case):
    Cout, Cin, P_ = case
    new, old = forms["2"][key(case)], forms["1"][key(case)]
    if Cin % 64:
        for f in (forms["2"], forms["1"]):
            assert list(f[key(case) + "_rc"]) == [2, 2]       # BUDDY_ERR_ARG from both entry points
        assert np.all(new == 7.0) and np.all(old == 7.0)      # nothing was launched
        return
    assert np.array_equal(new, old)
    V, U = inputs(case)
    ref = np.einsum("pmk,pnk->pmn", V.astype(np.float64), U.astype(np.float64))
    err = np.abs(new.astype(np.float64) - ref)
    worst = max(float(err[:, u * TPU:(u + 1) * TPU].max() / np.abs(ref[:, u * TPU:(u + 1) * TPU]).max()) for u in range(len(LEVELS)))
    worst_row = float((err.max(axis=2) / np.abs(ref).max(axis=2)).max())
    print(f"Cout={Cout} Cin={Cin} positions={P_}: f16x2 two-block form vs float64 {worst:.2e} (worst row {worst_row:.2e})")
    assert worst < 8e-5 and worst_row < 2e-3


def test_network_colpair_equals_one_block_forms():
    """nf = 128, B = 2, L = 2048 (17 frames, padded to 32: the shortest at which two levels run F(6x6,3x3): 6 x 43 and 3 x 22 tiles per utterance): forward +
    input-VJP with the two-block form wherever Cout >= 256 equal the one-block forms bit for bit."""
    import torch
    from test_hip_network import build
    net = build(128, 510, 128, 3)
    assert net.get_option("gemm") == 2 and net.get_option("wgemm_cb") == 0
    rs = np.random.RandomState(11)
    x = torch.from_numpy((0.3 * rs.standard_normal((2, 2048))).astype(np.float32))
    x[1] *= 1e-2
    cot = torch.from_numpy(rs.standard_normal((2, 2048)).astype(np.float32)).cuda()
    cn = torch.tensor([-1.0, 0.1], device="cuda")

    def run(n):
        xg = x.cuda().requires_grad_(True)
        y = n(xg, cn)
        g, = torch.autograd.grad(y, xg, cot)
        return y.detach(), g

    on, off = net.replica().set_option("wgemm_cb", 2), net.replica().set_option("wgemm_cb", 1)
    assert on.get_option("wgemm_cb") == 2 and off.get_option("wgemm_cb") == 1
    (y2, g2), (y1, g1) = run(on), run(off)
    assert torch.equal(y2, y1) and torch.equal(g2, g1)
    assert float(y2.abs().max()) > 0 and float(g2.abs().max()) > 0


if __name__ == "__main__":
    child(sys.argv[1])
