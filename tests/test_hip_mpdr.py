"""GPU: the wMPDR beamformer after multichannel WPE (``buddy_mpdr`` / ``buddy_wpe_mc_mpdr_dereverb``, csrc/mpdr.hip) against the float64
restatement of DESIGN.md section 25 in ``_mpdr_ref.py``.

Beamformer alone.  The input is the oracle's WPE output.  A case first states how well-posed its input is: the restatement with numpy's LU and
with a Cholesky factorisation must agree to 1e-11 (measured 1.6e-16 ... 3.2e-15).  The kernel is then held to 64 (D / loading) 2^-53 relative to the
largest output magnitude: cond(R) <= D / loading after the loading, one backward-stable solve, and a factor 64 for the D-term sums and the
normalisation (5.7e-8 at D = 8, loading 1e-6); measured 3.6e-16 ... 2.1e-14.

Chain.  ``wpe_mc_mpdr_dereverb`` against oracle WPE -> restatement -> oracle iSTFT.  The two float64 chains (LU / LU and Cholesky / Cholesky)
must be under 1e-5 apart (measured 5.4e-13 ... 2.3e-7), and the kernel is held to 1e-4, the bound of tests/test_hip_wpe_mc.py for the same
comparison (measured 3.2e-8 ... 3.1e-7).

Measured errors: profiles/mpdr_accuracy.txt."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mpdr_ref as bf  # noqa: E402
import _wpe_mc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [  # L, D, taps, delay, WPE iterations
    (16000, 4, 10, 3, 3),
    (12345, 2, 10, 2, 5),      # ragged
    (5000, 3, 4, 1, 2),        # 43 frames, fewer than the 256 threads
    (2000, 2, 3, 3, 1),        # 19 frames
    (24000, 8, 4, 3, 3),       # D = 8, 191 frames; more than 256 frames: test_more_frames_than_threads
]
ITEMS = (0, 1, 2)
LOADING = 1e-6


@functools.lru_cache(maxsize=None)
def _input(u, L, D):
    y = ref.mc_input(u, L, D)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def _wpe(u, L, D, taps, delay, iterations, solver="lu"):
    """the oracle's WPE output of item u (F, D, T) (solver lu: oracle/wpe_ref.py itself; cholesky: the restatement of _wpe_mc_ref.py)"""
    from oracle import wpe_ref
    Y = ref.spectrum(_input(u, L, D))
    X = wpe_ref.wpe(Y, taps=taps, delay=delay, iterations=iterations) if solver == "lu" else ref.wpe(Y, taps, delay, iterations, solver="cholesky")
    X.setflags(write=False)
    return X


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()            # a copy: the cached inputs are read-only


def _mpdr_gpu(X, **kw):
    from buddy_amd.utils.wpe import mpdr_hip
    return mpdr_hip(_cuda(X), **kw).cpu().numpy()


@pytest.mark.parametrize("L,D,taps,delay,iterations", CASES)
def test_mpdr_vs_restatement(L, D, taps, delay, iterations):
    """three items in ONE call, every item against the restatement's run on that item alone"""
    X = [_wpe(u, L, D, taps, delay, iterations) for u in ITEMS]
    F, _, T = X[0].shape
    Z = _mpdr_gpu(np.concatenate(X, 0), loading=LOADING)
    assert Z.shape == (len(ITEMS) * F, T) and np.isfinite(Z.view(np.float64)).all()
    for b, u in enumerate(ITEMS):
        zc, zl = bf.mpdr(X[b], solver="cholesky", loading=LOADING), bf.mpdr(X[b], solver="lu", loading=LOADING)
        fit, e = ref.rel(zc, zl), ref.rel(Z[b * F:(b + 1) * F], zc)
        print(f"mpdr L={L} D={D} T={T} item {u}: float64 LU vs Cholesky {fit:.2e} | kernel vs restatement {e:.2e} (bound {bf.bound(D, LOADING):.2e})")
        assert fit < 1e-11, ("the input is not fit for the comparison", L, D, u, fit)
        assert e < bf.bound(D, LOADING), (L, D, u, e)


def test_more_frames_than_threads():
    """T = 1, 257 and 700 from random numbers (a second and a third round of the frame loop with ragged tails), D = 3 and 8"""
    rs = np.random.RandomState(1)
    for D, T in [(3, 1), (8, 1), (3, 257), (8, 700)]:
        mix = rs.standard_normal((5, D, 1)) + 1j * rs.standard_normal((5, D, 1))
        X = mix * (rs.standard_normal((5, 1, T)) + 1j * rs.standard_normal((5, 1, T))) + 0.3 * (rs.standard_normal((5, D, T)) + 1j * rs.standard_normal((5, D, T)))
        Z = _mpdr_gpu(X, reference=D - 1, loading=LOADING)
        zc, zl = bf.mpdr(X, reference=D - 1, solver="cholesky", loading=LOADING), bf.mpdr(X, reference=D - 1, solver="lu", loading=LOADING)
        fit, e = ref.rel(zc, zl), ref.rel(Z, zc)
        print(f"mpdr random D={D} T={T}: float64 LU vs Cholesky {fit:.2e} | kernel vs restatement {e:.2e} (bound {bf.bound(D, LOADING):.2e})")
        assert np.isfinite(Z.view(np.float64)).all() and fit < 1e-11 and e < bf.bound(D, LOADING), (D, T, fit, e)


@pytest.mark.parametrize("L,D,taps,delay,iterations", CASES)
def test_chain_vs_oracle(L, D, taps, delay, iterations):
    from buddy_amd.utils.wpe import wpe_mc_mpdr_dereverb
    y = np.stack([_input(u, L, D) for u in ITEMS])
    out = wpe_mc_mpdr_dereverb(_cuda(y), taps=taps, delay=delay, iterations=iterations, loading=LOADING).cpu().numpy()
    assert out.shape == (len(ITEMS), L) and out.dtype == np.float32 and np.isfinite(out).all()
    for b, u in enumerate(ITEMS):
        a = bf.signal(bf.mpdr(_wpe(u, L, D, taps, delay, iterations, "lu"), solver="lu", loading=LOADING), L)
        c = bf.signal(bf.mpdr(_wpe(u, L, D, taps, delay, iterations, "cholesky"), solver="cholesky", loading=LOADING), L)
        fit, e = ref.rel(c, a), ref.rel(out[b], a)
        print(f"chain L={L} D={D} taps={taps} item {u}: float64 LU/LU vs Cholesky/Cholesky {fit:.2e} | kernel vs oracle chain {e:.2e}")
        assert fit < 1e-5, ("the input is not fit for a 1e-4 comparison", L, D, taps, u, fit)
        assert e < 1e-4, (L, D, taps, u, e)


def test_one_channel_is_a_copy():
    from buddy_amd.utils.wpe import wpe_mc_dereverb, wpe_mc_mpdr_dereverb
    rs = np.random.RandomState(2)
    X = rs.standard_normal((7, 1, 300)) + 1j * rs.standard_normal((7, 1, 300))
    assert np.array_equal(_mpdr_gpu(X), X[:, 0])
    y = _cuda(_input(0, 5000, 1))[None]
    assert torch.equal(wpe_mc_mpdr_dereverb(y, taps=4, delay=1, iterations=2), wpe_mc_dereverb(y, taps=4, delay=1, iterations=2)[:, 0])


def test_rows_are_independent():
    """a problem's bits do not depend on the batch: B = 2 in one call equals the two B = 1 calls, spectra and signals"""
    from buddy_amd.utils.wpe import mpdr_hip, wpe_mc_mpdr_dereverb
    L, D = 5000, 3
    y = _cuda(np.stack([_input(u, L, D) for u in (0, 1)]))
    both = wpe_mc_mpdr_dereverb(y, taps=4, delay=1, iterations=2)
    for b in range(2):
        assert torch.equal(both[b], wpe_mc_mpdr_dereverb(y[b:b + 1], taps=4, delay=1, iterations=2)[0])
    X = _cuda(np.concatenate([_wpe(u, L, D, 4, 1, 2) for u in (0, 1)], 0))
    F = X.shape[0] // 2
    Zb = torch.view_as_real(mpdr_hip(X))
    assert torch.equal(Zb[:F], torch.view_as_real(mpdr_hip(X[:F]))) and torch.equal(Zb[F:], torch.view_as_real(mpdr_hip(X[F:])))


@pytest.mark.parametrize("iterations", [1, 3])
def test_iteration_counts(iterations):
    X = _wpe(0, 5000, 3, 4, 1, 2)
    for r in (0, 2):
        e = ref.rel(_mpdr_gpu(X, reference=r, iterations=iterations), bf.mpdr(X, reference=r, iterations=iterations))
        print(f"mpdr 43 frames, reference {r}, {iterations} iteration(s): kernel vs restatement {e:.2e}")
        assert e < bf.bound(3, LOADING)


def test_silent_channels_and_silence():
    """A silent non-reference channel drops out: the D = 4 run with channel 2 zeroed equals the D = 3 run without it at the same ABSOLUTE loading
    (the loading is relative to tr(R) / D and lambda of the first iteration to the channel mean, so the D = 3 run takes 3/4 of the relative
    loading; the common factor of lambda cancels in w).  A silent reference channel is passed through: exactly zero.  Silence gives silence."""
    X = np.array(_wpe(0, 16000, 4, 10, 3, 3))
    X[:, 2] = 0
    a = _mpdr_gpu(X, loading=LOADING)
    b = _mpdr_gpu(np.ascontiguousarray(X[:, [0, 1, 3]]), loading=0.75 * LOADING)
    e = ref.rel(a, b)
    print(f"mpdr silent channel: D=4 with channel 2 zero vs the D=3 run {e:.2e} (bound {bf.bound(4, LOADING):.2e})")
    assert np.isfinite(a.view(np.float64)).all() and e < bf.bound(4, LOADING)
    z = _mpdr_gpu(X, reference=2, loading=LOADING)
    assert np.isfinite(z.view(np.float64)).all() and not z.any()
    assert np.array_equal(z, bf.mpdr(X, reference=2))
    from buddy_amd.utils.wpe import wpe_mc_mpdr_dereverb
    assert not _mpdr_gpu(np.zeros((3, 4, 50), np.complex128)).any()
    assert not wpe_mc_mpdr_dereverb(torch.zeros(1, 2, 5000, device="cuda"), taps=4, delay=1, iterations=2).any()


@pytest.mark.parametrize("snr_db", [20, 10])
def test_noise_property(snr_db):
    """the input of tests/test_mpdr_host.py: the kernel's noise ratio is the restatement's to 1e-3 relative"""
    clean0, y, sigma2 = bf.noisy_array(snr_db)
    Y = ref.spectrum(y.astype(np.float32))
    want = bf.noise_ratio(bf.signal(bf.mpdr(Y), y.shape[1]), clean0, sigma2)
    got = bf.noise_ratio(bf.signal(_mpdr_gpu(Y), y.shape[1]), clean0, sigma2)
    print(f"mpdr noise property at {snr_db} dB: kernel {got:.4f}, restatement {want:.4f}")
    assert want < 0.6 and abs(got - want) < 1e-3 * want


def test_refusals_through_the_raw_entries():
    """every refusal returns BUDDY_ERR_ARG before any launch: the output buffers keep their bits"""
    from buddy_amd import _lib
    lib = _lib.require_gpu()
    T, L = 16, 2000
    inf, nan = float("inf"), float("nan")
    #          D  ref it loading rows T
    for D, r, it, load, rows, Tn in [(9, 0, 2, 1e-6, 2, T), (0, 0, 2, 1e-6, 2, T), (2, 2, 2, 1e-6, 2, T), (2, -1, 2, 1e-6, 2, T), (2, 0, 0, 1e-6, 2, T),
                                     (2, 0, 2, -1e-6, 2, T), (2, 0, 2, inf, 2, T), (2, 0, 2, nan, 2, T), (2, 0, 2, 1e-6, 0, T), (2, 0, 2, 1e-6, 2, 0)]:
        X = torch.zeros(2, max(D, 1), T, 2, dtype=torch.float64, device="cuda")
        Z = torch.full((2, T, 2), 7.0, dtype=torch.float64, device="cuda")
        s = torch.zeros(2 * T, dtype=torch.float64, device="cuda")
        rc = lib.buddy_mpdr(_lib.ptr(X), _lib.ptr(Z), _lib.ptr(s), rows, D, Tn, r, it, load, _lib.stream_ptr())
        assert rc == 2, (D, r, it, load, rows, Tn, rc)
        torch.cuda.synchronize()
        assert bool((Z == 7.0).all())
    #          D  taps ref it loading B  L
    for D, taps, r, it, load, B, Ln in [(9, 4, 0, 2, 1e-6, 1, L), (0, 4, 0, 2, 1e-6, 1, L), (8, 13, 0, 2, 1e-6, 1, L), (2, 0, 0, 2, 1e-6, 1, L), (2, 4, 2, 2, 1e-6, 1, L),
                                        (2, 4, -1, 2, 1e-6, 1, L), (2, 4, 0, 0, 1e-6, 1, L), (2, 4, 0, 2, -1.0, 1, L), (2, 4, 0, 2, inf, 1, L), (2, 4, 0, 2, nan, 1, L),
                                        (2, 4, 0, 2, 1e-6, 0, L), (2, 4, 0, 2, 1e-6, 1, 0)]:
        y = torch.zeros(1, max(D, 1), L, device="cuda")
        out = torch.full((1, L), 7.0, device="cuda")
        w = torch.zeros(max(8, int(lib.buddy_wpe_mc_mpdr_workspace_bytes(1, max(D, 1), L)) // 8), dtype=torch.float64, device="cuda")
        rc = lib.buddy_wpe_mc_mpdr_dereverb(_lib.ptr(y), _lib.ptr(out), ctypes.c_void_p(w.data_ptr()), B, D, Ln, taps, 3, 3, r, it, load, _lib.stream_ptr())
        assert rc == 2, (D, taps, r, it, load, B, Ln, rc)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
