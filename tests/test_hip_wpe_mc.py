"""GPU: multichannel WPE (``buddy_wpe_mc`` / ``buddy_wpe_mc_dereverb``, csrc/wpe_mc.hip) against ``oracle/wpe_ref.py``, which is written for
any channel count D (numpy, independent of the product; parity with nara_wpe itself stays unpinned, the package is absent).

The systems are ill-conditioned (cond(R) up to ~1e14 on this input), so before it judges the kernel every parity case states how far two
float64 solutions of the same iterations are apart: the oracle (numpy LU) and the Cholesky path of the restatement in ``_wpe_mc_ref.py``
(whose LU path is the oracle bit for bit, asserted once below).  That distance, on the time-domain result, must stay under 1e-5 -- a
condition on the INPUT, met with a factor of two to spare (measured 3.8e-13 ... 4.4e-6) -- and the kernel is then held to 1e-4 on the
spectra and on the time-domain result, the bound tests/test_hip_wpe.py uses for the same comparison (Cholesky kernel, LU numpy, float32
output).  Measured errors: profiles/wpe_mc_accuracy.txt."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wpe_mc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [  # L, D, taps, delay, iterations
    (16000, 4, 10, 3, 3),
    (12345, 2, 10, 2, 5),      # ragged
    (48000, 8, 10, 3, 3),      # N = 80
    (48000, 8, 12, 3, 3),      # N = 96, the limit
    (32000, 2, 40, 2, 3),      # N = 80, long filter
    (5000, 3, 4, 1, 2),        # 43 frames
    (2000, 2, 3, 3, 1),        # 19 frames
]
ITEMS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def _input(u, L, D):
    y = ref.mc_input(u, L, D)
    y.setflags(write=False)
    return y


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()            # a copy: the cached inputs are read-only


@pytest.mark.parametrize("L,D,taps,delay,iterations", CASES)
def test_wpe_mc_vs_oracle(L, D, taps, delay, iterations):
    """spectra (``wpe_mc_hip`` on the oracle's STFT) and time-domain result (``wpe_mc_dereverb``), three items in ONE call each (B = 3),
    every item against the oracle's run on that item alone"""
    from buddy_amd.utils.wpe import frames, wpe_mc_dereverb, wpe_mc_hip
    from oracle import wpe_ref
    y = np.stack([_input(u, L, D) for u in ITEMS])                                   # (B, D, L)
    Y = [ref.spectrum(y[b]) for b in range(len(ITEMS))]                              # (F, D, T) each
    F, _, T = Y[0].shape
    assert T == frames(L)
    X = wpe_mc_hip(_cuda(np.concatenate(Y, 0)), taps=taps, delay=delay, iterations=iterations).cpu().numpy()
    out = wpe_mc_dereverb(_cuda(y), taps=taps, delay=delay, iterations=iterations).cpu().numpy()
    assert X.shape == (len(ITEMS) * F, D, T) and out.shape == y.shape and out.dtype == np.float32
    assert np.isfinite(X.view(np.float64)).all() and np.isfinite(out).all()
    for b, u in enumerate(ITEMS):
        Xo = wpe_ref.wpe(Y[b], taps=taps, delay=delay, iterations=iterations)
        xo = ref.signal(Xo, L)
        fit = ref.rel(ref.signal(ref.wpe(Y[b], taps, delay, iterations, solver="cholesky"), L), xo)
        es, et = ref.rel(X[b * F:(b + 1) * F], Xo), ref.rel(out[b], xo)
        print(f"wpe_mc L={L} D={D} taps={taps} delay={delay} it={iterations} item {u}: float64 LU vs Cholesky {fit:.2e} | "
              f"kernel vs oracle: spectra {es:.2e}, time {et:.2e}")
        assert fit < 1e-5, ("the input is not fit for a 1e-4 comparison", L, D, taps, u, fit)
        assert es < 1e-4 and et < 1e-4, (L, D, taps, u, es, et)


def test_restatement_lu_is_the_oracle_and_no_iterations_is_the_input():
    from buddy_amd.utils.wpe import wpe_mc_dereverb, wpe_mc_hip
    from oracle import wpe_ref
    L, D = 5000, 3
    y = _input(0, L, D)
    Y = ref.spectrum(y)
    assert np.array_equal(ref.wpe(Y, 4, 1, 2, solver="lu"), wpe_ref.wpe(Y, taps=4, delay=1, iterations=2))
    X = wpe_mc_hip(_cuda(Y), taps=4, delay=1, iterations=0).cpu().numpy()
    assert np.array_equal(X, Y)
    out = wpe_mc_dereverb(_cuda(y[None]), taps=4, delay=1, iterations=0).cpu().numpy()            # istft(stft(y)) = y
    assert ref.rel(out[0], y) < 1e-6


def test_one_channel_through_the_new_entry():
    """D = 1 is the existing warm-start kernel's problem: same input, few taps (well conditioned), both results at float32 output precision"""
    from buddy_amd.utils.wpe import wpe_dereverb, wpe_mc_dereverb
    y = _cuda(_input(0, 12345, 1))                                                   # (1, L)
    a = wpe_mc_dereverb(y[None], taps=7, delay=3, iterations=2).cpu().numpy()[0]
    b = wpe_dereverb(y, taps=7, delay=3, iterations=2).cpu().numpy()
    e = ref.rel(a, b)
    print(f"wpe_mc D=1 vs buddy_wpe_dereverb: {e:.2e}")
    assert e < 1e-6


def test_rows_are_independent():
    """a problem's bits do not depend on the batch: B = 2 in one call equals the two B = 1 calls, spectra and signals"""
    from buddy_amd.utils.wpe import wpe_mc_dereverb, wpe_mc_hip
    L, D = 5000, 3
    y = _cuda(np.stack([_input(u, L, D) for u in (0, 1)]))
    both = wpe_mc_dereverb(y, taps=4, delay=1, iterations=2)
    for b in range(2):
        assert torch.equal(both[b], wpe_mc_dereverb(y[b:b + 1], taps=4, delay=1, iterations=2)[0])
    Y = _cuda(np.concatenate([ref.spectrum(_input(u, L, D)) for u in (0, 1)], 0))
    F = Y.shape[0] // 2
    Xb = torch.view_as_real(wpe_mc_hip(Y, taps=4, delay=1, iterations=2))
    assert torch.equal(Xb[:F], torch.view_as_real(wpe_mc_hip(Y[:F], taps=4, delay=1, iterations=2)))
    assert torch.equal(Xb[F:], torch.view_as_real(wpe_mc_hip(Y[F:], taps=4, delay=1, iterations=2)))


def test_silent_channel():
    """D = 3 with channel 1 all zeros: R is singular (no oracle: numpy refuses it).  The zero pivots give zero rows of G, so the silent
    channel stays exactly zero and the other two get the D = 2 solution (lambda is 2/3 of the D = 2 one in every frame, which cancels in G)."""
    from buddy_amd.utils.wpe import wpe_mc_dereverb
    L = 5000
    y2 = _input(0, L, 2)
    y3 = np.stack([y2[0], np.zeros(L, np.float32), y2[1]])
    a = wpe_mc_dereverb(_cuda(y3[None]), taps=4, delay=1, iterations=2).cpu().numpy()[0]
    b = wpe_mc_dereverb(_cuda(y2[None]), taps=4, delay=1, iterations=2).cpu().numpy()[0]
    assert np.isfinite(a).all()
    assert not a[1].any()
    e = ref.rel(a[[0, 2]], b)
    print(f"wpe_mc silent channel: D=3 channels 0, 2 vs the D=2 run {e:.2e}")
    assert e < 1e-4
    z = wpe_mc_dereverb(torch.zeros(1, 2, L, device="cuda"), taps=4, delay=1, iterations=2)      # silent bins everywhere
    assert not z.any()


def test_refusals_through_the_raw_entry():
    """D = 9, D * taps = 104 and taps = 0 return BUDDY_ERR_ARG before any launch: the output buffer keeps its bits"""
    from buddy_amd import _lib
    lib = _lib.require_gpu()
    T = 16
    for D, taps in [(9, 4), (8, 13), (2, 0)]:
        Y = torch.zeros(2, D, T, 2, dtype=torch.float64, device="cuda")
        X = torch.full_like(Y, 7.0)
        s = torch.zeros(2 * T, dtype=torch.float64, device="cuda")
        rc = lib.buddy_wpe_mc(_lib.ptr(Y), _lib.ptr(X), _lib.ptr(s), 2, D, T, taps, 3, 3, _lib.stream_ptr())
        assert rc == 2, (D, taps, rc)
        assert b"wpe" in lib.buddy_last_error()
        y = torch.zeros(1, D, 2000, device="cuda")
        out = torch.full_like(y, 7.0)
        w = torch.zeros(max(8, int(lib.buddy_wpe_mc_workspace_bytes(1, D, 2000)) // 8), dtype=torch.float64, device="cuda")
        rc = lib.buddy_wpe_mc_dereverb(_lib.ptr(y), _lib.ptr(out), ctypes.c_void_p(w.data_ptr()), 1, D, 2000, taps, 3, 3, _lib.stream_ptr())
        assert rc == 2, (D, taps, rc)
        torch.cuda.synchronize()
        assert bool((X == 7.0).all()) and bool((out == 7.0).all())
