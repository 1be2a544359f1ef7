"""WPE (weighted prediction error) dereverberation for the ``wpe_scaled`` warm start of the blind sampler
(reference ``testing/EulerHeunSamplerDPS.py:32-54``: ``nara_wpe.utils.stft/istft`` with size 512 / shift 128 and
``nara_wpe.wpe.wpe(Y, taps=50, delay=2, iterations=5, statistics_mode='full')``).

``nara_wpe`` is a third-party package that is neither in the reference's ``requirements.txt`` nor installable offline, so the library
restates its published algorithm (Nakatani et al. 2010; Drude et al. 2018, batch "full statistics" variant) and its STFT conventions
(periodic Blackman analysis window, "fading" zero padding of size-shift samples on both sides, bi-orthogonal synthesis window).  PARITY
UNPINNED against the package itself; checked on the GPU against the independent numpy oracle ``oracle/wpe_ref.py``.
The whole estimate is ONE library call (``buddy_wpe_dereverb``, ``csrc/wpe.hip``): hand-written complex128 STFT, the iterations (inverse
power, correlation matrix, Cholesky solve, prediction filter; one workgroup per (utterance, bin) row) and the overlap-add iSTFT.  There is
no CPU form in the product: a CPU tensor raises ``BuddyHipError`` (the torch restatement used by host-logic tests lives in ``oracle/batched``).

Multichannel WPE (``wpe_mc_hip``, ``wpe_mc_dereverb``; ``csrc/wpe_mc.hip``) is the same algorithm for D channels, ``oracle/wpe_ref.py:91-120``
as written for any D: the front end of the real-recordings mode for microphone-array files (``tester.real_recordings.channels: wpe``) and the
WPE-alone baseline of the reports (``tools/wpe.py``).  Its defaults are nara_wpe's (taps 10, delay 3, 3 iterations).  Parity with nara_wpe
itself is unpinned for D > 1 as for D = 1, and whether the cascade WPE -> BUDDy scores better than the channel mean on a trained checkpoint is
UNMEASURED: there is no trained checkpoint here.

The wMPDR beamformer (``mpdr_hip``, ``wpe_mc_mpdr_dereverb``; ``csrc/mpdr.hip``) turns the D WPE outputs into one channel:
steering vector from the bin's covariance, weights that minimise the power weighted by 1 / |z_t|^2 under a distortionless constraint towards
the reference channel.  ``real_recordings.beamformer.use`` and ``tools/wpe.py --beamformer wmpdr`` reach it through the fused entry."""
from __future__ import annotations

import torch

from .. import _lib


def wpe_hip(Y, taps=10, delay=3, iterations=3):
    """The WPE iterations alone for D = 1 through the hand-written kernel (``buddy_wpe``): Y (F, 1, T) complex128 on the GPU."""
    lib = _lib.require_gpu()
    F, D, T = Y.shape
    assert D == 1 and Y.is_cuda and Y.dtype == torch.complex128
    Yr = torch.view_as_real(Y.contiguous()).contiguous()                    # (F, 1, T, 2) float64
    Xr = torch.empty_like(Yr)
    scratch = torch.empty(F * T, dtype=torch.float64, device=Y.device)
    _lib.check(lib.buddy_wpe(_lib.ptr(Yr), _lib.ptr(Xr), _lib.ptr(scratch), F, T, int(taps), int(delay), int(iterations), _lib.stream_ptr()))
    return torch.view_as_complex(Xr)


def wpe_dereverb(y, taps=50, delay=2, iterations=5, size=512, shift=128):
    """y (B, L) float32 on the GPU -> (B, L) float32: stft -> per-utterance single-channel WPE -> istft (reference :36-51), one library call."""
    lib = _lib.require_gpu()
    if not y.is_cuda:
        raise _lib.BuddyHipError("wpe_dereverb: the warm start runs on the MI355X only (got a CPU tensor)")
    assert (size, shift) == (512, 128), "the HIP warm start is built for the reference's stft_options (size 512, shift 128)"
    B, L = y.shape
    yc = y.contiguous().float()
    out = torch.empty_like(yc)
    work = torch.empty(int(lib.buddy_wpe_workspace_bytes(B, L)) // 8, dtype=torch.float64, device=y.device)
    _lib.check(lib.buddy_wpe_dereverb(_lib.ptr(yc), _lib.ptr(out), _lib.ptr(work), B, L, int(taps), int(delay), int(iterations), _lib.stream_ptr()))
    return out


# ---------------------------------------------------------------------------- multichannel WPE (csrc/wpe_mc.hip)
MAX_CHANNELS = 8
MAX_FILTER = 96          # D * taps: R (packed triangle) and P of one (utterance, bin) problem stay in the LDS of one workgroup


def supported(D, taps):
    """the shapes ``buddy_wpe_mc`` takes: 1 <= D <= 8 channels, taps >= 1, D * taps <= 96"""
    return 1 <= int(D) <= MAX_CHANNELS and int(taps) >= 1 and int(D) * int(taps) <= MAX_FILTER


def frames(L):
    """frame count of the STFT (size 512, shift 128, fading, tail padded to a whole frame) for L samples"""
    size, shift = 512, 128
    n = int(L) + 2 * (size - shift)
    if n < size:
        n = size
    elif (n + shift - size) % shift:
        n += shift - (n + shift - size) % shift
    return (n - size) // shift + 1


def _check_mc(name, D, taps, delay, iterations):
    if not 1 <= D <= MAX_CHANNELS:
        raise ValueError(f"{name}: {D} channels; the kernel takes 1 to {MAX_CHANNELS}")
    if taps < 1 or delay < 0 or iterations < 0:
        raise ValueError(f"{name}: taps >= 1, delay >= 0, iterations >= 0 (got {taps}, {delay}, {iterations})")
    if not supported(D, taps):
        raise ValueError(f"{name}: D * taps = {D * taps} is over the limit of {MAX_FILTER}")


def wpe_mc_hip(Y, taps=10, delay=3, iterations=3):
    """The WPE iterations for D channels (``buddy_wpe_mc``): Y (F, D, T) complex128 on the GPU -> (F, D, T); every row a problem of its own."""
    taps, delay, iterations = int(taps), int(delay), int(iterations)
    if Y.dim() != 3 or Y.dtype != torch.complex128 or Y.shape[0] < 1 or Y.shape[2] < 1:
        raise ValueError(f"wpe_mc_hip: Y must be (F, D, T) complex128, got {tuple(Y.shape)} {Y.dtype}")
    F, D, T = Y.shape
    _check_mc("wpe_mc_hip", D, taps, delay, iterations)
    lib = _lib.require_gpu()
    if not Y.is_cuda:
        raise _lib.BuddyHipError("wpe_mc_hip: runs on the MI355X only (got a CPU tensor)")
    Yr = torch.view_as_real(Y.contiguous()).contiguous()                    # (F, D, T, 2) float64
    Xr = torch.empty_like(Yr)
    scratch = torch.empty(F * T, dtype=torch.float64, device=Y.device)
    _lib.check(lib.buddy_wpe_mc(_lib.ptr(Yr), _lib.ptr(Xr), _lib.ptr(scratch), F, D, T, taps, delay, iterations, _lib.stream_ptr()))
    return torch.view_as_complex(Xr)


def wpe_mc_dereverb(y, taps=10, delay=3, iterations=3):
    """y (B, D, L) float32 on the GPU -> (B, D, L) float32: stft -> D-channel WPE per item and bin -> istft, all channels out, one library
    call.  Its workspace is B * 257 * frames(L) * (32 * D + 8) bytes: linear in D * L, the whole signal goes in one call."""
    taps, delay, iterations = int(taps), int(delay), int(iterations)
    if y.dim() != 3 or y.shape[0] < 1 or y.shape[2] < 1 or y.dtype != torch.float32:
        raise ValueError(f"wpe_mc_dereverb: y must be (B, D, L) float32, got {tuple(y.shape)} {y.dtype}")
    B, D, L = y.shape
    _check_mc("wpe_mc_dereverb", D, taps, delay, iterations)
    lib = _lib.require_gpu()
    if not y.is_cuda:
        raise _lib.BuddyHipError("wpe_mc_dereverb: runs on the MI355X only (got a CPU tensor)")
    yc = y.contiguous()
    out = torch.empty_like(yc)
    work = torch.empty(int(lib.buddy_wpe_mc_workspace_bytes(B, D, L)) // 8, dtype=torch.float64, device=y.device)
    _lib.check(lib.buddy_wpe_mc_dereverb(_lib.ptr(yc), _lib.ptr(out), _lib.ptr(work), B, D, L, taps, delay, iterations, _lib.stream_ptr()))
    return out


# ---------------------------------------------------------------------------- wMPDR beamformer after multichannel WPE (csrc/mpdr.hip)
def _check_bf(name, D, reference, iterations, loading):
    if not 1 <= D <= MAX_CHANNELS:
        raise ValueError(f"{name}: {D} channels; the kernel takes 1 to {MAX_CHANNELS}")
    if not 0 <= reference < D:
        raise ValueError(f"{name}: reference channel {reference} of {D}")
    if iterations < 1:
        raise ValueError(f"{name}: the beamformer needs iterations >= 1 (got {iterations})")
    if not (loading >= 0.0 and loading != float("inf")):
        raise ValueError(f"{name}: loading must be finite and >= 0 (got {loading})")


def mpdr_hip(X, reference=0, iterations=2, loading=1e-6):
    """The wMPDR beamformer alone (``buddy_mpdr``): X (F, D, T) complex128 on the GPU -> (F, T); every row a problem of
    its own.  The steering vector is the principal eigenvector of sum_t x x^H relative to ``reference``; ``loading`` (relative diagonal
    loading of the weighted covariance) defaults to 1e-6, a choice and not a measurement."""
    reference, iterations, loading = int(reference), int(iterations), float(loading)
    if X.dim() != 3 or X.dtype != torch.complex128 or X.shape[0] < 1 or X.shape[2] < 1:
        raise ValueError(f"mpdr_hip: X must be (F, D, T) complex128, got {tuple(X.shape)} {X.dtype}")
    F, D, T = X.shape
    _check_bf("mpdr_hip", D, reference, iterations, loading)
    lib = _lib.require_gpu()
    if not X.is_cuda:
        raise _lib.BuddyHipError("mpdr_hip: runs on the MI355X only (got a CPU tensor)")
    Xr = torch.view_as_real(X.contiguous()).contiguous()                    # (F, D, T, 2) float64
    Zr = torch.empty(F, T, 2, dtype=torch.float64, device=X.device)
    scratch = torch.empty(F * T, dtype=torch.float64, device=X.device)
    _lib.check(lib.buddy_mpdr(_lib.ptr(Xr), _lib.ptr(Zr), _lib.ptr(scratch), F, D, T, reference, iterations, loading, _lib.stream_ptr()))
    return torch.view_as_complex(Zr)


def wpe_mc_mpdr_dereverb(y, taps=10, delay=3, iterations=3, reference=0, bf_iterations=2, loading=1e-6):
    """y (B, D, L) float32 on the GPU -> (B, L) float32: stft -> D-channel WPE (the kernel and the bits of ``wpe_mc_dereverb``) -> wMPDR
    beamformer towards ``reference`` -> istft, one library call in the workspace of ``wpe_mc_dereverb``."""
    taps, delay, iterations = int(taps), int(delay), int(iterations)
    reference, bf_iterations, loading = int(reference), int(bf_iterations), float(loading)
    if y.dim() != 3 or y.shape[0] < 1 or y.shape[2] < 1 or y.dtype != torch.float32:
        raise ValueError(f"wpe_mc_mpdr_dereverb: y must be (B, D, L) float32, got {tuple(y.shape)} {y.dtype}")
    B, D, L = y.shape
    _check_mc("wpe_mc_mpdr_dereverb", D, taps, delay, iterations)
    _check_bf("wpe_mc_mpdr_dereverb", D, reference, bf_iterations, loading)
    lib = _lib.require_gpu()
    if not y.is_cuda:
        raise _lib.BuddyHipError("wpe_mc_mpdr_dereverb: runs on the MI355X only (got a CPU tensor)")
    yc = y.contiguous()
    out = torch.empty(B, L, dtype=torch.float32, device=y.device)
    work = torch.empty(int(lib.buddy_wpe_mc_mpdr_workspace_bytes(B, D, L)) // 8, dtype=torch.float64, device=y.device)
    _lib.check(lib.buddy_wpe_mc_mpdr_dereverb(_lib.ptr(yc), _lib.ptr(out), _lib.ptr(work), B, D, L, taps, delay, iterations, reference, bf_iterations,
                                              loading, _lib.stream_ptr()))
    return out
