"""Host side of the wMPDR beamformer after multichannel WPE (no GPU): the new symbols, the yaml defaults, the refusals before the GPU is asked
for, and two properties of the float64 restatement ``_mpdr_ref.py`` that the GPU tests lean on: its ten squarings find numpy's principal
eigenvector, and the beamformer lowers the reference channel's noise on a one-source array input.  Measured values: profiles/mpdr_accuracy.txt."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mpdr_ref as bf  # noqa: E402
import _wpe_mc_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("buddy_mpdr", "buddy_wpe_mc_mpdr_workspace_bytes", "buddy_wpe_mc_mpdr_dereverb")
PARITY = [(16000, 4, 10, 3, 3), (12345, 2, 10, 2, 5), (5000, 3, 4, 1, 2), (2000, 2, 3, 3, 1), (24000, 8, 4, 3, 3)]     # L, D, taps, delay, iterations


def test_symbols_are_declared_bound_and_exported():
    from buddy_amd import _lib
    capi = open(os.path.join(ROOT, "buddy_amd", "csrc", "capi.hip")).read()
    for name in NEW:                              # header, signatures and exports agree for every name: tests/test_abi_host.py
        assert re.search(r"\b%s\(" % name, capi), name
        assert name in _lib._SIGS and name in _lib.EXPORTED
    assert len(_lib._SIGS["buddy_mpdr"][1]) == 10 and len(_lib._SIGS["buddy_wpe_mc_mpdr_dereverb"][1]) == 13
    assert os.path.isfile(os.path.join(ROOT, "buddy_amd", "csrc", "mpdr.hip"))             # build.sh compiles and links every csrc/*.hip
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in NEW:
            assert hasattr(lib, name)
        assert lib.buddy_wpe_mc_mpdr_workspace_bytes(2, 8, 64000) == lib.buddy_wpe_mc_workspace_bytes(2, 8, 64000) > 0
        assert lib.buddy_wpe_mc_mpdr_workspace_bytes(0, 8, 64000) == 0


def test_yaml_defaults_and_beamformer_options():
    from buddy_amd.config import compose
    from buddy_amd.testing.tester import beamformer_options, channel_options
    rr = compose(tester="real_dereverberation_BUDDy").tester.real_recordings
    assert dict(rr.beamformer) == {"use": False, "iterations": 2, "loading": 1.0e-6}
    assert beamformer_options(rr) == (False, 2, 1e-6)
    assert beamformer_options({}) == (False, 2, 1e-6)                                       # a yaml written before the block existed
    assert channel_options(rr) == ("mean", 0, (10, 3, 3))                                   # untouched
    rr = compose(tester="real_dereverberation_BUDDy", overrides=["tester.real_recordings.channels=wpe", "tester.real_recordings.beamformer.use=true",
                                                                 "tester.real_recordings.beamformer.iterations=3"]).tester.real_recordings
    assert beamformer_options(rr) == (True, 3, 1e-6)
    for mode in ("mean", "reference"):
        with pytest.raises(AssertionError, match="channels: wpe"):
            beamformer_options({"channels": mode, "beamformer": {"use": True}})
    assert beamformer_options({"channels": "mean", "beamformer": {"use": False, "iterations": 4}}) == (False, 4, 1e-6)
    for bad in ({"iterations": 0}, {"loading": -1.0}, {"loading": float("inf")}):
        with pytest.raises(AssertionError):
            beamformer_options({"channels": "wpe", "beamformer": {"use": True, **bad}})


def test_arguments_are_validated_without_a_gpu():
    from buddy_amd.utils.wpe import mpdr_hip, wpe_mc_mpdr_dereverb
    y = torch.zeros(1, 2, 4000)
    for bad in (torch.zeros(2, 4000), torch.zeros(1, 9, 4000), torch.zeros(1, 2, 4000, dtype=torch.float64), torch.zeros(1, 2, 0)):
        with pytest.raises(ValueError):
            wpe_mc_mpdr_dereverb(bad)
    for kw in (dict(taps=0), dict(taps=49), dict(delay=-1), dict(reference=2), dict(reference=-1), dict(bf_iterations=0), dict(loading=-1e-6),
               dict(loading=float("nan")), dict(loading=float("inf"))):
        with pytest.raises(ValueError):
            wpe_mc_mpdr_dereverb(y, **kw)
    X = torch.zeros(4, 2, 30, dtype=torch.complex128)
    for bad in (torch.zeros(4, 2, 30, dtype=torch.complex64), torch.zeros(4, 30, dtype=torch.complex128), torch.zeros(4, 9, 30, dtype=torch.complex128),
                torch.zeros(4, 2, 0, dtype=torch.complex128)):
        with pytest.raises(ValueError):
            mpdr_hip(bad)
    for kw in (dict(reference=2), dict(iterations=0), dict(loading=-1.0), dict(loading=float("nan"))):
        with pytest.raises(ValueError):
            mpdr_hip(X, **kw)
    if not torch.cuda.is_available():                                                       # a CPU tensor of a valid shape: the product has no CPU form
        from buddy_amd._lib import BuddyHipError
        with pytest.raises(BuddyHipError):
            wpe_mc_mpdr_dereverb(y)
        with pytest.raises(BuddyHipError):
            mpdr_hip(X)


@pytest.mark.parametrize("L,D,taps,delay,iterations", PARITY)
def test_ten_squarings_find_the_principal_eigenvector(L, D, taps, delay, iterations):
    """on the parity inputs of tests/test_hip_mpdr.py (item 0): time-domain output with the squarings against the one with numpy.linalg.eigh"""
    from oracle import wpe_ref
    X = wpe_ref.wpe(ref.spectrum(ref.mc_input(0, L, D)), taps=taps, delay=delay, iterations=iterations)
    a = bf.signal(bf.mpdr(X, steering="squaring"), L)
    b = bf.signal(bf.mpdr(X, steering="eigh"), L)
    e = ref.rel(a, b)
    print(f"mpdr restatement L={L} D={D}: squaring vs eigh {e:.2e}")
    assert e < 1e-10


@pytest.mark.parametrize("snr_db", [20, 10])
def test_the_beamformer_lowers_the_reference_channels_noise(snr_db):
    """one source on four channels (gains 1, 0.9, 1.1, 0.8; fractional delays) in white noise: the residual against the clean reference channel has
    less than 0.6 of one channel's noise variance (the floor for spatially white noise is 1 / sum (g_d / g_0)^2 = 0.273)"""
    clean0, y, sigma2 = bf.noisy_array(snr_db)
    Z = bf.mpdr(ref.spectrum(y.astype(np.float32)))
    r = bf.noise_ratio(bf.signal(Z, y.shape[1]), clean0, sigma2)
    print(f"mpdr restatement, noise property at {snr_db} dB: var(z - clean_0) / sigma^2 = {r:.4f}")
    assert r < 0.6
