"""Sample-rate conversion for real recordings (``Tester.test_real_recordings``): a rational polyphase resampler, one library call
(``buddy_resample``, ``csrc/resample.hip``).  No reference counterpart: the reference's loaders assert ``samplerate == fs``.

``y[n] = sum_m x[m] h[n*down - m*up + c]`` with ``Lout = ceil(Lin*up/down)``: zero-stuffing by ``up``, a Kaiser-windowed sinc ``h`` of DC gain
``up`` cutting at ``rolloff`` of the lower Nyquist, every ``down``-th sample kept, zero extension at both ends -- in float64 this is
``scipy.signal.resample_poly(x, up, down, window=h/up, padtype='constant')``.  The taps are designed on the host in double (numpy only) and go
to the device as fp32; the filtering itself has no CPU form: a CPU tensor raises ``BuddyHipError``."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from .. import _lib


def ratio(fs_in, fs_out):
    """(up, down) in lowest terms: 44 100 -> 16 000 is (160, 441)"""
    fs_in, fs_out = int(fs_in), int(fs_out)
    assert fs_in > 0 and fs_out > 0, "sample rates must be positive"
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g


def out_length(Lin, up, down):
    return -((-int(Lin) * int(up)) // int(down))


@functools.lru_cache(maxsize=None)
def design_filter(up, down, zeros=24, beta=10.0, rolloff=0.9):
    """Odd-length symmetric low-pass, float64: ``zeros`` zero crossings of the sinc on either side at the lower of the two rates, Kaiser window,
    cut-off at ``rolloff`` of the lower Nyquist, sum(h) == up.  Cached per argument tuple (the same read-only array on every call)."""
    m = max(int(up), int(down))
    half = int(zeros) * m
    n = np.arange(-half, half + 1, dtype=np.float64)
    fc = float(rolloff) / m
    h = fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, float(beta))
    h *= up / h.sum()
    h.setflags(write=False)
    return h


_device_taps = {}


def _taps(up, down, device, design):
    key = (up, down, tuple(sorted(design.items())), str(device))
    if key not in _device_taps:
        _device_taps[key] = torch.from_numpy(design_filter(up, down, **design).astype(np.float32)).to(device)
    return _device_taps[key]


def resample(x, fs_in, fs_out, **design):
    """x (L,) or (B, L) float32 on the GPU at ``fs_in`` -> the same at ``fs_out`` with ceil(L*up/down) samples.  Equal rates return ``x`` itself."""
    up, down = ratio(fs_in, fs_out)
    if up == down:
        return x
    if not x.is_cuda:
        raise _lib.BuddyHipError("resample: the resampler runs on the MI355X only (got a CPU tensor)")
    lib = _lib.require_gpu()
    assert x.dim() in (1, 2) and x.dtype == torch.float32, "resample takes (L,) or (B, L) float32"
    xc = x.reshape(-1, x.shape[-1]).contiguous()
    B, Lin = xc.shape
    h = _taps(up, down, x.device, design)
    Lout = out_length(Lin, up, down)
    y = torch.empty(B, Lout, dtype=torch.float32, device=x.device)
    _lib.check(lib.buddy_resample(_lib.ptr(xc), B, Lin, _lib.ptr(h), h.numel(), up, down, _lib.ptr(y), Lout, _lib.stream_ptr()))
    return y[0] if x.dim() == 1 else y
