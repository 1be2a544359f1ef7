"""Seeded sampling: per-utterance counter-based noise streams (``tester.noise.generator: philox``).

Philox4x32-10 (Salmon et al., SC'11).  A stream is the key ``stream_key(seed, name)``; sample ``i`` of draw ``d`` of purpose ``p`` is word ``i & 3``
of the block with counter ``(i >> 2, d, p, 0)`` -- a pure function of ``(seed, name, p, d, i)``, so batch composition, sub-batch policy, file order and
world size drop out by construction.  On the GPU the draws come from ``buddy_philox_fill`` / ``buddy_perturb_philox`` (``csrc/rng.hip``), where they
are consumed; this module holds the key derivation, the stream bookkeeping (``PhiloxStreams``) and a vectorised numpy restatement of the words,
uniforms and normals in float64, which serves CPU-device runs and is what the GPU tests compare the kernels against.  No reference counterpart:
the reference draws with ``torch.randn`` / ``torch.rand`` on the global generators."""
from __future__ import annotations

import hashlib
import struct

import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57            # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # Weyl key increments
SAMPLER, PHASES, UPDATE_H, RIR_REG = 0, 1, 2, 3      # purposes: sampler normals, operator uniform phases, update_H(use_noise) normals, RIR-regulariser normals
NORMAL, UNIFORM, RAW = 0, 1, 2                       # kinds of buddy_philox_fill
Z_MAX = float(np.sqrt(50.0 * np.log(2.0)))           # 5.88705: u1 >= 2^-25 truncates the normal tail there (reached by one word pair in 2^48)


def stream_key(seed, name):
    """(k0, k1): the first two little-endian uint32 of sha256(f"{seed}:{name}")"""
    return struct.unpack("<II", hashlib.sha256(f"{int(seed)}:{name}".encode()).digest()[:8])


def philox4x32_10(counter, key):
    """counter: four integer arrays (or scalars) broadcast together, key: (k0, k1) -> (..., 4) uint32 output words"""
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(*counter)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & m32, (p0 >> s32) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return np.stack(c, axis=-1).astype(np.uint32)


def words(key, purpose, draw, n):
    """the first ``n`` 32-bit words of draw ``draw`` of purpose ``purpose`` of the stream ``key``: (n,) uint32"""
    blocks = (int(n) + 3) // 4
    return philox4x32_10((np.arange(blocks, dtype=np.uint64), int(draw), int(purpose), 0), key).reshape(-1)[:int(n)]


def uniforms_from_words(w):
    """(w >> 8) 2^-24 in [0, 1), float64 (exact in fp32 as well)"""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def normals_from_words(w):
    """Box-Muller per word pair in float64: u1 = ((w_even >> 8) + 0.5) 2^-24, u2 = (w_odd >> 8) 2^-24, r = sqrt(-2 log u1),
    z_even = r cos(2 pi u2), z_odd = r sin(2 pi u2).  ``w`` of even length."""
    k = (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float64)
    r = np.sqrt(-2.0 * np.log((k[0::2] + 0.5) * 2.0 ** -24))
    a = 2.0 * np.pi * (k[1::2] * 2.0 ** -24)
    z = np.empty(k.shape[0], dtype=np.float64)
    z[0::2], z[1::2] = r * np.cos(a), r * np.sin(a)
    return z


def uniforms(key, purpose, draw, n):
    return uniforms_from_words(words(key, purpose, draw, n))


def normals(key, purpose, draw, n):
    return normals_from_words(words(key, purpose, draw, 4 * ((int(n) + 3) // 4)))[:int(n)]


class PhiloxStreams:
    """One Philox stream per utterance name, with one draw counter per purpose shared by all rows (every row takes part in every draw).
    ``len()`` and slicing work; a slice is an independent object that starts from the parent's counters (the sub-batches of
    ``testing/concurrent.py`` and ``Tester.sample_observed`` cut ``noise[lo:hi]``): its rows draw what the parent's rows would draw."""

    def __init__(self, names, seed=0, device=None, _keys=None, _dev_keys=None, _counters=None):
        self.names, self.seed = list(names), int(seed)
        self.device = torch.device("cuda" if device is None else device)
        self.keys = np.array([stream_key(self.seed, n) for n in self.names], dtype=np.uint32).reshape(-1, 2) if _keys is None else _keys
        self.counters = [0, 0, 0, 0] if _counters is None else list(_counters)
        self._dev_keys = _dev_keys             # (B, 2) int32 device tensor holding the uint32 bit patterns, made at the first GPU draw

    def __len__(self):
        return len(self.names)

    def __getitem__(self, s):
        if not isinstance(s, slice):
            raise TypeError("PhiloxStreams takes slices: its draws are batched over the rows")
        dk = None if self._dev_keys is None else self._dev_keys[s]
        return PhiloxStreams(self.names[s], self.seed, self.device, _keys=self.keys[s], _dev_keys=dk, _counters=self.counters)

    def _device_keys(self):
        if self._dev_keys is None:
            self._dev_keys = torch.from_numpy(np.ascontiguousarray(self.keys).view(np.int32).copy()).to(self.device)
        assert self._dev_keys.is_contiguous()
        return self._dev_keys

    def _take(self, purpose, count):
        d = self.counters[purpose]
        self.counters[purpose] = d + int(count)
        assert self.counters[purpose] < 2 ** 32, "draw indices are 32-bit"
        return d

    def fill(self, purpose, n, kind=NORMAL, count=1):
        """the next ``count`` draws of ``purpose``: (count, B, n) fp32 on the streams' device, ONE launch on the GPU"""
        from .. import _lib
        B, n, count = len(self), int(n), int(count)
        d0 = self._take(purpose, count)
        if self.device.type != "cuda":
            gen = {NORMAL: normals, UNIFORM: uniforms}[kind]
            host = np.stack([np.stack([gen(self.keys[b], purpose, d0 + r, n) for b in range(B)]) for r in range(count)])
            return torch.from_numpy(host.astype(np.float32))
        out = torch.empty(count, B, n, dtype=torch.float32, device=self.device)
        _lib.check(_lib.require_gpu().buddy_philox_fill(out.data_ptr(), count, B, n, self._device_keys().data_ptr(), int(purpose), d0, int(kind),
                                                        _lib.stream_ptr()))
        return out

    def randn(self, purpose, shape, count=None):
        """standard normals (B, *shape) -- or (count, B, *shape), one draw each -- of the next draw(s) of ``purpose``"""
        shape = tuple(int(v) for v in shape)
        v = self.fill(purpose, int(np.prod(shape)), NORMAL, 1 if count is None else count)
        return v.reshape(((len(self),) if count is None else (int(count), len(self))) + shape)

    def rand(self, purpose, shape):
        """uniforms in [0, 1), (B, *shape), of the next draw of ``purpose``"""
        shape = tuple(int(v) for v in shape)
        return self.fill(purpose, int(np.prod(shape)), UNIFORM).reshape((len(self),) + shape)

    def perturb(self, x, scale):
        """x + scale * eps with eps the next sampler draw (purpose 0), generated in registers: one launch, no noise tensor (x: (B, L) fp32 on the GPU).
        The bits of ``buddy_perturb(x, randn(SAMPLER, (L,)), scale)``."""
        from .. import _lib
        assert x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.shape[0] == len(self), "one noise stream per utterance, (B, L) fp32"
        x = x.contiguous()
        out = torch.empty_like(x)
        d = self._take(SAMPLER, 1)
        _lib.check(_lib.require_gpu().buddy_perturb_philox(_lib.ptr(x), self._device_keys().data_ptr(), d, float(scale), _lib.ptr(out), x.shape[0],
                                                           x.shape[1], _lib.stream_ptr()))
        return out


def factory_from_config(tester_cfg, device):
    """``tester.noise`` -> a ``noise_factory(names)`` for the harness, or None for the default (torch's generators in the reference's draw order).
    Both keys are read with defaults, so a config written before the block existed means ``generator: torch``."""
    nz = tester_cfg.get("noise", None) if hasattr(tester_cfg, "get") else None
    gen = "torch" if nz is None else str(nz.get("generator", "torch"))
    if gen == "torch":
        return None
    if gen != "philox":
        raise ValueError(f"tester.noise.generator is 'torch' or 'philox', got {gen!r}")
    seed = int(nz.get("seed", 0))
    return lambda names: PhiloxStreams(list(names), seed, device)
