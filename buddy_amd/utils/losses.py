"""Reconstruction losses -- same factory surface as reference ``utils/losses.py:17-95`` (``get_loss(loss_args, operator)`` -> ``loss(x, x_hat)``).

The product evaluates the loss INSIDE ``libbuddy_hip.so``: the sampler's fast path fuses it with the operator (``buddy_blindop_rec_loss_grad`` /
``buddy_blindop_fir_loss_grad`` / ``buddy_blindop_optimize``: STFT-1024/512/128, loss, analytic adjoints), and the object ``get_loss`` returns is
CALLABLE like the reference's: ``loss(x, x_hat)`` is one library call (``buddy_blindop_stft_loss``) behind a ``torch.autograd.Function``, differentiable
w.r.t. either argument, so the reference's own ``get_likelihood_score`` / ``optimize_op`` (``testing/EulerHeunSamplerDPS.py:61-113``) run on it unmodified.

Supported: every name of the reference -- the compressed-spectrum family ``l2_comp_stft_{summean,sum,mean}`` (the shipped one is summean @ 0.667) with
any compression factor in (0, 1], ``l2_stft_sum``, ``l2_stft_mag_sum``, ``l2_stft_logmag_sum``, ``l2_log_stft_sum``, the time-domain ``l2_sum`` /
``l2_mean``, the optional ``freq_weighting`` (``sqrt`` / ``exp`` / ``log`` / ``linear``) of the STFT losses, and hybrids (``loss_1``, ``loss_2``, ...:
``:22-23``) through the callable.  The library handle holds one loss descriptor per term (slot 0 likelihood, 1 operator fit, 2 RIR-noise regulariser,
3 this callable; ``buddy_blindop_set_loss``).  The formulas as torch expressions live in ``oracle/batched/losses.py`` (test infrastructure).
Per-utterance semantics: the library returns one loss per utterance (``operator.last_loss_per_utt``) and the call returns their sum, so gradients
decouple per utterance."""
from __future__ import annotations

import numpy as np

# library loss kinds (include/buddy_hip.h, buddy_blindop_set_loss)
STFT_KINDS = {"l2_comp_stft_summean": 0, "l2_comp_stft_sum": 1, "l2_comp_stft_mean": 2, "l2_stft_sum": 3, "l2_stft_mag_sum": 4,
              "l2_stft_logmag_sum": 5, "l2_log_stft_sum": 6}
TIME_KINDS = {"l2_sum": 7, "l2_mean": 8}
KIND = {**STFT_KINDS, **TIME_KINDS}
KIND_NONE = 9
COMP_NAMES = ("l2_comp_stft_summean", "l2_comp_stft_sum", "l2_comp_stft_mean")
SUPPORTED = tuple(KIND)
NORM_MODE = {n: KIND[n] for n in COMP_NAMES}
WEIGHTING = {None: 0, "sqrt": 1, "exp": 2, "log": 3, "linear": 4}
COMPRESSION = 0.667          # the shipped configs' factor (conf/tester/*.yaml)
N_BINS = 513                 # operator STFT 1024 -> 513 bins


def weight_table(freq_weighting, n_bins=N_BINS):
    """the per-bin weights of reference ``get_frequency_weighting`` (utils/losses.py:3-14) on ``linspace(0, 1, n_bins) + 1``, float32, by the
    reference's op order (torch on the host); None for no weighting"""
    if freq_weighting is None:
        return None
    import torch
    f = torch.linspace(0, 1, n_bins) + 1
    if freq_weighting == "sqrt":
        w = torch.sqrt(f)
    elif freq_weighting == "exp":
        e = torch.exp(f)
        w = e - e[0]
    elif freq_weighting == "log":
        w = torch.log(1 + f)
    elif freq_weighting == "linear":
        w = f
    else:
        raise ValueError(f"freq_weighting {freq_weighting!r}: one of sqrt, exp, log, linear")
    return np.ascontiguousarray(w.numpy(), dtype=np.float32)


def bind_slot(h, slot, spec, uploaded=None):
    """point slot ``slot`` of library handle ``h`` at LossSpec ``spec`` (None: kind none); the weight table goes to the handle once
    (``uploaded``: a set of (handle, weighting) pairs already sent)"""
    from .. import _lib
    lib = _lib.load()
    if spec is None:
        _lib.check(lib.buddy_blindop_set_loss(h, int(slot), KIND_NONE, 0, float(COMPRESSION)))
        return
    fw = spec.fw_code
    key = (int(h.value if hasattr(h, "value") else h), fw)
    if fw and (uploaded is None or key not in uploaded):
        w = weight_table(spec.freq_weighting)
        _lib.check(lib.buddy_blindop_set_freq_weights(h, fw, w.ctypes.data))
        if uploaded is not None:
            uploaded.add(key)
    _lib.check(lib.buddy_blindop_set_loss(h, int(slot), spec.kind, fw, float(spec.compression_factor)))


class LossSpec:
    """A validated loss block: name, weight, compression factor, frequency weighting -- and, bound to an operator, the loss itself: ``spec(x, x_hat)``."""

    def __init__(self, name, weight, compression_factor, operator=None, freq_weighting=None):
        self.name, self.weight, self.operator = name, float(weight), operator
        self.compression_factor = float(COMPRESSION if compression_factor is None else compression_factor)
        self.freq_weighting = freq_weighting
        self.kind, self.fw_code = KIND[name], WEIGHTING[freq_weighting]

    @property
    def time_domain(self):
        return self.name in TIME_KINDS

    def __call__(self, x, x_hat):
        op = self.operator
        if op is None or not hasattr(op, "_loss_handle"):
            raise NotImplementedError(f"loss '{self.name}' needs an operator with a HIP loss handle (get_loss(loss_args, operator=...))")
        from ..testing.operators.subband_filtering import _StftLossFn
        a = x.unsqueeze(0) if x.dim() == 1 else x
        b = x_hat.unsqueeze(0) if x_hat.dim() == 1 else x_hat
        if a.shape != b.shape or a.dim() != 2 or not a.is_cuda:
            raise NotImplementedError(f"loss '{self.name}': two (U, L) GPU tensors of one shape expected, got {tuple(x.shape)} and {tuple(x_hat.shape)}")
        h = op._loss_handle(int(a.shape[0]), int(a.shape[1]))
        if not hasattr(op, "_fw_uploaded"):
            op.__dict__["_fw_uploaded"] = set()
        bind_slot(h, 3, self, op._fw_uploaded)         # slot 3 is the callable's own: the fused calls' slots stay as bound
        return _StftLossFn.apply(a, b, h, self.weight, op)

    def __repr__(self):
        return (f"LossSpec({self.name!r}, weight={self.weight}, compression_factor={self.compression_factor}"
                + (f", freq_weighting={self.freq_weighting!r})" if self.freq_weighting else ")"))


class HybridLoss:
    """sum of member losses (reference utils/losses.py:22-23); callable like them.  The operator's FUSED calls take one member only and refuse this."""

    def __init__(self, parts):
        self.parts, self.name = parts, "hybrid"

    def __call__(self, x, x_hat):
        out = self.parts[0](x, x_hat)
        for p in self.parts[1:]:
            out = out + p(x, x_hat)
        return out


def get_loss(loss_args, operator=None):
    if loss_args.name == "none":
        return None
    if hasattr(loss_args, "loss_1"):        # a hybrid: the sum of its members (reference :22-23), through the callable only
        parts = [get_loss(loss_args[k], operator=operator) for k in loss_args.keys() if str(k).startswith("loss_")]
        return HybridLoss([p for p in parts if p is not None])
    name = loss_args.name
    if name not in KIND:
        raise NotImplementedError(f"rec_loss {name} not implemented (the reference's names: {SUPPORTED})")
    c = loss_args.get("compression_factor", None)
    if name in COMP_NAMES and (c is None or not (0.0 < float(c) <= 1.0)):
        raise NotImplementedError(f"compression_factor {c}: the reference asserts 0 < factor <= 1 (utils/losses.py:60)")
    # the reference reads the key ``freq_weighting`` (utils/losses.py:30) and only for the STFT losses; the shipped configs set ``frequency_weighting``,
    # which it never reads (appendix B.8) -- nor does this
    fw = loss_args.get("freq_weighting", None) if name in STFT_KINDS else None
    if fw is not None and fw not in WEIGHTING:
        raise ValueError(f"freq_weighting {fw!r}: one of sqrt, exp, log, linear")
    return LossSpec(name, loss_args.get("weight", 1.0), c if name in COMP_NAMES else None, operator, fw)
