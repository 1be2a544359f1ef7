"""``NCSNppTime`` -- the reference's score-network plug point (``networks.ncsnpp.NCSNppTime``,
reference ``networks/ncsnpp.py:455-506``) backed by the hand-written gfx950 network in ``libbuddy_hip.so``.

Same surface as the reference class: constructor kwargs = ``conf/network/ncsnpp.yaml`` keys (incl. nested
``stft:{n_fft,hop_length,center}``), ``nn.Module`` protocol with the reference ``state_dict`` key names
(``all_modules.N.*``, ``output_layer.*``), ``forward(x:(B,1,L) f32, time_cond:(B,) f32) -> (B,1,L)``,
differentiable w.r.t. ``x`` (the input-VJP runs in HIP).  Parameters are registered with ``requires_grad=False``; after
``net.requires_grad_(True)`` the module is trainable: the parameter gradients run in HIP too (``buddy_ncsnpp_vjp_params``), and the
weights an optimizer changed in place are pushed to the library at the next forward (``buddy_ncsnpp_update_params``).
Only the shipped architecture family is supported (biggan resblocks, input_skip/sum, output_skip, the bottleneck attention plus the
attention sites of ``attn_resolutions``;
``fir`` False or True with the (1,3,3,1) kernel); anything else raises ``NotImplementedError`` at construction.
"""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..synth import attn_mask_of, module_specs


class _Bag(nn.Module):
    """parameter container; gives nested state-dict names without any compute."""


def _variance_scaling_uniform(shape, scale, in_axis, out_axis):
    # default_init: variance_scaling(scale, 'fan_avg', 'uniform') -- reference layers.py:54-91
    scale = 1e-10 if scale == 0 else scale
    rf = np.prod(shape) / shape[in_axis] / shape[out_axis]
    fan_in, fan_out = shape[in_axis] * rf, shape[out_axis] * rf
    var = scale / ((fan_in + fan_out) / 2)
    return (torch.rand(*shape) * 2.0 - 1.0) * np.sqrt(3 * var)


class _NetFn(torch.autograd.Function):
    # params: empty (inference, input-VJP only) or every parameter in the flat order of the library (training: save = 2)
    @staticmethod
    def forward(ctx, x, cnoise, scal, net, *params):
        B, L = x.shape
        lib = _lib.require_gpu()
        x = x.contiguous()
        y = torch.empty_like(x)
        ctx.train = any(ctx.needs_input_grad[4:])
        save = 2 if ctx.train else (1 if ctx.needs_input_grad[0] else 0)
        cin = cskip = cout = None
        if scal is not None:
            cin, cskip, cout = (s.contiguous() for s in scal)
        _lib.check(lib.buddy_ncsnpp_forward(net._get_handle(), _lib.ptr(x), _lib.ptr(cnoise.contiguous()), _lib.ptr(cin),
                                            _lib.ptr(cskip), _lib.ptr(cout), _lib.ptr(y), B, L, save, _lib.stream_ptr()))
        net._fwd_id += 1
        ctx.net, ctx.fwd_id = net, net._fwd_id
        ctx.saved_params = params
        return y

    @staticmethod
    def backward(ctx, g):
        net = ctx.net
        if ctx.fwd_id != net._fwd_id:
            raise _lib.BuddyHipError("backward through a stale NCSNppTime forward: the handle keeps one tape (call "
                                     "backward before the next forward)")
        g = g.contiguous()
        if not ctx.train:
            gx = torch.empty_like(g)
            _lib.check(_lib.load().buddy_ncsnpp_vjp(net._get_handle(), _lib.ptr(g), _lib.ptr(gx), _lib.stream_ptr()))
            return (gx, None, None, None) + (None,) * (len(ctx.needs_input_grad) - 4)
        gx = torch.empty_like(g) if ctx.needs_input_grad[0] else None
        if net._grad_flat is not None:
            # an optimizer owns the flat gradient buffer (attach_flat): written in place -- the parameters' .grad are views of it -- and no gradient
            # goes through autograd's accumulation.  The first backward after zero_grad overwrites, later ones add (torch's accumulate semantics)
            gp = net._grad_flat
            if gp.device != g.device:
                raise _lib.BuddyHipError(f"the attached gradient buffer is on {gp.device}, the backward runs on {g.device}")
            _lib.check(_lib.load().buddy_ncsnpp_vjp_params(net._get_handle(), _lib.ptr(g), _lib.ptr(gx), _lib.ptr(gp), int(net._grad_filled),
                                                           _lib.stream_ptr()))
            net._grad_filled = True
            return (gx, None, None, None) + (None,) * (len(ctx.needs_input_grad) - 4)
        gp = torch.empty(net._n_params, dtype=torch.float32, device=g.device)
        _lib.check(_lib.load().buddy_ncsnpp_vjp_params(net._get_handle(), _lib.ptr(g), _lib.ptr(gx), _lib.ptr(gp), 0, _lib.stream_ptr()))
        grads = []
        for (name, shape, kind, _), (off, n), p, need in zip(net._specs, net._offsets, ctx.saved_params, ctx.needs_input_grad[4:]):
            # the Fourier projection W has no gradient (reference layerspp.py: requires_grad=False): None, so optimizers skip it
            grads.append(gp[off:off + n].view(shape).to(p.device) if need and kind != "fourier" else None)
        return (gx, None, None, None) + tuple(grads)


class NCSNppTime(nn.Module):
    ATTENTION_MODES = {"flash": 0, "bf16": 1, "f16": 2, "matrix": 3, "auto": 4}
    GEMM_MODES = {"fp32": 0, "bf16x3": 1, "f16x2": 2, "f16": 3}       # "f16": opt-in fast mode (include/buddy_hip.h, buddy_ncsnpp_set_gemm)

    def __init__(self, stft=None, nonlinearity="swish", nf=128, ch_mult=(1, 2, 2, 2), num_res_blocks=1,
                 attn_resolutions=(0,), resamp_with_conv=True, time_conditional=True, fir=False,
                 fir_kernel=(1, 3, 3, 1), skip_rescale=True, resblock_type="biggan", progressive="output_skip",
                 progressive_input="input_skip", progressive_combine="sum", init_scale=0.0, fourier_scale=16,
                 image_size=256, embedding_type="fourier", input_channels=2, spatial_channels=1, dropout=0.0,
                 centered=True, discriminative=False, attention=None, gemm=None, **kwargs):
        super().__init__()
        self._init_kwargs = dict(stft=stft, nonlinearity=nonlinearity, nf=nf, ch_mult=ch_mult, num_res_blocks=num_res_blocks,
                                 attn_resolutions=attn_resolutions, resamp_with_conv=resamp_with_conv, time_conditional=time_conditional,
                                 fir=fir, fir_kernel=fir_kernel, skip_rescale=skip_rescale, resblock_type=resblock_type,
                                 progressive=progressive, progressive_input=progressive_input, progressive_combine=progressive_combine,
                                 init_scale=init_scale, fourier_scale=fourier_scale, image_size=image_size, embedding_type=embedding_type,
                                 input_channels=input_channels, spatial_channels=spatial_channels, dropout=dropout, centered=centered,
                                 discriminative=discriminative, attention=attention, gemm=gemm)
        assert stft is not None, "stft must be provided"          # reference ncsnpp.py:459
        unsupported = []
        if nonlinearity != "swish": unsupported.append("nonlinearity")
        if fir and tuple(int(v) for v in fir_kernel) != (1, 3, 3, 1): unsupported.append("fir_kernel other than (1, 3, 3, 1)")
        if not skip_rescale: unsupported.append("skip_rescale=False")
        if str(resblock_type).lower() != "biggan": unsupported.append("resblock_type")
        if str(progressive).lower() != "output_skip": unsupported.append("progressive")
        if str(progressive_input).lower() != "input_skip": unsupported.append("progressive_input")
        if str(progressive_combine).lower() != "sum": unsupported.append("progressive_combine")
        if str(embedding_type).lower() != "fourier": unsupported.append("embedding_type")
        if input_channels != 2 or spatial_channels != 1: unsupported.append("channels")
        if not time_conditional or discriminative or not centered or dropout not in (0, 0.0):
            unsupported.append("time_conditional/discriminative/centered/dropout")
        if nf % 32: unsupported.append("nf % 32")
        if unsupported:
            raise NotImplementedError("NCSNppTime (MI355X): unsupported options: " + ", ".join(unsupported))
        get = (lambda k: stft[k]) if isinstance(stft, dict) else (lambda k: getattr(stft, k))
        self.stft_kwargs = stft
        self.n_fft, self.hop_length = int(get("n_fft")), int(get("hop_length"))
        # attention sites: the reference BUILDS an AttnBlock where image_size // 2^l is in attn_resolutions (ncsnpp.py:195, 232) and RUNS one where the
        # tensor height -- the frequency bins F >> l -- is (:340, :387).  Where the two tests disagree its module index goes out of step: refused.
        R = tuple(int(r) for r in attn_resolutions)
        bins = self.n_fft // 2 + 1
        for lvl in range(len(ch_mult)):
            built, run = (int(image_size) >> lvl) in R, (bins >> lvl) in R
            if built != run:
                raise NotImplementedError(f"NCSNppTime (MI355X): attn_resolutions={list(R)} selects level {lvl} for image_size={image_size} "
                                          f"(resolution {int(image_size) >> lvl}: {'built' if built else 'not built'}) but not for the {bins} frequency "
                                          f"bins of n_fft={self.n_fft} (height {bins >> lvl}: {'run' if run else 'not run'}); the reference would "
                                          "build and run different attention blocks")
        self.attn_mask = attn_mask_of(R, image_size, len(ch_mult))
        assert bool(get("center")), "center=False not supported"
        self.nf, self.ch_mult, self.num_res_blocks = int(nf), tuple(int(c) for c in ch_mult), int(num_res_blocks)
        # attention core: None = library default (BUDDY_ATTN, else "auto": fp32, materialised while T <= 4096, flash beyond); "auto" | "flash" | "bf16" | "f16" | "matrix" (build extension, not a reference key:
        # bf16 / f16 are the opt-in fast mode of DESIGN.md section 4.3)
        if attention is not None and attention not in self.ATTENTION_MODES:
            raise NotImplementedError(f"attention must be one of {sorted(self.ATTENTION_MODES)}")
        self.attention = attention
        # arithmetic of the Winograd-domain GEMMs (build extension): None = library default (BUDDY_GEMM, else "f16x2": power-of-two-scaled two-term
        # f16 split of the fp32 operands, 2^-22, three f16 MFMA products); "bf16x3" = exact three-way bf16 split, six products; "fp32" = v_mfma_f32_32x32x2_f32
        if gemm is not None and gemm not in self.GEMM_MODES:
            raise NotImplementedError(f"gemm must be one of {sorted(self.GEMM_MODES)}")
        self.gemm = gemm
        self._options = {}              # per-handle launcher options set through set_option (build extension; keys: include/buddy_hip.h)
        self.fir = bool(fir)            # FIR (1,3,3,1) resampling instead of nearest / box (reference up_or_down_sampling.py:195-257); no parameters
        self._specs = module_specs(self.nf, self.ch_mult, self.num_res_blocks, attn_mask=self.attn_mask)
        # The architecture family (reference ncsnpp.py:184-270) is built for any level / block count (fixtures net_cm12_rb2, net_cm1122_rb1), with one
        # restriction of the GroupNorm kernels: they normalise float4 channel quads with one group's statistics, so every normalised tensor -- skip
        # concatenations included -- needs a multiple of 4 channels per group: C <= 128 or C % 128 == 0 (min(C // 4, 32) groups).  nf = 32 / 128 with the
        # reference's multipliers fit; nf = 64, ch_mult (1, 2, 2, 2) has a 192-channel concatenation (six per group) and is refused here.
        bad = sorted({shape[0] for name, shape, kind, _ in self._specs if kind == "gamma" and (shape[0] % 4 or (shape[0] > 128 and shape[0] % 128))})
        if bad:
            raise NotImplementedError(f"NCSNppTime (MI355X): unsupported width nf={self.nf}, ch_mult={self.ch_mult}: GroupNorm over {bad} channels "
                                      "(channels per group must be a multiple of 4: C <= 128 or C % 128 == 0)")
        # parameter containers under the reference names
        n_mod = 1 + max(int(n.split(".")[1]) for n, *_ in self._specs if n.startswith("all_modules."))
        self.all_modules = nn.ModuleList([_Bag() for _ in range(n_mod)])
        self.output_layer = _Bag()
        for name, shape, kind, _ in self._specs:
            parts = name.split(".")
            node = self
            for p in parts[:-1]:
                if p.isdigit():
                    node = node[int(p)]
                else:
                    if not hasattr(node, p):
                        setattr(node, p, _Bag())
                    node = getattr(node, p)
            node.register_parameter(parts[-1], nn.Parameter(self._init(name, shape, kind, init_scale, fourier_scale),
                                                            requires_grad=False))
        self._handle = None
        self._fwd_id = 0
        self._parent = None
        self._offsets, o = [], 0
        for _, shape, _, _ in self._specs:
            n = int(np.prod(shape))
            self._offsets.append((o, n))
            o += n
        self._n_params = o
        self._plist = None          # the parameters in the flat order (built on first use)
        self._watch = False         # set by the first training forward (and in deep copies): forwards check the parameters' versions
        self._synced = None         # the parameters' _version when the library last received them
        self._flat = None           # attach_flat: ONE device buffer in the library's flat order that every parameter's .data is a view of
        self._flat_dirty = False    # params_changed: a kernel wrote the flat buffer behind torch's back (no _version moved)
        self._grad_flat = None      # attach_flat: the optimizer's flat gradient buffer that buddy_ncsnpp_vjp_params writes into
        self._grad_filled = False   # the gradient buffer holds a gradient since the last zero_grad (the next backward adds to it)

    @staticmethod
    def _init(name, shape, kind, init_scale, fourier_scale):
        if kind == "fourier":
            return torch.randn(*shape) * fourier_scale                      # layerspp.py:37
        if kind in ("b", "beta"):
            return torch.zeros(*shape)
        if kind == "gamma":
            return torch.ones(*shape)
        leaf = name.split(".")[-2] if name.count(".") >= 2 else ""
        scaled = leaf in ("Conv_1", "NIN_3") or (len(shape) == 4 and shape[0] == 2 and shape[2] == 3)
        if name.endswith(".W"):                                             # NIN (in, out): layers.py:551
            return _variance_scaling_uniform(shape, init_scale if scaled else 0.1, 0, 1)
        if name.startswith("output_layer"):
            return _variance_scaling_uniform(shape, 1.0, 1, 0)
        return _variance_scaling_uniform(shape, init_scale if scaled else 1.0, 1, 0)

    # ---- handle management ---------------------------------------------------------------------------
    def _flat_params(self):
        sd = self.state_dict()
        return np.concatenate([sd[n].detach().float().cpu().numpy().ravel() for n, *_ in self._specs]).astype(np.float32)

    def _drop_handle(self):
        if getattr(self, "_handle", None) is not None:
            _lib.load().buddy_ncsnpp_destroy(self._handle)
        self._handle = None

    def _get_handle(self):
        if self._handle is None and getattr(self, "_parent", None) is not None:
            h = C.c_void_p()
            lib = _lib.require_gpu()
            _lib.check(lib.buddy_ncsnpp_replica(self._parent._get_handle(), C.byref(h)))
            if self.attention is not None:      # per-handle setting: a replica may run another attention core on the shared weights
                _lib.check(lib.buddy_ncsnpp_set_attention(h, self.ATTENTION_MODES[self.attention]))
            for k, v in self._options.items():
                _lib.check(lib.buddy_ncsnpp_set_option(h, k.encode(), int(v)))
            self._handle = h
            self._synced = self._versions()
        if self._handle is None:
            lib = _lib.require_gpu()
            blob = np.ascontiguousarray(self._flat_params())
            cm = (C.c_int * len(self.ch_mult))(*self.ch_mult)
            h = C.c_void_p()
            if self.attn_mask:
                _lib.check(lib.buddy_ncsnpp_create_attn(blob.ctypes.data, blob.size, self.nf, cm, len(self.ch_mult), self.num_res_blocks,
                                                        self.n_fft, self.hop_length, self.attn_mask, C.byref(h)))
            else:
                _lib.check(lib.buddy_ncsnpp_create(blob.ctypes.data, blob.size, self.nf, cm, len(self.ch_mult),
                                                   self.num_res_blocks, self.n_fft, self.hop_length, C.byref(h)))
            if self.fir:
                _lib.check(lib.buddy_ncsnpp_set_fir(h, 1))
            if self.attention is not None:
                _lib.check(lib.buddy_ncsnpp_set_attention(h, self.ATTENTION_MODES[self.attention]))
            if self.gemm is not None:
                _lib.check(lib.buddy_ncsnpp_set_gemm(h, self.GEMM_MODES[self.gemm]))
            for k, v in self._options.items():
                _lib.check(lib.buddy_ncsnpp_set_option(h, k.encode(), int(v)))
            self._handle = h
            self._synced = self._versions()
        return self._handle

    # ---- training: parameters as autograd inputs, freshness after in-place optimizer steps ----------------------------
    def _params(self):
        if self._plist is None:
            named = dict(self.named_parameters())
            self._plist = [named[n] for n, *_ in self._specs]
        return self._plist

    def _versions(self):
        return tuple(p._version for p in self._params())

    def _sync_params(self, device):
        """After an in-place change of the parameters (optimizer step, EMA update, a copy_ before fine-tuning) push them to the library's
        weight store (``buddy_ncsnpp_update_params``: no new handle).  Watched once the module trains (any parameter requires grad), has
        trained, or is a deep copy.  ``device``: the GPU the call runs on (its input's device)."""
        if not self._watch and torch.is_grad_enabled() and any(p.requires_grad for p in self._params()):
            self._watch = True          # before the check: weights changed in place while the module was not yet watched are caught too
        if self._handle is None:
            self._flat_dirty = False    # the handle is made from the parameters as they are now
        if not self._watch or self._handle is None:
            return
        v = self._versions()
        if v == self._synced and not self._flat_dirty:
            return
        if self._flat is not None:      # the parameters ARE this buffer: nothing to gather
            flat = self._flat
            if flat.device != torch.device(device):
                raise _lib.BuddyHipError(f"the attached flat parameter buffer is on {flat.device}, the forward runs on {device}")
        else:
            with torch.no_grad():
                flat = torch.cat([p.detach().reshape(-1).float().to(device) for p in self._params()])
        _lib.check(_lib.require_gpu().buddy_ncsnpp_update_params(self._handle, _lib.ptr(flat), _lib.stream_ptr()))
        self._synced = v
        self._flat_dirty = False

    def attach_flat(self, with_grad=False):
        """Move the parameters onto ONE flat fp32 device buffer in the library's order (the order of ``buddy_ncsnpp_create`` and of
        ``grad_params``) and re-point every ``param.data`` at its view; returns the buffer.  From then on the weight push uses it directly
        (no ``torch.cat``) and a kernel may update all weights in one pass: it then calls ``params_changed()``.  ``with_grad``: also returns a
        flat gradient buffer; ``buddy_ncsnpp_vjp_params`` writes into it, and the ``.grad`` of every parameter that requires grad is a view
        of it.  ``.to()`` / ``.cuda()`` afterwards detach both (the module then behaves as before)."""
        ps = self._params()
        dev = ps[0].device
        if dev.type != "cuda" or any(p.device != dev or p.dtype != torch.float32 for p in ps):
            raise _lib.BuddyHipError("attach_flat: the parameters must be fp32 on one GPU (there is no CPU path): move the module first")
        if self._flat is None:
            with torch.no_grad():
                flat = torch.cat([p.detach().reshape(-1) for p in ps])
            for p, (off, n) in zip(ps, self._offsets):
                p.data = flat[off:off + n].view(p.shape)
            self._flat = flat
            self._watch = True
            self._synced = None         # the data is the same, the tensors are not: the next forward pushes once
        if with_grad and self._grad_flat is None:
            self._grad_flat = torch.zeros(self._n_params, dtype=torch.float32, device=dev)
            self._grad_filled = False
            for p, (off, n) in zip(ps, self._offsets):
                if p.requires_grad:
                    p.grad = self._grad_flat[off:off + n].view(p.shape)
        return (self._flat, self._grad_flat) if with_grad else self._flat

    def params_changed(self):
        """A kernel wrote the attached flat parameter buffer (no ``_version`` moved): the next forward pushes the weights to the library"""
        if self._flat is None:
            raise _lib.BuddyHipError("params_changed without attach_flat: the parameters are separate tensors, torch tracks their versions")
        self._watch = True
        self._flat_dirty = True

    def grads_zeroed(self):
        """The optimizer's ``zero_grad``: the next backward overwrites the attached gradient buffer instead of adding to it"""
        self._grad_filled = False

    def _train_params(self):
        """The parameters as autograd inputs when any of them requires grad (training), else ()"""
        if not torch.is_grad_enabled():
            return ()
        ps = self._params()
        if not any(p.requires_grad for p in ps):
            return ()
        self._watch = True
        return tuple(ps)

    def __deepcopy__(self, memo):
        """EMA copies (reference trainer: copy.deepcopy(network)): the copy gets its own library handle on first use, never the original's"""
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k in ("_handle", "_parent", "_plist", "_synced", "_flat", "_grad_flat"):
                new.__dict__[k] = None
            else:
                new.__dict__[k] = copy.deepcopy(v, memo)
        new._fwd_id = 0
        new._watch = True
        new._flat_dirty = new._grad_filled = False      # the copy's parameters are separate tensors again (attach_flat gives it its own buffer)
        return new

    def set_option(self, key, value):
        """Per-handle launcher option (``buddy_ncsnpp_set_option``: fusion / layout A/B switches, attention core, GEMM arithmetic; an unknown key or
        a value out of range raises).  Applies to this module's handle only -- a replica made afterwards starts from the same settings."""
        lib = _lib.load()
        _lib.check(lib.buddy_option_validate(str(key).encode(), int(value)))     # BEFORE it is remembered: a rejected entry would be replayed (and
        if getattr(self, "_handle", None) is not None:                            # rejected) by every later handle and replica of this module
            _lib.check(lib.buddy_ncsnpp_set_option(self._handle, str(key).encode(), int(value)))
        self._options[str(key)] = int(value)
        return self

    def get_option(self, key):
        v = C.c_int()
        _lib.check(_lib.load().buddy_ncsnpp_get_option(self._get_handle(), str(key).encode(), C.byref(v)))
        return v.value

    def replica(self, attention=None):
        """A second module on the SAME parameters and the same prepared device weights (``buddy_ncsnpp_replica``: reference-counted, read-only)
        with its own library handle -- activation arena + VJP tape -- so another sub-batch can run concurrently on another HIP stream
        (buddy_amd/testing/concurrent.py).  Costs no weight memory and no preparation time.  ``attention``: the replica's attention core (per-handle).  A replica follows the weights its parent had
        when the replica's handle was made; reload the parent -> make new replicas."""
        if attention is not None and attention not in self.ATTENTION_MODES:   # validate BEFORE copying: a half-built copy still holds the parent's handle
            raise NotImplementedError(f"attention must be one of {sorted(self.ATTENTION_MODES)}")
        r = copy.copy(self)                     # shallow: shares _parameters / _modules (the nn.Parameters themselves)
        r.__dict__["_options"] = dict(self._options)
        r.__dict__["_handle"] = None            # first thing: the copy must never own (and on collection destroy) the parent's library handle
        if attention is not None:
            r.attention = attention
        r._fwd_id = 0
        object.__setattr__(r, "_parent", self)   # not a submodule: nn.Module.__setattr__ would register it in the shared _modules
        return r

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._plist = None
        self._drop_handle()
        self._parent = None                     # new weights: this module owns its handle again
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._plist = None
        if self._flat is not None and any(p.data_ptr() != self._flat.data_ptr() + 4 * off for p, (off, _) in zip(self._params(), self._offsets)):
            self._flat = self._grad_flat = None      # .to() / .cuda() gave the parameters new tensors: an attached optimizer notices and refuses
            self._flat_dirty = self._grad_filled = False
        self._drop_handle()
        self._parent = None
        return r

    def __del__(self):
        try:
            self._drop_handle()
        except Exception:
            pass

    def weight_bytes(self):
        """Device bytes of the (shared) weight store: {'params', 'packed_1x1', 'conv3_forms', 'conv3_form_count'}."""
        a, b, c, n = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_int()
        _lib.check(_lib.require_gpu().buddy_ncsnpp_weight_bytes(self._get_handle(), C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return {"params": a.value, "packed_1x1": b.value, "conv3_forms": c.value, "conv3_form_count": n.value}

    def arena_bytes(self, B, L, with_vjp=True):
        n = C.c_longlong()
        _lib.check(_lib.require_gpu().buddy_ncsnpp_reserve(self._get_handle(), B, L, int(with_vjp), C.byref(n)))
        return n.value

    # ---- compute -------------------------------------------------------------------------------------
    def forward(self, x, time_cond=None):
        """x: (B,1,L) (reference signature) or (B,L); time_cond: (B,) = c_noise."""
        squeeze = x.dim() == 3
        x2 = x[:, 0] if squeeze else x
        self._sync_params(x2.device)
        y = _NetFn.apply(x2.float(), time_cond.float().reshape(-1), None, self, *self._train_params())
        return y[:, None] if squeeze else y

    def denoise_fused(self, x, cnoise, cin, cskip, cout):
        """EDM denoiser with the preconditioning scalars folded into the STFT / overlap-add kernels:
        cskip[b]*x + cout[b]*net(cin[b]*x, cnoise[b]) (reference diff_params/shared.py:98-120).  x: (B,L); rest (B,)."""
        self._sync_params(x.device)
        return _NetFn.apply(x.float(), cnoise.float(), (cin.float(), cskip.float(), cout.float()), self, *self._train_params())

    def denoise_saved(self, x, scal4):
        """The EDM denoiser (as ``denoise_fused``) WITHOUT an autograd graph: forward with the handle's VJP tape kept; pair it with ``input_vjp``.
        The sampler's fast path (round 6) calls the two library entries directly -- no autograd engine, no ones / sum / mul helper kernels around
        them.  x (B, L); scal4 (4, B) = rows (cnoise, cin, cskip, cout)."""
        lib = _lib.require_gpu()
        x = x.contiguous().float()
        B, L = x.shape
        y = torch.empty_like(x)
        self._sync_params(x.device)
        _lib.check(lib.buddy_ncsnpp_forward(self._get_handle(), _lib.ptr(x), _lib.ptr(scal4[0]), _lib.ptr(scal4[1]), _lib.ptr(scal4[2]), _lib.ptr(scal4[3]),
                                            _lib.ptr(y), B, L, 1, _lib.stream_ptr()))
        self._fwd_id += 1           # an autograd node of an earlier forward is stale from here on
        return y

    def input_vjp(self, g):
        """(d denoise_saved / d x)^T g for the last ``denoise_saved`` (``buddy_ncsnpp_vjp``)"""
        g = g.contiguous().float()
        gx = torch.empty_like(g)
        _lib.check(_lib.load().buddy_ncsnpp_vjp(self._get_handle(), _lib.ptr(g), _lib.ptr(gx), _lib.stream_ptr()))
        return gx

    def tap(self, module_idx):
        """(B, frames, bins, C) copy of all_modules[module_idx]'s output from the last forward (parity tests)."""
        p = C.c_void_p()
        dims = (C.c_int * 4)()
        _lib.check(_lib.load().buddy_ncsnpp_tap(self._get_handle(), module_idx, C.byref(p), C.byref(dims)))
        n = int(np.prod(list(dims)))
        out = torch.empty(tuple(dims), dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().buddy_copy_d2d(out.data_ptr(), p, n * 4, _lib.stream_ptr()))
        torch.cuda.synchronize()
        return out
