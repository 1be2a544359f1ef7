"""``FusedAdam`` -- the optimizer of the training loop on the MI355X: gradient clipping, the Adam update and the EMA of the weights as two
library calls per step (``buddy_optim_sqnorm``, ``buddy_optim_step``; ``csrc/optim.hip``) on flat fp32 buffers, whatever the number of
parameter tensors.

It is a ``torch.optim.Optimizer`` with the constructor the reference's yaml gives its optimizer (``params, lr, betas, eps``) and the
``state_dict()`` / ``load_state_dict()`` layout of torch's own Adam with default options, so a checkpoint written by either loads into the
other (strategy 1 of ``utils/training_utils.py``).  The layout, as ``state_dict_layout`` restates it without a GPU:

    state         {index: {'step': 0-dim fp32 CPU tensor, 'exp_avg': tensor, 'exp_avg_sq': tensor}} for every parameter that has been
                  stepped, index = its position in ``params``; a parameter without gradient (the Fourier projection W) has no entry
    param_groups  one group: ``GROUP_DEFAULTS`` with lr / betas / eps as given, and 'params' = [0 .. N-1]

On construction the network's parameters move onto ONE flat buffer in the library's order (``NCSNppTime.attach_flat``); ``exp_avg`` and
``exp_avg_sq`` of every parameter are views of two more flat buffers, and the ``.grad`` of every parameter is a view of the flat gradient
buffer that ``buddy_ncsnpp_vjp_params`` writes.  There is no CPU path: without the library or a GPU construction raises ``BuddyHipError``.

Data parallelism (``attach_group``): every rank holds a full replica; ``step()`` runs ONE ``all_reduce(SUM)`` on the flat gradient buffer and
``buddy_optim_step_scaled`` with ``grad_scale = 1 / world`` turns the sum into the average inside the same pass (clipping included).
``broadcast_state`` makes the replicas equal, ``check_replicas`` proves that they still are: four 64-bit checksums per rank
(``buddy_optim_checksum``), gathered and compared.  With the ``nccl`` backend (RCCL) the collectives take the device buffers; with any other
backend (gloo: ranks sharing a GPU in tests) they are staged through one pinned host buffer that is allocated once."""
from __future__ import annotations

import ctypes as C
import math

import torch

from .. import _lib

# the option fields of a torch Adam group with every option at its default (checked against torch's own in tests/test_trainer_host.py)
GROUP_DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False,
                      differentiable=False, fused=None, decoupled_weight_decay=False)
STATE_KEYS = ("step", "exp_avg", "exp_avg_sq")
REPLICA_BUFFERS = ("param", "exp_avg", "exp_avg_sq", "ema")     # the rows of replica_checksums(), as check_replicas names them


def replica_disagreements(table):
    """``table``: world x 4 checksums (rows = ranks, columns = ``REPLICA_BUFFERS``) -> [(buffer name, [ranks that differ from rank 0])] for every
    buffer on which the ranks do not all agree.  Plain integers in, plain data out: needs no GPU."""
    out = []
    for j, name in enumerate(REPLICA_BUFFERS):
        bad = [r for r in range(1, len(table)) if int(table[r][j]) != int(table[0][j])]
        if bad:
            out.append((name, bad))
    return out


def state_dict_layout(shapes, requires_grad, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, stepped=True):
    """The documented layout of ``FusedAdam.state_dict()`` for parameters of these shapes, as nested plain data: tensors are replaced by
    ``(shape, dtype, device type)``.  Needs no GPU; the host test compares it with torch's Adam on CPU tensors."""
    group = dict(GROUP_DEFAULTS, lr=lr, betas=tuple(betas), eps=eps, params=list(range(len(shapes))))
    state = {}
    if stepped:
        for i, (shape, rg) in enumerate(zip(shapes, requires_grad)):
            if rg:
                state[i] = {"step": ((), torch.float32, "cpu"), "exp_avg": (tuple(shape), torch.float32, None),
                            "exp_avg_sq": (tuple(shape), torch.float32, None)}
    return {"state": state, "param_groups": [group]}


def describe_state_dict(sd):
    """a state dict in the plain form of ``state_dict_layout`` (device type None for the moment buffers: they live where the parameters do)"""
    state = {}
    for i, st in sd["state"].items():
        state[i] = {k: (tuple(t.shape), t.dtype, "cpu" if k == "step" else None) for k, t in st.items()}
        assert st["step"].device.type == "cpu"
    groups = [{k: (tuple(v) if k == "betas" else v) for k, v in g.items()} for g in sd["param_groups"]]
    return {"state": state, "param_groups": groups}


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, network=None):
        """``params``: ``network.parameters()`` (every parameter, in that order) or the network itself; ``network``: the ``NCSNppTime`` whose
        parameters they are -- required, because the flat order and the weight push are the module's."""
        if network is None and isinstance(params, torch.nn.Module):
            network, params = params, params.parameters()
        if network is None or not hasattr(network, "attach_flat"):
            raise ValueError("FusedAdam needs network=<NCSNppTime>: it works on the module's flat parameter buffer")
        params = list(params)
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid hyper-parameters lr={lr} betas={betas} eps={eps}")
        self._lib = _lib.require_gpu()                  # no CPU fallback: raises BuddyHipError here
        ordered = network._params()
        if len(params) != len(ordered) or any(a is not b for a, b in zip(params, ordered)):
            raise ValueError("FusedAdam: params must be network.parameters(), all of them in their order")
        super().__init__(params, dict(GROUP_DEFAULTS, lr=float(lr), betas=tuple(float(b) for b in betas), eps=float(eps)))
        self.network = network
        self._p, self._g = network.attach_flat(with_grad=True)
        self._n = self._p.numel()
        self._m = torch.zeros_like(self._p)
        self._v = torch.zeros_like(self._p)
        self._offsets = list(network._offsets)
        self._buddy_params = ordered
        chunk = int(self._lib.buddy_optim_sqnorm_chunk())
        self._partials = torch.zeros((self._n + chunk - 1) // chunk, dtype=torch.float64, device=self._p.device)
        self._sqnorm = torch.zeros(1, dtype=torch.float64, device=self._p.device)
        self._ema = self._ema_net = None
        # frozen ranges: parameters that do not require grad (torch's Adam never sees them); adjacent ones merge
        fr = []
        for p, (off, n) in zip(ordered, self._offsets):
            if not p.requires_grad:
                if fr and fr[-1][1] == off:
                    fr[-1][1] = off + n
                else:
                    fr.append([off, off + n])
        if len(fr) > 8:
            raise ValueError(f"FusedAdam: {len(fr)} separate frozen parameter ranges (the kernel takes 8)")
        self._frozen_key = tuple(p.requires_grad for p in ordered)
        self._frozen = (C.c_longlong * max(2 * len(fr), 1))(*[x for r in fr for x in r])
        self._n_frozen = len(fr)
        self._group = None              # attach_group: data-parallel replicas
        self._world, self._rank, self._device_coll, self._host = 1, 0, False, None
        self._scale = None              # the factor on the gradient buffer in the last step (None: the unscaled entry ran)

    # ---- data parallelism ---------------------------------------------------------------------------------------------------------
    def attach_group(self, group=None, world=None, rank=None):
        """Make this optimizer one of ``world`` data-parallel replicas.  ``group``: a ``torch.distributed`` process group (None: the default
        group, which must be initialised); ``world`` / ``rank`` default to the group's.  A group of one rank is taken as it is: the
        collectives still run."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise _lib.BuddyHipError("attach_group: torch.distributed is not initialised")
        self._group = group if group is not None else dist.group.WORLD
        self._world = int(world) if world is not None else dist.get_world_size(self._group)
        self._rank = int(rank) if rank is not None else dist.get_rank(self._group)
        if self._world != dist.get_world_size(self._group) or not 0 <= self._rank < self._world:
            raise ValueError(f"attach_group: world {self._world} / rank {self._rank} do not fit the group ({dist.get_world_size(self._group)} ranks)")
        self._device_coll = dist.get_backend(self._group) == "nccl"
        dev = self._p.device
        if not self._device_coll and self._host is None:
            self._host = torch.empty(self._n, dtype=torch.float32, pin_memory=True)     # the one staging buffer of every host-staged collective
        chunk = int(self._lib.buddy_optim_sqnorm_chunk())
        self._ck_partials = torch.zeros((self._n + chunk - 1) // chunk, dtype=torch.int64, device=dev)
        self._ck = torch.zeros(len(REPLICA_BUFFERS), dtype=torch.int64, device=dev)
        return self

    def _need_group(self, what):
        if self._group is None:
            raise _lib.BuddyHipError(f"{what} without attach_group")

    def _all_reduce_sum(self, t):
        """SUM over the ranks into the flat device buffer ``t``, ordered on the current stream: after the kernels already launched on it,
        before those launched next"""
        import torch.distributed as dist
        if self._device_coll:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self._group)     # RCCL waits for the current stream and the stream waits for it
            return
        h = self._host[:t.numel()]
        h.copy_(t, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self._group)
        t.copy_(h, non_blocking=True)           # stream-ordered: the next D2H copy into the pinned buffer queues behind it

    def _broadcast(self, t, src):
        import torch.distributed as dist
        if self._device_coll:
            dist.broadcast(t, src, group=self._group)
            return
        h = self._host[:t.numel()]
        if self._rank == src:
            h.copy_(t, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        dist.broadcast(h, src, group=self._group)
        if self._rank != src:
            t.copy_(h, non_blocking=True)
            torch.cuda.current_stream().synchronize()       # the pinned buffer is reused by the next broadcast at once

    def _small_collective(self, fn, t):
        """a few bytes through ``fn`` (the tensor where the backend wants it); returns the result on the CPU"""
        if self._device_coll:
            return fn(t.to(self._p.device)).cpu()
        return fn(t.cpu())

    @torch.no_grad()
    def broadcast_state(self, src=0, weights_only=False):
        """Every rank takes rank ``src``'s parameters, moments, EMA and per-parameter step counters (``weights_only``: the parameters alone)"""
        import torch.distributed as dist
        self._need_group("broadcast_state")
        self._check_attached(grads=False)
        self._broadcast(self._p, src)
        self.network.params_changed()
        if weights_only:
            return
        self._broadcast(self._m, src)
        self._broadcast(self._v, src)
        if self._ema is not None:
            self._broadcast(self._ema, src)
            self._ema_net.params_changed()
        steps = torch.tensor([float(self.state[p]["step"]) if (p in self.state and len(self.state[p])) else -1.0 for p in self._buddy_params],
                             dtype=torch.float64)

        def bc(t):
            dist.broadcast(t, src, group=self._group)
            return t
        steps = self._small_collective(bc, steps)
        for p, t in zip(self._buddy_params, steps.tolist()):
            if t < 0:
                self.state.pop(p, None)
                continue
            off, n = self._offsets[self._buddy_index[p]]
            self.state[p] = {"step": torch.tensor(t, dtype=torch.float32), "exp_avg": self._m[off:off + n].view(p.shape),
                             "exp_avg_sq": self._v[off:off + n].view(p.shape)}

    def broadcast_int(self, value, src=0):
        """rank ``src``'s integer on every rank (the iteration counter of a resumed run)"""
        import torch.distributed as dist
        self._need_group("broadcast_int")

        def bc(t):
            dist.broadcast(t, src, group=self._group)
            return t
        return int(self._small_collective(bc, torch.tensor([int(value)], dtype=torch.int64))[0])

    def gather_floats(self, t):
        """``t``: (k, b) floats of this rank -> (k, world * b) on the CPU, the ranks' columns in rank order (logging: a few floats per step)"""
        import torch.distributed as dist
        self._need_group("gather_floats")

        def gather(x):
            rows = [torch.empty_like(x) for _ in range(self._world)]
            dist.all_gather(rows, x.contiguous(), group=self._group)
            return torch.cat(rows, dim=1)
        return self._small_collective(gather, t)

    def replica_checksums(self):
        """The checksums of p, m, v and the EMA buffer (0 without one) as a 4-element int64 device tensor; eight launches, no synchronisation"""
        self._need_group("replica_checksums")
        st = _lib.stream_ptr()
        self._ck.zero_()
        for j, buf in enumerate((self._p, self._m, self._v, self._ema)):
            if buf is not None:
                _lib.check(self._lib.buddy_optim_checksum(_lib.ptr(buf), self._n, self._ck_partials.data_ptr(), self._ck.data_ptr() + 8 * j, st))
        return self._ck

    def check_replicas(self):
        """All-gather the 32 bytes of ``replica_checksums`` and raise ``BuddyHipError`` -- on every rank: each sees the same table -- naming the
        buffers on which ranks disagree with rank 0, and those ranks"""
        import torch.distributed as dist
        ck = self.replica_checksums()

        def gather(t):
            rows = [torch.empty_like(t) for _ in range(self._world)]
            dist.all_gather(rows, t, group=self._group)
            return torch.stack(rows)
        table = self._small_collective(gather, ck).tolist()
        bad = replica_disagreements(table)
        if bad:
            raise _lib.BuddyHipError("FusedAdam.check_replicas: the replicas have drifted apart: " +
                                     "; ".join(f"{name} differs from rank 0 on rank(s) {ranks}" for name, ranks in bad))
        return table

    # ---- EMA ----------------------------------------------------------------------------------------------------------------------
    def attach_ema(self, ema_net):
        """``ema_net``: the deep copy of the network that holds the EMA weights.  Its parameters move onto one flat buffer, which
        ``step(ema_s=...)`` and ``ema_update`` write; the copy is told so that its next forward sees the new weights."""
        self._ema = ema_net.attach_flat()
        self._ema_net = ema_net
        if self._ema.numel() != self._n or self._ema.device != self._p.device:
            raise ValueError("attach_ema: the EMA module does not match the network")
        return self._ema

    def ema_update(self, ema_s):
        """the EMA on its own: ema = ema * ema_s + p * (1 - ema_s), one launch"""
        self._check_attached(grads=False)
        if self._ema is None:
            raise _lib.BuddyHipError("ema_update without attach_ema")
        _lib.check(self._lib.buddy_optim_ema(_lib.ptr(self._ema), _lib.ptr(self._p), self._n, float(ema_s), _lib.stream_ptr()))
        self._ema_net.params_changed()

    # ---- the step -----------------------------------------------------------------------------------------------------------------
    def _check_attached(self, grads=True):
        net = self.network
        if net._flat is not self._p or (self._ema is not None and self._ema_net._flat is not self._ema):
            raise _lib.BuddyHipError("FusedAdam: the module's parameters left the flat buffer (.to() / .cuda() after the optimizer was made): "
                                     "build the optimizer after moving the module")
        if tuple(p.requires_grad for p in self._buddy_params) != self._frozen_key:
            raise _lib.BuddyHipError("FusedAdam: requires_grad of a parameter changed after the optimizer was made")
        if not grads:
            return
        if net._grad_flat is not self._g or not net._grad_filled:
            raise _lib.BuddyHipError("FusedAdam.step: no gradient in the flat buffer (call backward through the network after zero_grad)")
        base = self._g.data_ptr()
        for p, (off, n) in zip(self._buddy_params, self._offsets):
            if p.requires_grad and (p.grad is None or p.grad.data_ptr() != base + 4 * off or p.grad.numel() != n or not p.grad.is_contiguous()):
                raise _lib.BuddyHipError(f"FusedAdam.step: the .grad of a parameter of shape {tuple(p.shape)} is not its view of the flat gradient "
                                         "buffer (zero_grad(set_to_none=True) on the module, or a gradient assigned by hand); use the optimizer's "
                                         "zero_grad -- gradients are not gathered silently")

    def zero_grad(self, set_to_none=True):
        """Keeps every ``.grad`` as its view of the flat buffer and tells the network that the next backward overwrites the buffer instead of
        adding to it.  ``set_to_none`` is accepted for signature compatibility only: nothing is ever set to None, because ``step`` needs the views."""
        for p, (off, n) in zip(self._buddy_params, self._offsets):
            if p.requires_grad and p.grad is None:
                p.grad = self._g[off:off + n].view(p.shape)
        self.network.grads_zeroed()

    def _advance_steps(self):
        t = None
        for p in self._buddy_params:
            if not p.requires_grad:
                continue
            st = self.state[p]
            if len(st) == 0:
                off, n = self._offsets[self._buddy_index[p]]
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = self._m[off:off + n].view(p.shape)
                st["exp_avg_sq"] = self._v[off:off + n].view(p.shape)
            st["step"] += 1
            s = float(st["step"])
            if t is not None and s != t:
                raise _lib.BuddyHipError(f"FusedAdam: parameters at different step counts ({t:g} and {s:g}): one fused pass has one bias correction")
            t = s
        return t

    @property
    def _buddy_index(self):
        if not hasattr(self, "_buddy_index_cache"):
            self._buddy_index_cache = {p: i for i, p in enumerate(self._buddy_params)}
        return self._buddy_index_cache

    @torch.no_grad()
    def step(self, closure=None, max_norm=0.0, ema_s=None, grad_scale=None):
        """One optimizer step.  ``max_norm`` > 0: clip the global gradient norm to it first (``clip_grad_norm_``; the gradient buffer itself
        is left unclipped).  ``ema_s``: also update the attached EMA with this factor in the same pass.  ``grad_scale``: the buffer holds a
        SUM of gradients (backward called more than once since ``zero_grad``) and the step, clipping included, uses ``grad_scale`` times it.
        With a group the buffer is first summed over the ranks by one all-reduce and the factor 1 / world is applied on top."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_attached()
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        t = self._advance_steps()
        if t is None:
            return loss
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t                 # Python floats, as torch's single-tensor Adam computes them
        step_size, bc2_sqrt = g["lr"] / bc1, math.sqrt(bc2)
        st = _lib.stream_ptr()
        ema = self._ema if ema_s is not None else None
        if ema_s is not None and ema is None:
            raise _lib.BuddyHipError("step(ema_s=...) without attach_ema")
        if self._group is not None:
            self._all_reduce_sum(self._g)       # the one collective of the step: from here on the buffer holds the sum over the ranks
        if max_norm is not None and max_norm > 0:
            self.grad_sqnorm()
        head = (_lib.ptr(self._p), _lib.ptr(self._g), _lib.ptr(self._m), _lib.ptr(self._v), _lib.ptr(ema), self._n, self._sqnorm.data_ptr(),
                float(max_norm or 0.0), b1, b2, g["eps"], step_size, bc2_sqrt, float(ema_s) if ema_s is not None else 0.0)
        if self._group is not None or grad_scale is not None:
            self._scale = (1.0 if grad_scale is None else float(grad_scale)) / self._world
            _lib.check(self._lib.buddy_optim_step_scaled(*head, self._scale, self._frozen, self._n_frozen, st))
        else:
            self._scale = None
            _lib.check(self._lib.buddy_optim_step(*head, self._frozen, self._n_frozen, st))
        self.network.params_changed()
        if ema is not None:
            self._ema_net.params_changed()
        return loss

    def grad_sqnorm(self):
        """launch the squared global gradient norm; returns the one-element device double (no synchronisation).  Inside a data-parallel step
        it is the squared norm of the SUM over the ranks."""
        _lib.check(self._lib.buddy_optim_sqnorm(_lib.ptr(self._g), self._n, self._partials.data_ptr(), self._sqnorm.data_ptr(), _lib.stream_ptr()))
        return self._sqnorm

    def grad_norm(self):
        """the global gradient norm of the last clipped step as a Python float (synchronises: logging and tests only): of the gradient the
        step used -- with a group the average over the ranks, sqrt(sqnorm) / world"""
        norm = math.sqrt(float(self._sqnorm.item()))
        return norm * self._scale if self._scale is not None else norm

    # ---- checkpoints --------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """Accepts the state dict of torch's Adam (or this class's own): the moments are copied into the flat buffers and every
        ``state[p]`` points at its views again"""
        super().load_state_dict(state_dict)
        with torch.no_grad():
            for p in self._buddy_params:
                st = self.state.get(p)
                if not st:
                    continue
                if not p.requires_grad:
                    raise ValueError("the state dict has optimizer state for a parameter that does not require grad here")
                off, n = self._offsets[self._buddy_index[p]]
                for key, flat in (("exp_avg", self._m), ("exp_avg_sq", self._v)):
                    view = flat[off:off + n].view(p.shape)
                    view.copy_(st[key])
                    st[key] = view
                st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).detach().cpu().reshape(())
