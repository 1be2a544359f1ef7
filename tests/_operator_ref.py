"""The float64 arbiter of the blind operator tests (helper: no tests in it).

A thin layer over the torch restatement (``oracle.batched.operators.BlindSubbandFiltering``, ``oracle.batched.losses.get_loss``,
``oracle.batched.sampler.EulerHeunSamplerDPSTorch.optimize_op``) run on the CPU under ``oracle.precision.fp64()``: it injects the parameters
(decay, weights, phases) it is given -- the HIP handle's own, so both sides start from the same numbers --, runs the restatement and hands
every quantity back as a float64 numpy array.  It is NOT a new restatement of the algorithm.  ``fp64=False`` runs the very same calls with
the default dtype left at float32: the fp32 restatement whose error against the arbiter the tolerances are set against.

Used by tests/test_operator_ref_host.py (CPU: the arbiter against itself, against its fp32 form and against the reference fixtures) and by
tests/test_hip_operator_shapes.py (GPU: the HIP operator against the arbiter)."""
from __future__ import annotations

import contextlib
import functools
import json
import os
import time

import numpy as np
import torch

SR = 16000
OVERRIDES = ["tester.posterior_sampling.warm_initialization.mode=reverb_scaled"]

# id -> (U, L); T = 1 + (L + 512) // 128 frames.  What each one reaches in csrc/operator.hip:
SHAPES = {
    "sub_hop": (3, 100),             # T = 5: L < hop, one partial FIR tile / gradh chunk, T < 100 taps, U*T % 4 = 3, losses with fewer elements than threads
    "tile_exact": (2, 7552),         # T = 64: exactly one FIR tile / gradh chunk
    "tile_plus_one": (2, 7680),      # T = 65: the second tile / chunk holds one frame
    "odd": (5, 8001),                # T = 67: odd L, odd U*T, the last frame straddles the end
    "same_as_rir": (2, 13824),       # T = 113 = Td, L == Lr
    "longer_than_rir": (1, 20000),   # T = 161: L > Lr, U = 1
    "grid_cap": (8, 65536),          # T = 517: U*T*513 > 8192*256, the second grid-stride trip of every gridf kernel
}

# what tests/test_hip_operator_golden.py holds the HIP operator to at the fixture shape, per quantity class
GOLDEN_BOUND = {"design": 1e-5, "stft": 1e-5, "filter": 1e-4, "loss": 1e-4, "grad": 2e-3, "loop": 2e-3}
_FORWARD_CLASS = {"A": "design", "stft_x": "stft", "stft_rir": "stft", "H": "filter", "deg": "filter", "rir": "filter"}


def klass(name):
    """quantity name -> its row of GOLDEN_BOUND: everything after optimize_op is "loop" (2e-3 through iteration 3), loss values are "loss",
    every gradient / vjp is "grad", the forward pieces have their own rows"""
    if name.startswith("loop_"):
        return "loop"
    last = name.split(".")[-1]
    if last in _FORWARD_CLASS:
        return _FORWARD_CLASS[last]
    if last == "value" or last.startswith("l_") or last.startswith("only_l_"):
        return "loss"
    return "grad"


# The fp32 CPU restatement's own error against the float64 arbiter (fraction of abs-max) per (shape, quantity), recorded by running this file
# (``python tests/_operator_ref.py``, 8 threads) and checked again by tests/test_operator_ref_host.py.
FP32_ERR_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "operator_shapes_fp32_err.json")


@functools.lru_cache(maxsize=None)
def fp32_err():
    with open(FP32_ERR_FILE) as f:
        return json.load(f)


def rel(a, b):
    """max |a - b| / max |b| with b the reference (complex arrays as complex numbers, never as angles)"""
    a, b = to_np(a), to_np(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def to_np(t):
    if torch.is_tensor(t):
        t = t.detach().cpu()
        return t.to(torch.complex128 if t.is_complex() else torch.float64).numpy().copy()       # never a view of a live parameter
    return np.asarray(t)


def bound(shape_id, name):
    """the larger of the golden-test bound of the quantity's class and four times the fp32 restatement's own recorded error"""
    return max(GOLDEN_BOUND[klass(name)], 4.0 * fp32_err()["errors"][shape_id][name])


def config(n_iters=3):
    from buddy_amd.config import compose
    args = compose(overrides=list(OVERRIDES))
    args.tester.posterior_sampling.blind_hp.op_updates_per_step = n_iters
    return args


def loss_block(name, fw=None, weight=1.0, c=0.667):
    from buddy_amd.config import AttrDict
    la = AttrDict(name=name, weight=weight)
    if "comp" in name:
        la["compression_factor"] = c
    if fw is not None:
        la["freq_weighting"] = fw
    return la


@functools.lru_cache(maxsize=None)
def signals(U, L):
    """float32 (x, y, x_den, w), rows differ: x = synth_clean(u), y = x * a synthetic RIR no longer than half the signal, x_den the mixture the
    existing likelihood tests use, w a seeded cotangent"""
    from buddy_amd.synth import synth_clean, synth_rir
    x = np.stack([synth_clean(u, L) for u in range(U)])
    taps = min(1500, max(8, L // 2))
    y = np.stack([np.convolve(x[u].astype(np.float64), synth_rir(u, taps).astype(np.float64))[:L] for u in range(U)]).astype(np.float32)
    xd = (0.9 * x + 0.01 * x[:, ::-1]).astype(np.float32)
    w = np.random.RandomState(77).standard_normal((U, L)).astype(np.float32)
    return x, y, xd, w


def cotangent(seed, shape):
    return np.random.RandomState(seed).standard_normal(tuple(shape)).astype(np.float32)


class Arbiter:
    """The restatement with injected parameters.  ``noise``: one ``oracle.sampler_ref.NoiseStream`` per row (the constructor takes two draws
    from each, like every BlindSubbandFiltering; the regulariser one per iteration).  ``decay`` / ``weights`` / ``phases``: float arrays in the
    reference layouts (U, E, bands) / (U, 513, Nf), copied in before H is built from them; all None: the operator as constructed, then
    ``update_H(use_noise=True)`` like the reference fixtures."""

    def __init__(self, args, U, noise, decay=None, weights=None, phases=None, fp64=True):
        from oracle.batched.operators import BlindSubbandFiltering
        self.args, self.U, self.fp64, self.noise = args, int(U), bool(fp64), noise
        self.ps = args.tester.posterior_sampling
        with self._mode():
            self.op = BlindSubbandFiltering(args.tester.informed_dereverberation.op_hp, SR, num_utts=U, noise=noise, device="cpu")
            for p in self.op.params + self.op.params_phases:
                p.requires_grad = False
            if decay is None:
                self.op.update_H(use_noise=True)
            else:
                with torch.no_grad():
                    self.op.params[0].copy_(self._t(decay))
                    self.op.params[1].copy_(self._t(weights))
                self.op.params_phases[0] = self._t(phases).clone()
                self.op.update_H()
        self.Lr = self.op.length_rir + 1024

    def _mode(self):
        from oracle import precision
        return precision.fp64() if self.fp64 else contextlib.nullcontext()

    @staticmethod
    def _t(a):
        a = a.detach().cpu() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return a.to(torch.complex128 if a.is_complex() and torch.get_default_dtype() == torch.float64 else
                    (torch.complex64 if a.is_complex() else torch.get_default_dtype()))

    def _settle(self):
        """after a pass that differentiated the parameters: H again the detached filter of the current parameters"""
        for p in self.op.params + self.op.params_phases:
            p.requires_grad = False
            p.grad = None
        self.op.update_H()

    # ---- (a) forward pieces
    def forward(self, x):
        with self._mode(), torch.no_grad():
            op, xx = self.op, self._t(x)
            r = op.get_time_RIR().reshape(self.U, -1)
            return {"A": to_np(op.design_filter()), "H": to_np(op.H), "stft_x": to_np(op.apply_stft(xx)), "stft_rir": to_np(op.apply_stft(r)),
                    "deg": to_np(op.degradation(xx)), "rir": to_np(r)}

    # ---- (b) adjoints: autograd of the pieces with H (complex) and the signals as leaves.  A complex leaf's .grad is dL/dRe + j dL/dIm.
    def adjoints(self, x, w_deg, w_rir, W_x, W_rir):
        """cotangents: w_deg (U, L), w_rir (U, Lr) real; W_x (U, 513, T, 2), W_rir (U, 513, Td, 2) real views"""
        with self._mode():
            op = self.op
            H = op.H.detach().clone().requires_grad_(True)
            xx = self._t(x).requires_grad_(True)
            gx, gH = torch.autograd.grad((op.degradation(xx, H=H) * self._t(w_deg)).sum(), (xx, H))
            if w_rir is None:
                return {"vjp_x": to_np(gx)}
            H2 = op.H.detach().clone().requires_grad_(True)
            gH2, = torch.autograd.grad((op.get_time_RIR(H=H2).reshape(self.U, -1) * self._t(w_rir)).sum(), H2)
            out = {"vjp_x": to_np(gx), "vjp_H": to_np(gH), "vjp_rir_H": to_np(gH2)}
            rir = op.get_time_RIR().detach().reshape(self.U, -1)
            for key, sig, W in (("adj_stft_x", self._t(x), W_x), ("adj_stft_rir", rir, W_rir)):
                s = sig.clone().requires_grad_(True)
                g, = torch.autograd.grad((torch.view_as_real(op.apply_stft(s)) * self._t(W)).sum(), s)
                out[key] = to_np(g)
            return out

    # ---- (c) likelihood and parameter gradients
    def likelihood(self, x_den, y, block=None):
        from oracle.batched.losses import get_loss
        with self._mode():
            xd = self._t(x_den).requires_grad_(True)
            v = get_loss(block if block is not None else self.ps.rec_loss, self.op)(self._t(y), self.op.degradation(xd), per_utt=True)
            g, = torch.autograd.grad(v.sum(), xd)
            return {"l_lik": to_np(v), "g_x": to_np(g)}

    def param_grads(self, x_den, y, noise=None, t_op=0.0):
        """one gradient evaluation of optimize_op's objective; ``noise`` (U, Lr) = the regulariser's draw, None = the reconstruction term alone"""
        from oracle.batched.losses import get_loss
        with self._mode():
            op = self.op
            prm = op.params + op.params_phases
            for p in prm:
                p.requires_grad = True
            op.update_H()
            l1 = get_loss(self.ps.rec_loss_params, op)(self._t(y), op.degradation(self._t(x_den)), per_utt=True)
            tot, out = l1.sum(), {"l_rec": to_np(l1)}
            if noise is not None:
                rt = op.get_time_RIR().reshape(self.U, -1)
                l2 = get_loss(self.ps.RIR_noise_regularization.loss, op)(rt, (rt + float(t_op) * self._t(noise)).detach(), per_utt=True)
                tot, out["l_reg"] = tot + l2.sum(), to_np(l2)
            gs = torch.autograd.grad(tot, prm)
            out.update(g_decay=to_np(gs[0]), g_weights=to_np(gs[1]), g_phases=to_np(gs[2]))
            self._settle()
            return out

    # ---- (d) the callable loss: per-utterance values and the gradient w.r.t. both arguments
    def loss(self, block, a, b):
        from oracle.batched.losses import get_loss
        with self._mode():
            aa, bb = self._t(a).requires_grad_(True), self._t(b).requires_grad_(True)
            v = get_loss(block, self.op)(aa, bb, per_utt=True)
            ga, gb = torch.autograd.grad(v.sum(), (aa, bb))
            return {"value": to_np(v), "g_a": to_np(ga), "g_b": to_np(gb)}

    # ---- (e) optimize_op: the restatement's own loop (torch's Adam), then what the parameters produce
    def optimize(self, x_den, y, t):
        from buddy_amd.instantiate import instantiate
        from oracle.batched.sampler import EulerHeunSamplerDPSTorch
        with self._mode():
            op = self.op
            start = [p.detach().clone() for p in op.params + op.params_phases]
            smp = EulerHeunSamplerDPSTorch(torch.nn.Identity(), instantiate(self.args.diff_params), self.args)
            smp.bind(self._t(y), op, True)
            smp.optimize_op(self._t(x_den), torch.tensor(float(t)))
            st = smp.optimizer_operator.state
            out = {}
            for nm, p in (("decay", op.params[0]), ("weights", op.params[1]), ("phases", op.params_phases[0])):
                out["m_" + nm], out["v_" + nm] = to_np(st[p]["exp_avg"]), to_np(st[p]["exp_avg_sq"])
                out[nm] = to_np(p)
            with torch.no_grad():
                self._settle()                               # the final update_H: H of the parameters AFTER the last step
                out["A"] = to_np(op.design_filter())
                out["H"], out["rir"] = to_np(op.H), to_np(op.get_time_RIR().reshape(self.U, -1))
                for p, s in zip(op.params, start[:2]):       # the other answers are those of the injected parameters
                    p.copy_(s)
                op.params_phases[0] = start[2]
                self._settle()
            return out


SEED, T_OP, LR_LEN, TD = 40, 0.004, 13824, 113


def streams(U, k=2):
    """row u's noise stream, ``k`` draws in (every BlindSubbandFiltering constructor takes two: the phases, then update_H's noise)"""
    from oracle.sampler_ref import NoiseStream
    ns = [NoiseStream(SEED + u) for u in range(U)]
    for n in ns:
        n.k = k
    return ns


def reg_noise(U):
    """the regulariser's draw of a fresh operator: draw 2 of every row's stream, float32 (U, Lr)"""
    return np.stack([n.randn((LR_LEN,)).float().numpy() for n in streams(U)])


def initial_params(args, U):
    """float32 (decay, weights, phases) of a freshly constructed fp32 restatement with the rows' noise streams: what the CPU tests inject where the
    GPU tests inject the HIP handle's own"""
    from oracle.batched.operators import BlindSubbandFiltering
    op = BlindSubbandFiltering(args.tester.informed_dereverberation.op_hp, SR, num_utts=U, noise=streams(U, 0), device="cpu")
    return tuple(p.detach().float().numpy().copy() for p in (op.params[0], op.params[1], op.params_phases[0]))


class Case:
    """One shape of the table with its inputs and the arbiter's answers, each computed once and kept (the tests of a shape share them)."""

    def __init__(self, shape_id, decay, weights, phases, fp64=True):
        self.id = shape_id
        self.U, self.L = SHAPES[shape_id]
        self.T = 1 + (self.L + 512) // 128
        self.x, self.y, self.xd, self.w = signals(self.U, self.L)
        self.w_rir = cotangent(78, (self.U, LR_LEN))
        self.W_x = cotangent(79, (self.U, 513, self.T, 2))
        self.W_rir = cotangent(80, (self.U, 513, TD, 2))
        self.noise = reg_noise(self.U)
        self.params = (np.asarray(decay, np.float32), np.asarray(weights, np.float32), np.asarray(phases, np.float32))
        self.args = config(3)
        self.arb = Arbiter(self.args, self.U, streams(self.U), *self.params, fp64=fp64)
        self.seconds = {}
        self._memo = {}

    def _once(self, key, fn):
        if key not in self._memo:
            self._memo[key], self.seconds[key] = timed(fn)
        return self._memo[key]

    def forward(self):
        return self._once("forward", lambda: self.arb.forward(self.x))

    def adjoints(self):
        return self._once("adjoints", lambda: self.arb.adjoints(self.x, self.w, self.w_rir, self.W_x, self.W_rir))

    def likelihood(self):
        return self._once("likelihood", lambda: self.arb.likelihood(self.xd, self.y))

    def param_grads(self, with_noise=True):
        return self._once("param_grads" if with_noise else "param_grads_only",
                          lambda: self.arb.param_grads(self.xd, self.y, self.noise if with_noise else None, T_OP))

    def loss(self, block):
        return self._once(("loss", block.name, block.get("freq_weighting", None)), lambda: self.arb.loss(block, 0.8 * self.x, 0.9 * self.y))

    def loop(self):
        """three iterations of optimize_op from the injected parameters; the arbiter puts the parameters back afterwards"""
        def run():
            for n in self.arb.noise:
                n.k = 2
            out = self.arb.optimize(self.xd, self.y, T_LOOP)
            flat = {"loop_" + k: v for k, v in out.items() if k != "phases"}
            flat["loop_Aejphi"] = a_ejphi(out["A"], out["phases"])
            return flat
        return self._once("loop", run)

    def section(self, name):
        """the arbiter's answers of one section of the table as a flat {quantity name: float64 array}"""
        if name == "forward":
            return self.forward()
        if name == "adjoints":
            return self.adjoints()
        if name == "vjp_x":
            return self._once("vjp_x", lambda: self.arb.adjoints(self.x, self.w, None, None, None))
        if name == "likelihood":
            return self.likelihood()
        if name == "param_grads":
            return self.param_grads(True)
        if name == "param_grads_only":
            return {"only_" + k: v for k, v in self.param_grads(False).items()}
        if name == "loss":
            out = {}
            for nm, fw in LOSS_EDGE_BLOCKS:
                out.update({f"loss.{nm}.{fw}.{k}": v for k, v in self.loss(loss_block(nm, fw, LOSS_WEIGHT)).items()})
            return out
        if name == "loop":
            return self.loop()
        raise KeyError(name)


T_LOOP, LOSS_WEIGHT = 0.02, 3.0
LOSS_EDGE_BLOCKS = (("l2_comp_stft_summean", None), ("l2_stft_sum", "sqrt"), ("l2_mean", None))
LOSS_SHAPES, LOOP_SHAPES, ROW_SHAPES = ("sub_hop", "tile_plus_one"), ("sub_hop", "odd", "same_as_rir"), ("sub_hop", "odd")


def sections(shape_id):
    """which sections a shape runs: grid_cap is there for the second grid-stride trip, not for the loop"""
    if shape_id == "grid_cap":
        return ("forward", "vjp_x", "likelihood")
    s = ["forward", "adjoints", "likelihood", "param_grads", "param_grads_only"]
    if shape_id in LOSS_SHAPES:
        s.append("loss")
    if shape_id in LOOP_SHAPES:
        s.append("loop")
    return tuple(s)


def errors(case, other):
    """every quantity of every section of the shape: error of ``other`` (a Case of the same shape) against ``case``"""
    out = {}
    for sec in sections(case.id):
        ref, got = case.section(sec), other.section(sec)
        out.update({k: rel(got[k], ref[k]) for k in ref})
    return out


def a_ejphi(A, phases):
    """what the phases produce: A e^{j phi} (phases of bins at the magnitude floor are round-off on any implementation)"""
    return to_np(A) * np.exp(1j * to_np(phases))


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    out = fn(*a, **k)
    return out, time.perf_counter() - t0


@functools.lru_cache(maxsize=None)
def host_pair(shape_id):
    """(float64 arbiter, fp32 restatement) of a shape on the parameters of a freshly constructed fp32 restatement"""
    U, _ = SHAPES[shape_id]
    prm = initial_params(config(3), U)
    return Case(shape_id, *prm, fp64=True), Case(shape_id, *prm, fp64=False)


if __name__ == "__main__":       # record the fp32 restatement's own error and the arbiter's CPU time per shape
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.set_num_threads(8)
    rec = {"errors": {}, "arbiter_seconds": {}}
    for sid in SHAPES:
        c64, c32 = host_pair(sid)
        rec["errors"][sid] = {k: float(f"{v:.3e}") for k, v in errors(c64, c32).items()}
        rec["arbiter_seconds"][sid] = round(sum(c64.seconds.values()), 2)
        print(sid, rec["arbiter_seconds"][sid], "s", max(rec["errors"][sid].items(), key=lambda kv: kv[1] / GOLDEN_BOUND[klass(kv[0])]))
    with open(FP32_ERR_FILE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
