"""Concurrent sub-batches: one batch of utterances sampled as S independent sub-batches on S HIP streams, stepped in lock-step from one host
thread.  Per-utterance semantics make the result identical to the single-batch run (rows never interact); the gain is occupancy -- the
latency-bound pieces of one sub-batch's step (operator optimisation: ~75 small launches per Adam iteration, bottleneck-resolution layers, the
sampler's elementwise tail) run beside the large kernels of the other.  Measured: B = 8 as 2 x 4 on one MI355X 110.0 -> 103.8 ms per step.
New capability (the reference samples one utterance at a time, testing/tester.py:153); each sub-batch owns a network handle (activation arena +
VJP tape live inside it), a sampler and an operator."""
from __future__ import annotations

import torch

from ..instantiate import instantiate


class SubBatch:
    def __init__(self, sampler, y, operator, blind, stream):
        self.s, self.y, self.op, self.blind, self.stream = sampler, y, operator, blind, stream
        self.x = self.x_den = None

    def begin(self):
        """what predict_conditional does before its loop (testing/EulerHeunSamplerDPS.py predict_conditional + predict)"""
        s = self.s
        with torch.cuda.stream(self.stream):
            s.bind(self.y, self.op, self.blind)
            t = s.create_schedule()
            self.t, self.g = t.tolist(), s.get_gamma(t).tolist()
            self.x = s.initialize_x(tuple(self.y.shape), self.y.device, t)

    def step(self, i):
        with torch.cuda.stream(self.stream):
            self.s.step_counter = i
            self.x, self.x_den = self.s.step(self.x, self.t[i], self.t[i + 1], self.g[i], self.blind)


def split_rows(n, parts):
    """contiguous row ranges of near-equal size"""
    parts = max(1, min(parts, n))
    base, extra = divmod(n, parts)
    out, lo = [], 0
    for p in range(parts):
        hi = lo + base + (1 if p < extra else 0)
        out.append((lo, hi)); lo = hi
    return out


def split_groups(groups, parts):
    """``split_rows`` for tied operator rows: at most ``parts`` contiguous row ranges whose boundaries fall on group boundaries (a group lives inside
    one operator), as even as those allow: every cut is the group boundary nearest to the even cut.  One group gives one part."""
    n = len(groups)
    starts = [b for b in range(1, n) if groups[b] != groups[b - 1]]
    parts = max(1, min(int(parts), len(starts) + 1))
    cuts = []
    for p in range(1, parts):
        lo = cuts[-1] if cuts else 0
        cand = [b for b in starts if b > lo]
        if not cand:
            break
        cuts.append(min(cand, key=lambda b: (abs(b - p * n / parts), b)))
    edges = [0] + cuts + [n]
    return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]


class ConcurrentSampler:
    """S samplers (own network replica each) + S streams, created once and reused for every batch."""

    def __init__(self, args, network, diff_params, sub_batches):
        self.args, self.S = args, int(sub_batches)
        nets = [network] + [network.replica() for _ in range(self.S - 1)]
        self.samplers = [instantiate(args.tester.sampler, n, diff_params, args) for n in nets]
        self.streams = [torch.cuda.Stream() for _ in range(self.S)]

    def predict_conditional(self, ys, operators, blind, noises=None):
        """ys / operators: one (rows, L) tensor and one operator per sub-batch -> list of (rows, L) estimates (x_den of the last step)"""
        cur = torch.cuda.current_stream()
        subs = []
        for k, (y, op) in enumerate(zip(ys, operators)):
            self.samplers[k].noise = None if noises is None else noises[k]
            self.streams[k].wait_stream(cur)
            subs.append(SubBatch(self.samplers[k], y, op, blind, self.streams[k]))
        for sb in subs:
            sb.begin()
        T = subs[0].s.T
        for i in range(T):
            for sb in subs:
                sb.step(i)
        for sb in subs:
            cur.wait_stream(sb.stream)
        self.last = subs
        return [sb.x_den.detach() for sb in subs]
