"""The general GEMM (1x1 convolutions / NIN layers) at the network's shapes IN ISOLATION: buddy_gemm_bf16x3 against buddy_gemm_f16x2, operands rotated through
enough buffers that no launch finds its A rows in the Infinity Cache.  Prints ms and algorithmic GB/s (A read once + C written once) per shape.
usage: [BUDDY_GEN_ROWS=32|64] python tools/gen_gemm_one.py [out.json]
       [BUDDY_GEN_ROWS=64 | BUDDY_GEN_CP=2] python tools/gen_gemm_one.py --digest
--digest: SHA-256 of what buddy_gemm_f16x2 / buddy_gemm_f16x2_gn_bwd and buddy_gemm_bf16x3 / buddy_gemm_bf16x3_gn_bwd write for seeded inputs at three small
shapes that select the three f16x2 tilings (two-source A, bias, accumulate; two-source x / two-destination dx), to compare two builds bit for bit.  Run it in
fresh processes under the defaults, BUDDY_GEN_ROWS=64 and BUDDY_GEN_CP=2, so that the small M also passes through the large forms."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from buddy_amd import _lib

lib = _lib.require_gpu(); P = _lib.ptr; S = _lib.stream_ptr
SHAPES = [(1048576, 128, 384), (1048576, 128, 256), (262144, 256, 512), (262144, 256, 384), (262144, 256, 256), (262144, 128, 256), (262144, 128, 128),
          (262144, 256, 128), (65536, 256, 512), (65536, 256, 256), (16384, 256, 256)]


def pack(W, arith):
    N, K = W.shape
    if arith == "f16x2":
        W3 = torch.empty(lib.buddy_wgemm_f16x2_packed_bytes(1, N, K) // 4, dtype=torch.int32, device="cuda")
        _lib.check(lib.buddy_wgemm_f16x2_pack_weights(P(W), W3.data_ptr(), 1, N, K, S()))
    else:
        W3 = torch.empty(N * K * 6 // 4, dtype=torch.int32, device="cuda")
        _lib.check(lib.buddy_wgemm_pack_weights(P(W), W3.data_ptr(), 1, N, K, S()))
    return W3


def main():
    out = []
    for M, N, K in SHAPES:
        per = 4 * M * (K + N)
        nbuf = max(2, min(16, int(1.5e9 // per) + 1))
        A = [torch.randn(M, K, device="cuda") for _ in range(nbuf)]
        Cc = [torch.empty(M, N, device="cuda") for _ in range(nbuf)]
        W = torch.randn(N, K, device="cuda") / K ** 0.5
        bias = torch.randn(N, device="cuda")
        row = {"M": M, "N": N, "K": K, "nbuf": nbuf}
        for arith in ("bf16x3", "f16x2"):
            W3 = pack(W, arith)
            gemm = lib.buddy_gemm_f16x2 if arith == "f16x2" else lib.buddy_gemm_bf16x3
            run = lambda i: _lib.check(gemm(P(A[i % nbuf]), K, None, 0, 0, W3.data_ptr(), P(Cc[i % nbuf]), N, M, N, K, P(bias), 1.0, 0, S()))
            for i in range(nbuf):
                run(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 4 * nbuf
            e0.record()
            for i in range(reps):
                run(i)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            row[arith + "_ms"] = ms
            row[arith + "_GBps"] = per / ms / 1e6
        out.append(row)
        print(row, flush=True)
        del A, Cc
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


def digest():
    sha = lambda *ts: hashlib.sha256(b"".join(t.cpu().contiguous().numpy().tobytes() for t in ts)).hexdigest()
    for M, N, B in [(333, 128, 1), (32845, 128, 1), (32847, 256, 3)]:
        K, C0, HW, G = 128, 64, M // B, 32
        g = torch.Generator(device="cpu").manual_seed(1000 * N + M)
        rnd = lambda *shape: torch.randn(*shape, generator=g)
        A = (rnd(M, K) * torch.logspace(-3, 3, M)[:, None]).cuda()                      # rows six decades apart: the running row scale moves
        W, bias, prev = rnd(N, K).cuda(), rnd(N).cuda(), rnd(M, N).cuda()
        A0, A1 = A[:, :C0].contiguous(), A[:, C0:].contiguous()
        x, da, gamma, beta = (rnd(B, HW, N) * 1.5 + 0.3).cuda(), rnd(B, HW, N).cuda(), (1 + 0.2 * rnd(N)).cuda(), (0.2 * rnd(N)).cuda()
        xg = x.double().reshape(B, HW, G, N // G)
        stats = torch.stack([xg.mean(dim=(1, 3)), 1.0 / torch.sqrt(xg.var(dim=(1, 3), unbiased=False) + 1e-6)], dim=-1).float().contiguous()
        X0 = N // 2 if N > 128 else 0                                                   # the x / dx split (a multiple of 128)
        x0, x1 = (x[..., :X0].contiguous(), x[..., X0:].contiguous()) if X0 else (x, None)
        scratch, red = torch.empty(B * 256 * N * 2, dtype=torch.float64, device="cuda"), torch.empty(B, G, 2, device="cuda")
        for arith, gemm, gn_bwd in (("f16x2", lib.buddy_gemm_f16x2, lib.buddy_gemm_f16x2_gn_bwd), ("bf16x3", lib.buddy_gemm_bf16x3, lib.buddy_gemm_bf16x3_gn_bwd)):
            Wp = pack(W, arith)
            Cc = prev.clone()
            _lib.check(gemm(P(A0), C0, P(A1), K - C0, C0, Wp.data_ptr(), P(Cc), N, M, N, K, P(bias), 0.5, 1, S()))
            d0, d1 = torch.zeros_like(x0), (prev.reshape(B, HW, N)[..., X0:].contiguous() if X0 else None)
            _lib.check(gn_bwd(P(A), K, Wp.data_ptr(), P(x0), P(x1) if X0 else None, X0, P(da), P(stats), P(gamma), P(beta), G, 1, 0.70710678,
                              P(d0), P(d1) if X0 else None, 0, 1 if X0 else 0, scratch.data_ptr(), P(red), B, HW, N, K, S()))
            torch.cuda.synchronize()
            print(f"M={M} N={N} K={K} gemm_{arith} {sha(Cc)} gn_bwd {sha(d0, d1) if X0 else sha(d0)}", flush=True)


if __name__ == "__main__":
    digest() if "--digest" in sys.argv[1:] else main()
