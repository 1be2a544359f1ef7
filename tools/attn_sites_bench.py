"""Attention sites (attn_resolutions): cost per step and the head-width-32 flash kernels.

usage: python tools/attn_sites_bench.py kernels      C = 32 and C = 64 flash kernels (forward, backward; the split count the network picks) at
                                                     T = 8256 and 32768, B = 1: ms per call and achieved TFLOP/s (4 B T^2 C forward, 2.5x that backward)
       python tools/attn_sites_bench.py net          network forward (tape kept) + input-VJP at nf = 128, B = 8, L = 64000 (4 s), image_size 256,
                                                     attn_resolutions (0,) [the shipped config], (32,), (64, 32): ms per step
Run under `rocprofv3 --kernel-trace --stats` for the per-kernel summary (profiles/README.md)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from buddy_amd import _lib  # noqa: E402


def kernels(reps=5):
    lib = _lib.require_gpu()
    P, S = _lib.ptr, _lib.stream_ptr
    for T in (8256, 32768):
        for C in (32, 64):
            B = 1
            q, k, v, dO = (torch.randn(B, T, C, device="cuda") for _ in range(4))
            O = torch.empty_like(q); lse = torch.empty(B, T, device="cuda"); dl = torch.empty(B, T, device="cuda")
            dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
            ns = lib.buddy_flash_attention_splits(B, T)
            ws = torch.empty(max(lib.buddy_flash_attention_workspace(B, T, C, ns), 1), device="cuda")
            sc = C ** -0.5
            f = lambda: _lib.check(lib.buddy_flash_attention_fwd_split(P(q), P(k), P(v), P(O), P(lse), B, T, C, sc, ns, P(ws), S()))  # noqa: E731
            b = lambda: _lib.check(lib.buddy_flash_attention_bwd_split(P(q), P(k), P(v), P(O), P(dO), P(lse), P(dl), P(dq), P(dk), P(dv), B, T, C, sc,  # noqa: E731
                                                                       ns, P(ws), S()))
            fl = 4.0 * B * T * T * C
            out = []
            for fn in (f, b):
                fn(); torch.cuda.synchronize(); t = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize(); out.append((time.perf_counter() - t) / reps)
            print(f"C={C:3d} B={B} T={T} splits={ns}: fwd {out[0] * 1e3:8.3f} ms ({fl / out[0] / 1e12:6.1f} TF/s)   "
                  f"bwd {out[1] * 1e3:8.3f} ms ({2.5 * fl / out[1] / 1e12:6.1f} TF/s)", flush=True)


def net(reps=10, B=8, L=64000):
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.synth import synth_state_dict
    rs = np.random.RandomState(0)
    x = torch.from_numpy((0.3 * rs.standard_normal((B, L))).astype(np.float32)).cuda()
    g = torch.from_numpy(rs.standard_normal((B, L)).astype(np.float32)).cuda()
    scal4 = torch.tensor([[-0.5] * B, [1.0] * B, [0.5] * B, [0.5] * B], dtype=torch.float32).cuda()
    for R in ("[0]", "[32]", "[64,32]"):
        args = compose(overrides=[f"network.attn_resolutions={R}"])
        m = instantiate(args.network)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(5, 128, attn_mask=m.attn_mask).items()})
        m = m.cuda().eval()
        for _ in range(2):
            m.denoise_saved(x, scal4); m.input_vjp(g)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            m.denoise_saved(x, scal4); m.input_vjp(g)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t) / reps * 1e3
        print(f"attn_resolutions={R:8s} mask={m.attn_mask:#06b} B={B} L={L}: forward + input-VJP {ms:8.2f} ms/step", flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    {"kernels": kernels, "net": net}[sys.argv[1] if len(sys.argv) > 1 else "kernels"]()
