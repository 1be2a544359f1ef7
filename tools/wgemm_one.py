"""ONE shape of the Winograd-domain batched GEMM (csrc/wgemm.hip), a few launches (for rocprofv3 --pmc passes and kernel experiments).
usage: python tools/wgemm_one.py Mt N K [positions] [reps] [bf16x3|f16x2] [form]   (f16x2: Mt = 8 utterances x Mt / 8 tiles)
       python tools/wgemm_one.py --table form [out.json]
       python tools/wgemm_one.py --digest bf16x3|f16|form
form (f16x2 only; sets the process defaults before the library reads them): rt2 = one column block per workgroup (BUDDY_WGEMM_CB=1: wgemm_f16x2_rt2_kernel
from 64 tiles per utterance on), cb2 = two column blocks per workgroup wherever Cout >= 256 (BUDDY_WGEMM_CB=2: wgemm_f16x2_kernel<2>), rt1 = the 32-row
one-block kernel (BUDDY_WGEMM_RT=1), rule = the library's own choice.
--table: every distinct shape with Cout >= 256 among the batched GEMMs of one bench.py step (B = 8 x 64 000, nf = 128), 64 positions, each IN ISOLATION:
operands rotated through enough buffers that no launch finds its V rows in the Infinity Cache, HIP-event time per launch.  One form per process; run the
forms alternating.
--digest: SHA-256 of what buddy_gemm_winograd_domain_bf16x3, _f16 or _f16x2 (in the given form) writes for seeded inputs at small shapes that reach every edge
of the store -- 129 and 300 rows (no multiple of 32 or 64), 43 tiles per utterance (the 32-row kernel under the defaults) and 100 (an utterance boundary inside a
wave), Cout 128 / 256 / 384, Cin 64 / 192, 5 positions (one per blockIdx.z) and 8 (folded) -- to compare two builds bit for bit."""
import hashlib, json, os, sys, time
FORMS = {"rt2": {"BUDDY_WGEMM_CB": "1"}, "cb2": {"BUDDY_WGEMM_CB": "2"}, "rt1": {"BUDDY_WGEMM_RT": "1"}, "rule": {}}
table = len(sys.argv) > 1 and sys.argv[1] == "--table"
digest = len(sys.argv) > 2 and sys.argv[1] == "--digest"
form = sys.argv[2] if table or (digest and sys.argv[2] in FORMS) else (sys.argv[7] if len(sys.argv) > 7 else "rule")
os.environ.update(FORMS[form])
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from buddy_amd import _lib
lib = _lib.require_gpu()
P = _lib.ptr; S = _lib.stream_ptr
# (tiles, Cout, Cin, launches per step: forward + data-gradient)
SHAPES = [(29584, 256, 256, 2), (29584, 256, 128, 1), (29584, 384, 128, 1), (7568, 256, 256, 8), (7568, 256, 128, 1), (7568, 256, 384, 1), (7568, 256, 512, 1),
          (7568, 384, 256, 1), (7568, 512, 256, 1), (5624, 1024, 256, 1), (5624, 256, 1024, 1), (1936, 256, 256, 14), (1936, 256, 512, 2), (1936, 512, 256, 2),
          (1520, 1024, 256, 1), (1520, 256, 1024, 1), (528, 256, 256, 20), (528, 256, 512, 2), (528, 512, 256, 2), (400, 1024, 256, 1), (400, 256, 1024, 1)]


def f16x2_setup(A, Bt, Mt, N, K, nb, utts=8):
    U2 = torch.empty(int(lib.buddy_wgemm_f16x2_packed_bytes(nb, N, K)) // 4, dtype=torch.int32, device="cuda")
    _lib.check(lib.buddy_wgemm_f16x2_pack_weights(P(Bt), U2.data_ptr(), nb, N, K, S()))
    vmax = torch.empty(utts, 64, 32, dtype=torch.int32, device="cuda")
    _lib.check(lib.buddy_abs_max_bits(P(A), nb, utts, (Mt // utts) * K, vmax.data_ptr(), S()))
    return U2, vmax


if digest:
    arith = "f16x2" if sys.argv[2] in FORMS else sys.argv[2]
    for utts, tpu, N, K, nb in [(3, 43, 128, 64, 5), (3, 43, 256, 192, 8), (3, 43, 384, 192, 5), (3, 100, 128, 192, 8), (3, 100, 256, 192, 5), (3, 100, 384, 64, 8)]:
        Mt = utts * tpu
        g = torch.Generator(device="cpu").manual_seed(1000 * Mt + N + K + nb)
        level = torch.tensor([1.0, 3e-4, 2e3]).repeat_interleave(tpu)[None, :, None]      # per-utterance (f16x2) and per-tile (f16) scales that differ
        Vh = torch.randn(nb, Mt, K, generator=g) * torch.exp(2.0 * torch.randn(1, Mt, 1, generator=g)) * level
        A, Bt = Vh.cuda(), (torch.randn(nb, N, K, generator=g) * torch.exp(torch.randn(nb, 1, 1, generator=g))).cuda()
        Cm = torch.full((nb, Mt, N), 7.0, device="cuda")
        if arith == "bf16x3":
            U3 = torch.empty(nb * N * K * 6 // 4, dtype=torch.int32, device="cuda")
            _lib.check(lib.buddy_wgemm_pack_weights(P(Bt), U3.data_ptr(), nb, N, K, S()))
            _lib.check(lib.buddy_gemm_winograd_domain_bf16x3(P(A), U3.data_ptr(), P(Cm), Mt, N, K, nb, S()))
        elif arith == "f16":                                      # the operand format of include/buddy_hip.h (buddy_gemm_winograd_domain_f16)
            e = 141 - ((Vh.abs().amax(dim=(0, 2)).view(torch.int32) >> 23) & 0xFF).clamp(15, 253)
            V16 = (Vh.double() * torch.pow(2.0, e.double())[None, :, None]).half().cuda()
            vexp = e.to(torch.int8).cuda()
            U1 = torch.empty(int(lib.buddy_wgemm_f16_packed_bytes(nb, N, K)), dtype=torch.uint8, device="cuda")
            _lib.check(lib.buddy_wgemm_f16_pack_weights(P(Bt), U1.data_ptr(), nb, N, K, S()))
            _lib.check(lib.buddy_gemm_winograd_domain_f16(V16.data_ptr(), vexp.data_ptr(), U1.data_ptr(), P(Cm), Mt, N, K, nb, S()))
        else:
            U2, vmax = f16x2_setup(A, Bt, Mt, N, K, nb, utts)
            _lib.check(lib.buddy_gemm_winograd_domain_f16x2(P(A), U2.data_ptr(), P(Cm), Mt, N, K, nb, vmax.data_ptr(), tpu, S()))
        torch.cuda.synchronize()
        print(f"wgemm {arith} {form if arith == 'f16x2' else '-'} utts={utts} tiles/utt={tpu} Cout={N} Cin={K} P={nb}: "
              f"{hashlib.sha256(Cm.cpu().numpy().tobytes()).hexdigest()}", flush=True)
    sys.exit(0)


if table:
    out = []
    for Mt, N, K, per_step in SHAPES:
        nb, per = 64, 4 * 64 * Mt * (K + N)
        nbuf = max(2, min(16, int(1.5e9 // per) + 1))
        A = [torch.randn(nb, Mt, K, device="cuda") for _ in range(nbuf)]
        Cm = [torch.empty(nb, Mt, N, device="cuda") for _ in range(nbuf)]
        Bt = torch.randn(nb, N, K, device="cuda")
        U2, vmax = f16x2_setup(A[0], Bt, Mt, N, K, nb)       # one abs-max for all buffers: the same distribution
        run = lambda i: _lib.check(lib.buddy_gemm_winograd_domain_f16x2(P(A[i % nbuf]), U2.data_ptr(), P(Cm[i % nbuf]), Mt, N, K, nb, vmax.data_ptr(), Mt // 8, S()))
        for i in range(nbuf):
            run(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = max(4 * nbuf, 8)
        e0.record()
        for i in range(reps):
            run(i)
        e1.record()
        torch.cuda.synchronize()
        row = {"form": form, "tiles": Mt, "Cout": N, "Cin": K, "per_step": per_step, "nbuf": nbuf, "us": 1e3 * e0.elapsed_time(e1) / reps}
        out.append(row)
        print(row, flush=True)
        del A, Cm
    if len(sys.argv) > 3:
        json.dump(out, open(sys.argv[3], "w"), indent=1)
    sys.exit(0)

Mt, N, K = (int(v) for v in sys.argv[1:4]); nb = int(sys.argv[4]) if len(sys.argv) > 4 else 64; reps = int(sys.argv[5]) if len(sys.argv) > 5 else 5
A = torch.randn(nb, Mt, K, device="cuda"); Bt = torch.randn(nb, N, K, device="cuda"); Cm = torch.empty(nb, Mt, N, device="cuda")
U3 = torch.empty(nb * N * K * 6 // 4, dtype=torch.int32, device="cuda")
_lib.check(lib.buddy_wgemm_pack_weights(P(Bt), U3.data_ptr(), nb, N, K, S()))
mode = sys.argv[6] if len(sys.argv) > 6 else "bf16x3"
f = lambda: _lib.check(lib.buddy_gemm_winograd_domain_bf16x3(P(A), U3.data_ptr(), P(Cm), Mt, N, K, nb, S()))
if mode == "f16x2":
    U2, vmax = f16x2_setup(A, Bt, Mt, N, K, nb)
    f = lambda: _lib.check(lib.buddy_gemm_winograd_domain_f16x2(P(A), U2.data_ptr(), P(Cm), Mt, N, K, nb, vmax.data_ptr(), Mt // 8, S()))
f(); f(); torch.cuda.synchronize(); t = time.perf_counter()
for _ in range(reps): f()
torch.cuda.synchronize(); dt = (time.perf_counter() - t) / reps
print(f"wgemm {mode} {form} P={nb} Mt={Mt} N={N} K={K}: {dt*1e3:.3f} ms {2.0*nb*Mt*N*K/dt/1e12:.1f} TF-eq {(6.0 if mode == 'f16x2' else 12.0)*nb*Mt*N*K/dt/1e12:.0f} TF executed "
      f"{(Mt*K+Mt*N)*nb*4/dt/1e9:.0f} GB/s", flush=True)
