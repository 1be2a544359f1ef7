"""GPU: SRMR (csrc/srmr.hip, buddy_amd/utils/srmr.py) against the float64 restatement tests/_srmr_ref.py: each C entry alone on ragged rows with NaN
behind every row and guard words behind every output, the whole call at 16, 48 and 8 kHz, the tester writing its CSV files in the real-recordings mode
and in a paired mode, and the stand-alone tool reading them back."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _srmr_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_clean, synth_rir  # noqa: E402
from buddy_amd.utils import srmr as S  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 12345.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24
J, K = 23, 8


@pytest.fixture(scope="module")
def lib():
    return _lib.require_gpu()


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def padded(rows, ld, fill=np.nan):
    """rows of their own lengths -> (B, ld) float32 on the device with ``fill`` behind every row (NaN: a read past the end would show)"""
    out = np.full((len(rows), ld), fill, np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return torch.from_numpy(out).cuda()


def guarded(n, dtype, fill):
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


def split(buf, n, fill):
    """the first n words; asserts the guard words behind them are intact"""
    a = buf.cpu().numpy()
    assert np.all(a[n:] == fill), "guard words overwritten"
    return a[:n]


# ---- 1. the envelope -------------------------------------------------------------------------------------------------------------------------
def device_bank():
    """the bank as the library takes it, the channels in the order of ``gammatone_bank()`` (highest first)"""
    t32 = R.taps32()
    off = np.concatenate([[0], np.cumsum([len(r) for r, _ in t32])]).astype(np.int32)
    g_re = torch.from_numpy(np.concatenate([r for r, _ in t32])).cuda()
    g_im = torch.from_numpy(np.concatenate([i for _, i in t32])).cuda()
    return g_re, g_im, (_lib.C.c_int * len(off))(*off.tolist())


def run_envelope(lib, rows, lde_extra=3):
    """env (B, 23, lde) of ragged rows, downloaded; every word at or behind lens[b] still holds the sentinel"""
    B, lens = len(rows), [len(r) for r in rows]
    ld, lde = max(lens) + 5, max(lens) + lde_extra
    x_d, lens_d = padded(rows, ld), dev_i32(lens)
    g_re, g_im, off = device_bank()
    env = guarded(B * J * lde, torch.float32, SENTINEL)
    rc = lib.buddy_gammatone_env(_lib.ptr(x_d), lens_d.data_ptr(), B, ld, _lib.ptr(g_re), _lib.ptr(g_im), off, J, _lib.ptr(env), lde, _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    got = split(env, B * J * lde, SENTINEL).reshape(B, J, lde)
    for b, n in enumerate(lens):
        assert np.all(got[b, :, n:] == SENTINEL), b                                      # nothing written at or behind the row's end
    return got


def test_envelope_of_unit_impulses(lib):
    """an impulse at sample n0 reads the taps out one by one: env[n] = |g_j[n - n0]| from the fp32 taps within 2 ulp (one product per component is
    exact; the squares, their sum and the root round), for every channel and every tap including the last, and exactly zero before the impulse and
    behind the last tap.  Impulses at sample 0, across a tile edge, and at the row's last sample"""
    T = lib.buddy_srmr_tile()
    L = 2 * T + 353
    at = [0, T - 77, L - 1]
    rows = [np.zeros(L, np.float32) for _ in at]
    for r, n0 in zip(rows, at):
        r[n0] = 1.0
    got = run_envelope(lib, rows, lde_extra=0)                                           # L is odd: the scalar stores
    got4 = run_envelope(lib, rows, lde_extra=3)                                          # lde = L + 3 is a multiple of 4: the 16-byte stores
    assert (L + 3) % 4 == 0 and np.array_equal(got[:, :, :L].view(np.uint32), got4[:, :, :L].view(np.uint32))
    worst = 0.0
    for b, n0 in enumerate(at):
        for j, (gr, gi) in enumerate(R.taps32()):
            want = np.zeros(L)
            n = min(len(gr), L - n0)
            assert n == len(gr) or b == 2
            want[n0:n0 + n] = np.sqrt(gr[:n].astype(np.float64) ** 2 + gi[:n].astype(np.float64) ** 2)
            err = np.abs(got[b, j, :L].astype(np.float64) - want)
            assert np.all(err[want == 0.0] == 0.0), (b, j)
            ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
            worst = max(worst, float((err / ulp).max()))
            assert np.all(err <= 2.0 * ulp), (b, j, float((err / ulp).max()))
    print(f"envelope of impulses: worst error {worst:.3f} ulp")


def test_envelope_ragged_vs_restatement(lib):
    """rows of 1, 56, 57, 58 (the shortest channel's taps and its neighbours), 1145, 1146, 1147 (the longest's) and tile - 1, tile, tile + 1,
    2 tile + 1 samples, three to a batch.  Every sample within (N_j + 4) 2^-24 sum_t |g_j[t]| max|x_b| of the float64 restatement: the worst case of
    an fp32 sum of N_j products (N_j u), the rounding of the taps (u) and of the magnitude (2 u).  A row alone equals the row in its batch bit for bit"""
    T = lib.buddy_srmr_tile()
    lens = [1, 56, 57, 58, 1145, 1146, 1147, T - 1, T, T + 1, 2 * T + 1]
    assert min(len(g) for g in R.taps()) == 57 and max(len(g) for g in R.taps()) == 1146
    rows = [R.speechlike(u, max(L, 64))[:L].astype(np.float32) for u, L in enumerate(lens)]
    rows[0][0] = 0.25
    sums = np.array([np.abs(g).sum() for g in R.taps()])
    N = np.array([len(g) for g in R.taps()])
    worst = 0.0
    got = {}
    for s in range(0, len(rows), 3):
        part = rows[s:s + 3]
        env = run_envelope(lib, part)
        for b, r in enumerate(part):
            want = R.envelope(r.astype(np.float64))
            tol = (N + 4) * U24 * sums * float(np.abs(r).max())
            err = np.abs(env[b, :, :len(r)].astype(np.float64) - want)
            worst = max(worst, float((err / tol[:, None]).max()))
            assert np.all(err <= tol[:, None]), (len(r), float((err / tol[:, None]).max()))
            got[len(r)] = env[b, :, :len(r)]
    print(f"envelope, ragged rows: worst error / bound {worst:.4f}")
    for L in (58, 2 * T + 1):
        alone = run_envelope(lib, [rows[lens.index(L)]], lde_extra=8)
        assert np.array_equal(alone[0, :, :L].view(np.uint32), got[L].view(np.uint32)), L


def test_entries_refuse_bad_arguments(lib):
    """BUDDY_ERR_ARG with nothing launched (the outputs keep their sentinel)"""
    st = _lib.stream_ptr()
    x, lens = padded([np.ones(5000, np.float32)], 5000), dev_i32([5000])
    g_re, g_im, off = device_bank()
    env = guarded(J * 5000, torch.float32, SENTINEL)
    args = lambda **kw: [kw.get("x", _lib.ptr(x)), lens.data_ptr(), kw.get("B", 1), kw.get("ld", 5000), _lib.ptr(g_re), _lib.ptr(g_im), kw.get("off", off),
                         kw.get("J", J), _lib.ptr(env), kw.get("lde", 5000), st]
    long_off = (_lib.C.c_int * 2)(0, 1537)
    for kw in (dict(x=None), dict(B=0), dict(ld=4999), dict(lde=4999), dict(J=0), dict(J=33), dict(off=long_off, J=1)):
        assert lib.buddy_gammatone_env(*args(**kw)) == 2, kw
    coef = (_lib.C.c_double * 48)(*S.modulation_bank().coef.reshape(-1).tolist())
    bad_coef = (_lib.C.c_double * 48)(*(2.0 * S.modulation_bank().coef).reshape(-1).tolist())
    E, fr = guarded(J * K, torch.float64, SENTINEL), guarded(1, torch.int32, -77)
    margs = lambda **kw: [_lib.ptr(env), lens.data_ptr(), 1, J, kw.get("lde", 5000), kw.get("coef", coef), kw.get("K", K), kw.get("W", 4096), kw.get("H", 1024),
                          E.data_ptr(), kw.get("ldm", 1), fr.data_ptr(), st]
    for kw in (dict(lde=4999), dict(coef=bad_coef), dict(K=9), dict(K=0), dict(W=4095), dict(W=2048, H=512, ldm=1), dict(H=1000, W=4000), dict(W=8192, H=2048),
               dict(ldm=0)):
        assert lib.buddy_modulation_energies(*margs(**kw)) == 2, kw
    out, eb, fl = guarded(3, torch.float64, SENTINEL), guarded(J * K, torch.float64, SENTINEL), guarded(1, torch.int32, -77)
    frames = dev_i32([1])
    erbs, low = (_lib.C.c_double * J)(*([50.0] * J)), (_lib.C.c_double * K)(*([10.0] * K))
    for kw in (dict(K=7), dict(J=0), dict(ldm=0)):
        rc = lib.buddy_srmr_scores(E.data_ptr(), frames.data_ptr(), 1, kw.get("J", J), kw.get("K", K), kw.get("ldm", 1), erbs, low, out.data_ptr(), eb.data_ptr(),
                                   fl.data_ptr(), st)
        assert rc == 2, kw
    torch.cuda.synchronize()
    split(env, J * 5000, SENTINEL), split(E, J * K, SENTINEL), split(fr, 1, -77), split(out, 3, SENTINEL), split(eb, J * K, SENTINEL), split(fl, 1, -77)
    assert all(float(v) == SENTINEL for v in env[:8].cpu()) and float(E[0]) == SENTINEL and int(fr[0]) == -77 and float(out[0]) == SENTINEL


# ---- 2. modulation energies on a given envelope ----------------------------------------------------------------------------------------------
def test_modulation_energies_vs_restatement(lib):
    """nine channels (two workgroups per row, the second with one channel) of a positive fp32 envelope; lengths 4095 (no frame), 4096, 5119, 5120, one
    staging chunk behind the first frame and the third hop edge, each with its neighbours, three to a batch.  Every E[j, k, m] within 1e-9 relative
    of ``lfilter`` and a windowed sum in float64 (two float64 forms of this recursion differ by at most 5e-12 on such energies), frames exact"""
    C = lib.buddy_modulation_chunk()
    lens = [4095, 4096, 5119, 5120, 4096 + C - 1, 4096 + C, 4096 + C + 1, 6143, 6144, 6145, 5121, 4097]
    Jm = 9
    rs = np.random.RandomState(3)
    worst = 0.0
    coef = (_lib.C.c_double * 48)(*S.modulation_bank().coef.reshape(-1).tolist())
    for s in range(0, len(lens), 3):
        ln = lens[s:s + 3]
        B, lde, ldm = len(ln), max(ln) + 2, max(R.frames_of(n) for n in ln) + 2
        env = np.full((B, Jm, lde), np.nan, np.float32)
        for b, n in enumerate(ln):
            for j in range(Jm):
                env[b, j, :n] = np.abs(R.speechlike(10 * s + 3 * b + j, n) + 0.05 * rs.standard_normal(n)).astype(np.float32)
        env_d, lens_d = torch.from_numpy(env).cuda(), dev_i32(ln)
        E, fr = guarded(B * Jm * K * ldm, torch.float64, SENTINEL), guarded(B, torch.int32, -77)
        rc = lib.buddy_modulation_energies(_lib.ptr(env_d), lens_d.data_ptr(), B, Jm, lde, coef, K, R.W, R.H, E.data_ptr(), ldm, fr.data_ptr(), _lib.stream_ptr())
        assert rc == 0, lib.buddy_last_error().decode()
        torch.cuda.synchronize()
        got = split(E, B * Jm * K * ldm, SENTINEL).reshape(B, Jm, K, ldm)
        assert split(fr, B, -77).tolist() == [R.frames_of(n) for n in ln]
        for b, n in enumerate(ln):
            M = R.frames_of(n)
            assert np.all(got[b, :, :, M:] == SENTINEL), n                               # nothing written behind the row's frames
            if M:
                want = R.frame_energies(env[b, :, :n].astype(np.float64))
                rel = np.abs(got[b, :, :, :M] - want) / want
                worst = max(worst, float(rel.max()))
                assert np.all(rel <= 1e-9), (n, float(rel.max()))
    print(f"modulation energies: worst relative error {worst:.3e}")


# ---- 3. the scores on given energies ---------------------------------------------------------------------------------------------------------
def test_scores_on_given_energies(lib):
    """every branch of K* (5, 6, 7, 8) through a chosen erb / lower-edge table, the strict > 0.9 rule on an exact tie and just above it, a zero
    denominator, a zero total, frames = 0.  Values within 1e-12 relative; K*, BW, the flags and the NaNs exact; Ebar is the mean over the frames"""
    low = np.array([3.0, 5.0, 8.0, 14.0, 23.0, 37.0, 61.0, 100.0])
    erbs = np.array([30.0, 50.0, 80.0, 120.0])
    Js = 4
    cases = []
    for j in range(4):
        e = np.full((Js, K), 1e-3)
        e[j] = 1.0 + 0.1 * np.arange(K)
        cases.append((e, 3))
    tie = np.zeros((Js, K))
    tie[0, 0], tie[1, 4] = 9.0, 1.0
    above = tie.copy()
    above[0, 0] = 9.0000001
    lowonly = np.zeros((Js, K))
    lowonly[:, :4] = 1.0
    cases += [(tie, 2), (above, 2), (lowonly, 2), (np.zeros((Js, K)), 2), (np.ones((Js, K)), 0)]
    want_k = [5, 6, 7, 8, 6, 5, 8, None, None]
    ldm = 4
    c_erb, c_low = (_lib.C.c_double * Js)(*erbs.tolist()), (_lib.C.c_double * K)(*low.tolist())
    for s in range(0, len(cases), 3):
        part = cases[s:s + 3]
        B = len(part)
        E = np.full((B, Js, K, ldm), np.nan)
        for b, (e, M) in enumerate(part):
            for m in range(M):
                E[b, :, :, m] = e * (1.0 + 0.5 * (m - (M - 1) / 2.0))                    # frames that average to e
        E_d, fr_d = torch.from_numpy(E).cuda(), dev_i32([M for _, M in part])
        out, eb, fl = guarded(B * 3, torch.float64, SENTINEL), guarded(B * Js * K, torch.float64, SENTINEL), guarded(B, torch.int32, -77)
        rc = lib.buddy_srmr_scores(E_d.data_ptr(), fr_d.data_ptr(), B, Js, K, ldm, c_erb, c_low, out.data_ptr(), eb.data_ptr(), fl.data_ptr(), _lib.stream_ptr())
        assert rc == 0, lib.buddy_last_error().decode()
        torch.cuda.synchronize()
        got, ebar, flags = split(out, B * 3, SENTINEL).reshape(B, 3), split(eb, B * Js * K, SENTINEL).reshape(B, Js, K), split(fl, B, -77)
        for b, (e, M) in enumerate(part):
            if M == 0:
                assert np.isnan(ebar[b]).all() and np.isnan(got[b]).all() and flags[b] == 0
                continue
            mean = np.zeros((Js, K))
            for m in range(M):
                mean = mean + E[b, :, :, m]
            mean = mean / M
            assert np.array_equal(ebar[b], mean), s + b
            w = R.scores(mean, M, erbs, low)
            print(f"scores case {s + b}: got {got[b].tolist()} flag {flags[b]}  want {w}")
            assert flags[b] == w[3]
            for q in (1, 2):
                assert (math.isnan(w[q]) and math.isnan(got[b, q])) or got[b, q] == w[q], (s + b, q)
            assert (math.isnan(w[0]) and math.isnan(got[b, 0])) or abs(got[b, 0] - w[0]) <= 1e-12 * abs(w[0]), s + b
            if want_k[s + b] is not None:
                assert got[b, 1] == want_k[s + b], s + b


# ---- 4. the whole call -----------------------------------------------------------------------------------------------------------------------
def _check_whole_call(fs, rows, lines):
    """``srmr`` on ragged rows at ``fs`` against the restatement: stages 2 and 3 on the downloaded envelope to 1e-9 relative, and the value against the
    float64 restatement within max(32 d32, 2^-20) relative, d32 the restatement's own difference with its fp32-envelope switch on and off"""
    lens = [len(r) for r in rows]
    x_d = padded(rows, max(lens) + 9)
    res = S.srmr(x_d, fs, lens=lens, return_envelope=True)
    env = res.envelope.cpu().numpy()
    ok = True
    for b, r in enumerate(rows):
        x16 = R.to_16k(r.astype(np.float64), fs)
        n16 = len(x16)
        assert int(res.samples[b]) == lens[b] and int(res.frames[b]) == R.frames_of(n16) >= 1
        st23 = R.from_envelope(env[b, :, :n16].astype(np.float64))
        assert int(res.flags[b]) == st23["flag"] == 1 and int(res.kstar[b]) == st23["kstar"] and abs(float(res.bandwidth[b]) / st23["bw"] - 1.0) <= 1e-12, b
        assert abs(float(res.values[b]) / st23["srmr"] - 1.0) <= 1e-9, b
        assert np.all(np.abs(res.energies[b].numpy() / st23["energies"] - 1.0) <= 1e-9), b
        w64, w32 = R.srmr(r.astype(np.float64), fs), R.srmr(r.astype(np.float64), fs, fp32=True)
        d32 = abs(w32["srmr"] / w64["srmr"] - 1.0)
        bound = max(32.0 * d32, 2.0 ** -20)
        rel = abs(float(res.values[b]) / w64["srmr"] - 1.0)
        line = (f"fs {fs:5d} row {b} samples {lens[b]:5d} frames {int(res.frames[b]):2d}: got {float(res.values[b]):.12f} restatement64 {w64['srmr']:.12f} "
                f"rel {rel:.3e} d32 {d32:.3e} bound {bound:.3e}  K* {int(res.kstar[b])} BW {float(res.bandwidth[b]):.2f}")
        print(line)
        lines.append(line)
        ok = ok and rel <= bound and int(res.kstar[b]) == w64["kstar"] and abs(float(res.bandwidth[b]) / w64["bw"] - 1.0) <= 1e-12
    assert ok, "\n".join(lines)                                    # the printed lines are what profiles/srmr_accuracy.txt records
    return res, x_d


def test_srmr_vs_restatement_16k():
    rows = [R.speechlike(u, L).astype(np.float32) for u, L in enumerate((24000, 17001, 4096))]
    rows[1] = signal.fftconvolve(rows[1].astype(np.float64), synth_rir(1, 5000, t60=0.4).astype(np.float64))[:17001].astype(np.float32)
    res, x_d = _check_whole_call(16000, rows, ["srmr at 16 kHz against the float64 restatement (tests/test_hip_srmr.py); bound = max(32 d32, 2^-20), relative", ""])
    alone = S.srmr(x_d[1:2, :17001].contiguous(), 16000)             # a row's result does not depend on its batch
    assert np.array_equal(alone.values.numpy().view(np.uint64), res.values[1:2].numpy().view(np.uint64))
    assert torch.equal(alone.energies, res.energies[1:2]) and int(alone.kstar[0]) == int(res.kstar[1])
    assert res.energies.shape == (3, 23, 8) and res.values.dtype == torch.float64
    short = S.srmr(x_d[:1, :4095].contiguous(), 16000)                # no full frame
    assert math.isnan(float(short.values[0])) and int(short.flags[0]) == 0 and int(short.frames[0]) == 0 and int(short.kstar[0]) == 0
    for bad in (7999, 16000.5):
        with pytest.raises(ValueError):
            S.srmr(x_d, bad)
    gain = S.srmr(3.7 * x_d[:1, :24000].contiguous(), 16000)          # the input gain cancels up to fp32 rounding of the scaled samples
    assert abs(float(gain.values[0]) / float(res.values[0]) - 1.0) < 2.0 ** -20


@pytest.mark.parametrize("fs,lens", [(48000, (24000, 15001)), (8000, (24000, 9000))])
def test_srmr_vs_restatement_other_rates(fs, lens):
    rows = []
    for u, L in enumerate(lens):
        x = signal.resample_poly(R.speechlike(u, int(math.ceil(L * 16000 / fs)) + 8), fs // 8000, 2)[:L]      # a speechlike signal at the rate fs
        rows.append(x.astype(np.float32))
    assert all(len(r) == L for r, L in zip(rows, lens))
    _check_whole_call(fs, rows, [])


def test_srmr_falls_with_reverberation():
    L = 24000
    x = R.speechlike(0, L)
    rows = [x] + [signal.fftconvolve(x, synth_rir(0, taps=int(1.2 * t60 * 16000) + 1000, t60=t60).astype(np.float64))[:L] for t60 in (0.2, 0.8)]
    want = [R.srmr(r)["srmr"] for r in rows]
    assert want[0] > want[1] > want[2]
    got = S.srmr(torch.from_numpy(np.stack(rows).astype(np.float32)).cuda(), 16000).values.tolist()
    print("dry, t60 0.2, t60 0.8:", " ".join(f"{v:.4f}" for v in got), " restatement:", " ".join(f"{v:.4f}" for v in want))
    assert got[0] > got[1] > got[2]


# ---- 5. the tester and the tool --------------------------------------------------------------------------------------------------------------
SMALL = ["tester.sampling_params.T=3", "tester.posterior_sampling.blind_hp.op_updates_per_step=2",
         "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "network.nf=32", "tester.noise.generator=philox", "tester.sub_batches=1",
         "+gpu=0", "tester.overriden_name=run", "+allow_random_init=true"]
COLUMNS = ["file", "samples_in", "samples_out", "srmr_in", "srmr_out", "srmr_delta", "kstar_in", "kstar_out", "bw_in", "bw_out", "flags_in", "flags_out",
           "frames_in", "frames_out"]


def _tree(base):
    out = {}
    for dp, _, fs in os.walk(base):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, base)] = open(p, "rb").read()
    return out


def _same(a, b):
    return (isinstance(a, float) and math.isnan(a) and math.isnan(b)) or a == b


def _reverberant(u, n, fs):
    x = signal.resample_poly(R.speechlike(u, int(math.ceil(n * 16000 / fs)) + 8), fs // 16000, 1)[:n] if fs != 16000 else R.speechlike(u, n)
    y = signal.fftconvolve(x, synth_rir(u, 2000).astype(np.float64))[:n]
    return (0.3 * y / np.abs(y).max()).astype(np.float32)


def _run_real(tmp, tag, extra):
    import test as cli
    data = os.path.join(tmp, "recordings")
    if not os.path.exists(data):
        os.makedirs(data)
        wavfile.write(os.path.join(data, "A.wav"), 48000, _reverberant(0, 21600, 48000))       # 0.45 s: 7200 samples at the model's rate
        wavfile.write(os.path.join(data, "C.wav"), 16000, _reverberant(1, 11200, 16000))
    out = os.path.join(tmp, tag)
    torch.manual_seed(0)                                      # +allow_random_init draws the network from torch's generator: the same weights in both runs
    t = cli.main(["--config-name=conf_VCTK.yaml", "tester=real_dereverberation_BUDDy", *SMALL, "tester.real_recordings.chunk_seconds=1.024",
                  "tester.real_recordings.overlap_seconds=0.128", f"model_dir={out}", f"dset.test.path={data}", "+batch_size=4", *extra])
    return t, os.path.join(out, "run", "real_blind_dereverberation", "VCTK_16k_4s_time")


def _recompute(base, subs):
    """score_signals on the wavs of the run, read back, per sub-directory"""
    names = sorted(f[:-4] for f in os.listdir(os.path.join(base, "reconstructed")) if f.endswith(".wav"))
    cols = {}
    for s in subs:
        sigs = []
        for n in names:
            fs, a = wavfile.read(os.path.join(base, s, n + ".wav"))
            assert a.dtype == np.float32 and a.ndim == 1
            sigs.append((a, fs))
        cols[s] = S.score_signals(sigs, "cuda")
    return names, cols


def _check_rows(rows, names, cols, clean=False):
    by = {r["file"]: r for r in rows}
    assert sorted(by) == names and len(rows) == len(names)                                # one line per written wav
    for b, n in enumerate(names):
        r = by[n]
        for tag, s in (("in", "degraded"), ("out", "reconstructed")):
            c = cols[s][b]
            assert _same(r[f"srmr_{tag}"], c["srmr"]) and r[f"kstar_{tag}"] == c["kstar"] and _same(r[f"bw_{tag}"], c["bw"]), (n, tag)
            assert r[f"flags_{tag}"] == c["flags"] and r[f"frames_{tag}"] == c["frames"] and r[f"samples_{tag}"] == c["samples"], (n, tag)
        assert _same(r["srmr_delta"], r["srmr_out"] - r["srmr_in"])
        assert r["flags_in"] == r["flags_out"] == 1 and math.isfinite(r["srmr_out"]) and r["srmr_in"] > 0.0
        if clean:
            c = cols["original"][b]
            assert r["srmr_clean"] == c["srmr"] and r["kstar_clean"] == c["kstar"] and r["bw_clean"] == c["bw"]


def _check_summary(base, rows, values):
    summ = R.read_csv(os.path.join(base, "srmr_summary.csv"))
    assert [s["value"] for s in summ] == values
    for s in summ:
        v = np.array([r[s["value"]] for r in rows])
        v = v[~np.isnan(v)]
        assert s["n"] == len(v) == len(rows) and s["mean"] == float(np.mean(v)) and s["median"] == float(np.median(v)) and s["std"] == float(np.std(v)), s


def test_tester_real_recordings_report_and_tool(tmp_path):
    t_on, on = _run_real(str(tmp_path), "on", ["tester.srmr.use=true"])
    rows = R.read_csv(os.path.join(on, "srmr.csv"))
    assert [r["file"] for r in rows] == [r["file"] for r in t_on.srmr_report] == ["A", "C"] and list(rows[0]) == list(t_on.srmr_report[0]) == COLUMNS
    names, cols = _recompute(on, ("degraded", "reconstructed"))
    _check_rows(rows, names, cols)
    by = {r["file"]: r for r in rows}
    assert (by["A"]["samples_in"], by["A"]["samples_out"], by["C"]["samples_in"], by["C"]["samples_out"]) == (7200, 21600, 11200, 11200)
    assert (by["A"]["frames_in"], by["A"]["frames_out"], by["C"]["frames_out"]) == (4, 4, 7)   # degraded/ at the model's rate, reconstructed/ at the input's
    _check_summary(on, rows, ["srmr_in", "srmr_out", "srmr_delta"])
    _, off = _run_real(str(tmp_path), "off", [])
    tree_on, tree_off = _tree(on), _tree(off)
    assert not [f for f in tree_off if f.endswith(".csv")]
    assert sorted(set(tree_on) - set(tree_off)) == ["srmr.csv", "srmr_summary.csv"] and not set(tree_off) - set(tree_on)
    wavs = [f for f in tree_off if f.endswith(".wav")]
    assert len(wavs) == 6
    for f in wavs:
        assert tree_on[f] == tree_off[f], f                    # every wav of the run is byte-identical with the report on
    # the tool, in a child process: the mode directory gives the tester's rows
    saved = open(os.path.join(on, "srmr.csv")).read()
    saved_summary = open(os.path.join(on, "srmr_summary.csv")).read()
    os.remove(os.path.join(on, "srmr.csv")), os.remove(os.path.join(on, "srmr_summary.csv"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "srmr.py"), on], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "srmr_out" in p.stdout
    assert open(os.path.join(on, "srmr.csv")).read() == saved and open(os.path.join(on, "srmr_summary.csv")).read() == saved_summary
    # in this process: a list of wavs (an int16 stereo file among them) and a pair of directories
    import importlib.util
    spec = importlib.util.spec_from_file_location("buddy_tools_srmr", os.path.join(ROOT, "tools", "srmr.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    y = _reverberant(2, 12000, 16000)
    st = str(tmp_path / "stereo.wav")
    wavfile.write(st, 16000, np.round(np.stack([y, 0.5 * y], axis=1) * 32767.0).astype(np.int16))
    outd = str(tmp_path / "scored")
    got = tool.main([st, os.path.join(on, "degraded", "C.wav"), "--out", outd])
    assert [r["file"] for r in got] == ["stereo", "C"] and got[1]["srmr_out"] == by["C"]["srmr_in"] and math.isnan(got[1]["srmr_in"])
    mono = np.mean(np.round(np.stack([y, 0.5 * y], axis=1) * 32767.0).astype(np.int16).astype(np.float64) / 32768.0, axis=1).astype(np.float32)
    assert got[0]["srmr_out"] == S.score_signals([(mono, 16000)], "cuda")[0]["srmr"]
    assert [r["file"] for r in R.read_csv(os.path.join(outd, "srmr.csv"))] == ["stereo", "C"]
    pair = tool.main(["--input", os.path.join(on, "degraded"), "--estimate", os.path.join(on, "reconstructed"), "--out", outd])
    assert [(r["file"], r["srmr_in"], r["srmr_out"]) for r in pair] == [(r["file"], r["srmr_in"], r["srmr_out"]) for r in rows]
    with pytest.raises(SystemExit):                          # nothing to score
        tool.main([])
    wavfile.write(str(tmp_path / "slow.wav"), 4000, y)
    with pytest.raises(SystemExit, match="8000"):
        tool.main([str(tmp_path / "slow.wav")])


def test_tester_paired_mode_writes_clean_columns(tmp_path):
    import test as cli
    data = str(tmp_path / "data")
    for u, n_rir in enumerate((3000, 2400)):
        for sub, x in (("clean", synth_clean(u, 16000)), ("rir", np.concatenate([np.zeros(37, np.float32), synth_rir(u, n_rir)]))):
            d = os.path.join(data, sub, "p001")
            os.makedirs(d, exist_ok=True)
            wavfile.write(os.path.join(d, f"p001_{u:03d}.wav"), 16000, x.astype(np.float32))
    out = str(tmp_path / "on")
    torch.manual_seed(0)
    t = cli.main(["--config-name=conf_VCTK.yaml", "tester=blind_dereverberation_BUDDy", *SMALL, f"model_dir={out}", f"dset.test.path={data}",
                  "dset.test.num_examples=2", "+batch_size=2", "tester.srmr.use=true"])
    base = os.path.join(out, "run", "blind_dereverberation", "VCTK_16k_4s_time")
    rows = R.read_csv(os.path.join(base, "srmr.csv"))
    assert list(rows[0]) == COLUMNS + ["srmr_clean", "kstar_clean", "bw_clean"] == list(t.srmr_report[0])
    names, cols = _recompute(base, ("degraded", "reconstructed", "original"))
    _check_rows(rows, names, cols, clean=True)
    assert all(r["samples_in"] == r["samples_out"] == 16000 and r["frames_out"] == 12 for r in rows)
    _check_summary(base, rows, ["srmr_in", "srmr_out", "srmr_delta", "srmr_clean"])
    assert sorted(f for f in os.listdir(base) if f.endswith(".csv")) == ["srmr.csv", "srmr_summary.csv"]      # the metrics block stays off
