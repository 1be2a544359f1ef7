"""GPU: the spectral distortion report (csrc/spectral.hip, buddy_amd/utils/spectral.py) against the float64 oracle tests/_spectral_ref.py: each C entry
alone on ragged rows with NaN behind every row and guard words behind every output, the whole call at 16 kHz and at 48 kHz, the tester writing its CSV
files and the stand-alone tool reading them back.

The cases (``_spectral_ref.pairs``): three rows of 12 000, 7777 and 559 samples at 16 kHz -- 73 (not a multiple of the four frames of a workgroup), 47 and
exactly one frame -- of second-order AR noise under a slow amplitude modulation with one exact-zero gap; the estimates are the first convolved with a
decaying-noise tail, the second with added noise, the third identical; a fourth row of 399 samples has no frame and must come back undefined."""
import functools
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _spectral_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_clean, synth_rir  # noqa: E402
from buddy_amd.utils import metrics as M  # noqa: E402
from buddy_amd.utils import spectral as S  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 12345.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24
NBIN = 257


@pytest.fixture(scope="module")
def lib():
    return _lib.require_gpu()


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def dev_f64(v):
    return torch.tensor(list(v), dtype=torch.float64, device="cuda")


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


@functools.lru_cache(maxsize=None)
def cases(fs=16000):
    """(estimates, clean signals) of the four rows at ``fs``; computed once, never modified"""
    es, xs = R.pairs(fs)
    short = R.ar_noise(7, 399 * (fs // 16000), fs)
    es, xs = es + [(0.5 * short).astype(np.float32)], xs + [short]
    for a in es + xs:
        a.setflags(write=False)
    return tuple(es), tuple(xs)


@functools.lru_cache(maxsize=None)
def oracle(fs, dtype):
    es, xs = cases(fs)
    return tuple(R.evaluate(e, x, fs, dtype) for e, x in zip(es, xs))


# ---- 1. magnitude spectra ------------------------------------------------------------------------------------------------------------------
def test_frame_spectra_vs_oracle(lib):
    """per (frame, bin): |got - want| <= 45 * 2^-24 * sqrt(512) * ||w x_m||_2, the bound of test_band_spectra_vs_oracle (nine radix-2 stages at about 5u
    relative each in the 2-norm, Parseval, and the magnitude is 1-Lipschitz in X).  Asserted on the CPU first: the oracle of the same row shifted by
    one sample misses that bound by more than 1e3 times it, so the bound cannot hide an indexing error.  Rows of 73, 47, 1 and 0 frames in one ragged
    batch; row 1 also alone."""
    es, xs = cases()
    rows = list(xs) + [es[0]]
    for r in rows[:2]:
        n = len(r) - 1
        fr = R.framed(r[:n])
        tol = 45 * U24 * math.sqrt(512.0) * np.sqrt(np.sum(fr * fr, axis=1))
        live = tol > 0.0
        miss = np.abs(R.spectra(r[1:]) - R.spectra(r[:n]))[live] / tol[live, None]
        assert miss.max() > 1e3, miss.max()

    def run(rws):
        B, ln = len(rws), [len(r) for r in rws]
        ld, ldf = max(ln) + 7, max(max(R.frames_of(n) for n in ln), 1) + 3
        x_d, lens_d = padded(rws, ld), dev_i32(ln)
        out = guarded(B * ldf * NBIN, torch.float32, SENTINEL)
        rc = lib.buddy_frame_spectra(_lib.ptr(x_d), lens_d.data_ptr(), B, ld, S.FRAME, S.HOP, _lib.ptr(out), ldf, _lib.stream_ptr())
        assert rc == 0, lib.buddy_last_error().decode()
        torch.cuda.synchronize()
        return split(out, B * ldf * NBIN, SENTINEL).reshape(B, ldf, NBIN)

    got = run(rows)
    assert [R.frames_of(len(r)) for r in rows] == [73, 47, 1, 0, 73]
    worst = 0.0
    for b, r in enumerate(rows):
        F = R.frames_of(len(r))
        assert np.all(got[b, F:] == SENTINEL), b                                          # nothing written behind the row's frames
        if not F:
            continue
        fr = R.framed(r)
        tol = 45 * U24 * math.sqrt(512.0) * np.sqrt(np.sum(fr * fr, axis=1))              # per frame; zero for the frames inside the gap
        err = np.abs(got[b, :F].astype(np.float64) - R.spectra(r))
        assert np.all(err <= tol[:, None]), (b, float((err[tol > 0] / tol[tol > 0, None]).max()))
        worst = max(worst, float((err[tol > 0] / tol[tol > 0, None]).max()))
        zero = [f for f in range(F) if not fr[f].any()]
        assert (zero == [19, 20, 21, 22]) == (F > 22) and not got[b, zero].any()          # an all-zero frame has an all-zero spectrum, exactly
    print(f"frame_spectra: worst error / bound {worst:.4f}")
    alone = run(rows[1:2])
    assert np.array_equal(alone[0, :47].view(np.uint32), got[1, :47].view(np.uint32))    # a row's result does not depend on its batch
    x_d, lens_d, out = padded(rows[:1], 12000), dev_i32([12000]), guarded(73 * NBIN, torch.float32, SENTINEL)
    for frame, hop, ldf in ((513, 160, 73), (0, 160, 73), (400, 0, 73), (400, 160, 72)):
        assert lib.buddy_frame_spectra(_lib.ptr(x_d), lens_d.data_ptr(), 1, 12000, frame, hop, _lib.ptr(out), ldf, _lib.stream_ptr()) == 2
    split(out, 73 * NBIN, SENTINEL)


# ---- 2. CD and fwSegSNR on given spectra ---------------------------------------------------------------------------------------------------
def given_spectra():
    """the oracle's own fp32 spectra of the four pairs as the library takes them: (B, ldf, 257) float32 with NaN behind every row's frames"""
    es, xs = cases()
    Fs = [R.frames_of(len(x)) for x in xs]
    ldf = max(Fs) + 2
    X, E = np.full((4, ldf, NBIN), np.nan, np.float32), np.full((4, ldf, NBIN), np.nan, np.float32)
    gd = []
    for b, (e, x) in enumerate(zip(es, xs)):
        X[b, :Fs[b]], E[b, :Fs[b]] = R.spectra(x, np.float32), R.spectra(e, np.float32)
        gd.append(R.gain_floor(e, x))
    return X, E, Fs, ldf, gd


def test_cd_and_fwsegsnr_on_given_spectra(lib):
    """the kernels on the oracle's fp32 spectra: only the order of the double sums differs, so the row values agree within 1e-10 (the project's bound
    for scores on given spectra) and the counted frames exactly.  Row 3 has no frame: NaN, flag 0, count 0."""
    X, E, Fs, ldf, gd = given_spectra()
    B = 4
    X_d, E_d, frames_d = torch.from_numpy(X).cuda(), torch.from_numpy(E).cuda(), dev_i32(Fs)
    g_d, d_d = dev_f64([g for g, _ in gd]), dev_f64([d for _, d in gd])
    st = _lib.stream_ptr()
    out, flags, counts = guarded(B, torch.float64, SENTINEL), guarded(B, torch.int32, -77), guarded(B, torch.int32, -77)
    nws = lib.buddy_cepstral_distance_workspace(B, max(Fs))
    assert nws == 8 * B * max(Fs) * 50
    ws = guarded(nws // 8, torch.float64, SENTINEL)
    rc = lib.buddy_cepstral_distance(_lib.ptr(X_d), _lib.ptr(E_d), frames_d.data_ptr(), B, ldf, g_d.data_ptr(), d_d.data_ptr(), out.data_ptr(), flags.data_ptr(),
                                     ws.data_ptr(), nws, st)
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    split(ws, nws // 8, SENTINEL)
    got, got_flags = split(out, B, SENTINEL).copy(), split(flags, B, -77).copy()
    assert got_flags.tolist() == [1, 1, 1, 0] and np.isnan(got[3])
    for b in range(3):
        want, fl = R.cd(X[b, :Fs[b]].astype(np.float64), E[b, :Fs[b]].astype(np.float64), *gd[b])
        print(f"cepstral_distance F {Fs[b]}: got {got[b]:.15f} want {want:.15f} ({abs(got[b] - want):.1e})")
        assert fl == 1 and abs(got[b] - want) <= 1e-10, b
    assert got[0] > 1.0 and got[1] > 0.5 and got[2] == 0.0
    assert lib.buddy_cepstral_distance(_lib.ptr(X_d), _lib.ptr(E_d), frames_d.data_ptr(), B, ldf, g_d.data_ptr(), d_d.data_ptr(), out.data_ptr(),
                                       flags.data_ptr(), ws.data_ptr(), nws - 8, st) == 2
    assert lib.buddy_cepstral_distance(_lib.ptr(X_d), _lib.ptr(E_d), frames_d.data_ptr(), B, max(Fs) - 1, g_d.data_ptr(), d_d.data_ptr(), out.data_ptr(),
                                       flags.data_ptr(), ws.data_ptr(), nws, st) == 2

    Md = torch.from_numpy(S.mel_bands().copy()).cuda()
    out, flags = guarded(B, torch.float64, SENTINEL), guarded(B, torch.int32, -77)
    nws = lib.buddy_fwsegsnr_workspace(B, max(Fs))
    assert nws == 16 * B * max(Fs)
    ws = guarded(nws // 8, torch.float64, SENTINEL)
    rc = lib.buddy_fwsegsnr(_lib.ptr(X_d), _lib.ptr(E_d), frames_d.data_ptr(), B, ldf, g_d.data_ptr(), Md.data_ptr(), 23, out.data_ptr(), counts.data_ptr(),
                            flags.data_ptr(), ws.data_ptr(), nws, st)
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    split(ws, nws // 8, SENTINEL)
    got, got_flags, got_counts = split(out, B, SENTINEL), split(flags, B, -77), split(counts, B, -77)
    assert got_flags.tolist() == [1, 1, 1, 0] and np.isnan(got[3]) and got_counts.tolist() == [69, 43, 1, 0]
    for b in range(3):
        want, fl, n = R.fwsegsnr(X[b, :Fs[b]].astype(np.float64), E[b, :Fs[b]].astype(np.float64), gd[b][0])
        print(f"fwsegsnr F {Fs[b]}: got {got[b]:.15f} want {want:.15f} ({abs(got[b] - want):.1e}) counted {got_counts[b]}")
        assert fl == 1 and n == got_counts[b] and abs(got[b] - want) <= 1e-10, b
    assert got[0] < 25.0 and abs(got[2] - 35.0) <= 1e-12
    assert lib.buddy_fwsegsnr(_lib.ptr(X_d), _lib.ptr(E_d), frames_d.data_ptr(), B, ldf, g_d.data_ptr(), Md.data_ptr(), 65, out.data_ptr(), counts.data_ptr(),
                              flags.data_ptr(), ws.data_ptr(), nws, st) == 2
    assert lib.buddy_fwsegsnr(_lib.ptr(X_d), _lib.ptr(E_d), frames_d.data_ptr(), B, ldf, g_d.data_ptr(), Md.data_ptr(), 23, out.data_ptr(), counts.data_ptr(),
                              flags.data_ptr(), ws.data_ptr(), nws - 8, st) == 2


# ---- 3. LLR ----------------------------------------------------------------------------------------------------------------------------------
def test_llr_vs_oracle(lib):
    """from the signals, all in double on both sides: row values within 1e-9 and counts exact.  Levinson-Durbin amplifies rounding by about the inverse
    of the normalised prediction error E_p / r[0]; the oracle shows it at or above 1e-3 in every counted frame of these inputs (asserted first), which
    leaves 2^-53 / 1e-3 times a few hundred operations far inside 1e-9."""
    es, xs = cases()
    want = [R.llr(e, x) for e, x in zip(es, xs)]
    assert min(w[3] for w in want[:3]) >= 1e-3, [w[3] for w in want]
    assert [w[2] for w in want] == [69, 43, 1, 0] and want[3][1] == 0
    B, ln = 4, [len(x) for x in xs]
    ld = max(ln) + 5
    e_d, x_d, lens_d = padded(es, ld), padded(xs, ld), dev_i32(ln)
    out, flags, counts = guarded(B, torch.float64, SENTINEL), guarded(B, torch.int32, -77), guarded(B, torch.int32, -77)
    nws = lib.buddy_llr_workspace(B, max(ln), S.FRAME, S.HOP)
    assert nws == 16 * B * 73
    ws = guarded(nws // 8, torch.float64, SENTINEL)
    st = _lib.stream_ptr()
    rc = lib.buddy_llr(_lib.ptr(e_d), _lib.ptr(x_d), lens_d.data_ptr(), B, ld, S.FRAME, S.HOP, S.LPC_ORDER, out.data_ptr(), counts.data_ptr(), flags.data_ptr(),
                       ws.data_ptr(), nws, st)
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    split(ws, nws // 8, SENTINEL)
    got, got_flags, got_counts = split(out, B, SENTINEL), split(flags, B, -77), split(counts, B, -77)
    assert got_flags.tolist() == [1, 1, 1, 0] and np.isnan(got[3]) and got_counts.tolist() == [69, 43, 1, 0]
    for b in range(3):
        print(f"llr row {b}: got {got[b]:.15f} want {want[b][0]:.15f} ({abs(got[b] - want[b][0]):.1e}) counted {got_counts[b]} min E_p / r0 {want[b][3]:.4f}")
        assert abs(got[b] - want[b][0]) <= 1e-9, b
    assert got[0] > 0.01 and got[1] > 0.01 and got[2] == 0.0
    for frame, hop, order, nb in ((513, 160, 12, nws), (400, 0, 12, nws), (400, 160, 17, nws), (400, 160, 0, nws), (400, 160, 12, nws - 8)):
        assert lib.buddy_llr(_lib.ptr(e_d), _lib.ptr(x_d), lens_d.data_ptr(), B, ld, frame, hop, order, out.data_ptr(), counts.data_ptr(), flags.data_ptr(),
                             ws.data_ptr(), nb, st) == 2


# ---- 4. and 5. the whole call --------------------------------------------------------------------------------------------------------------------
def test_evaluate_vs_oracle():
    """evaluate at 16 kHz and at 48 kHz (through the project's resampler) on the four rows, ragged through ``lens`` with NaN behind every row.  For
    every value |got - oracle64| <= max(32 D32, 2^-20): D32 is the largest difference, over the rows of the rate, between the oracle's fp32-rounded run
    and its float64 run (the largest, so that one lucky draw of a cancelling sum does not set the bound; another FFT factorisation and summation
    order has other error constants, hence the 32; 2^-20 is far below the digit these scores are read in).  Flags, frames and both counts exact.  Row
    1 scored alone equals row 1 of the batch bit for bit.  Every figure is written to profiles/spectral_accuracy.txt."""
    lines = ["spectral.evaluate against the float64 oracle (tests/test_hip_spectral.py::test_evaluate_vs_oracle); bound = max(32 D32, 2^-20), D32 the largest",
             "|oracle32 - oracle64| of the value over the rows of the rate", ""]
    ok = True
    for fs in (16000, 48000):
        es, xs = cases(fs)
        w64, w32 = oracle(fs, np.float64), oracle(fs, np.float32)
        lens = [len(x) for x in xs]
        B, L = 4, max(lens) + 9
        d32 = np.nanmax(np.abs(np.stack([a[0] for a in w64]) - np.stack([a[0] for a in w32]))[:3], axis=0)
        bound = np.maximum(32.0 * d32, 2.0 ** -20)
        e_d, x_d = padded(es, L), padded(xs, L)
        res = S.evaluate(e_d, x_d, fs, lens=lens)
        got = res.values.numpy()
        assert res.names == S.VALUES and res.alignment is None and res.samples.tolist() == lens
        for b in range(B):
            assert (int(res.flags[b]), int(res.frames[b]), int(res.llr_frames[b]), int(res.fwsegsnr_frames[b])) == w64[b][1:], (fs, b, w64[b][1:])
            for q, name in enumerate(S.VALUES):
                want = w64[b][0][q]
                if math.isnan(want):
                    assert b == 3 and math.isnan(got[b, q])
                    lines.append(f"{fs} Hz row {b} {name:>8}: undefined on both sides (no full frame)")
                    continue
                err = abs(got[b, q] - want)
                line = (f"{fs} Hz row {b} {name:>8}: got {got[b, q]:.12f} oracle64 {want:.12f} diff {err:.3e} d32(row) {abs(want - w32[b][0][q]):.3e} "
                        f"D32 {d32[q]:.3e} bound {bound[q]:.3e}")
                print(line)
                lines.append(line)
                ok = ok and err <= bound[q]
        assert res.frames.tolist() == [73, 47, 1, 0] and res.flags.tolist() == [7, 7, 7, 0]
        alone = S.evaluate(e_d[1:2, :lens[1]].contiguous(), x_d[1:2, :lens[1]].contiguous(), fs)
        assert np.array_equal(alone.values.numpy().view(np.uint64), res.values[1:2].numpy().view(np.uint64)), fs
        assert (int(alone.flags[0]), int(alone.llr_frames[0]), int(alone.fwsegsnr_frames[0])) == (7, int(res.llr_frames[1]), int(res.fwsegsnr_frames[1]))
        if fs == 16000:
            part = S.evaluate(e_d, x_d, fs, lens=lens, values=("llr",))
            assert torch.equal(part.values[:3, 1], res.values[:3, 1]) and torch.isnan(part.values[:, [0, 2]]).all() and part.flags.tolist() == [2, 2, 2, 0]
            assert part.names == ("llr",) and part.fwsegsnr_frames.tolist() == [0] * 4 and part.llr_frames.tolist() == res.llr_frames.tolist()
            with pytest.raises(ValueError):
                S.evaluate(e_d, x_d, 8000)
            with pytest.raises(ValueError):
                S.evaluate(e_d, x_d, fs, values=("pesq",))
            al = S.evaluate(e_d, x_d, fs, lens=lens, align=5.0)                           # the lag search at the input rate, then the same kernels
            ma = M.align(e_d, x_d, fs, lens=lens, max_lag_ms=5.0)
            assert al.alignment is not None and al.alignment.lag.tolist() == ma.lag.tolist() and al.samples.tolist() == ma.lens.tolist()
            hand = S.evaluate(ma.est, ma.ref, fs, lens=ma.lens)
            assert np.array_equal(al.values.numpy().view(np.uint64), hand.values.numpy().view(np.uint64))
    try:
        with open(os.path.join(ROOT, "profiles", "spectral_accuracy.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                                                              # a read-only checkout: the printed lines are the record
    assert ok, "\n".join(lines)


# ---- 6. the tester and the tool ------------------------------------------------------------------------------------------------------------------
SMALL = ["tester.sampling_params.T=3", "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "network.nf=32", "tester.noise.generator=philox",
         "tester.sub_batches=1", "+gpu=0", "tester.overriden_name=run", "+allow_random_init=true"]
COLUMNS = (["file", "samples"] + [f"{m}_{k}" for m in S.VALUES for k in ("in", "out", "delta")] +
           ["flags_in", "flags_out", "frames", "llr_frames_in", "llr_frames_out", "fwsegsnr_frames_in", "fwsegsnr_frames_out"])
LAGS = ["lag_in", "lag_out", "lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out", "align_flags_in", "align_flags_out"]


def _run_tester(tmp, tag, extra):
    """informed mode, the nf = 32 fixture network, two utterances of one second"""
    import test as cli
    data = os.path.join(tmp, "data")
    if not os.path.exists(data):
        for u, n_rir in enumerate((3000, 2400)):
            for sub, x in (("clean", synth_clean(u, 16000)), ("rir", np.concatenate([np.zeros(37, np.float32), synth_rir(u, n_rir)]))):
                d = os.path.join(data, sub, "p001")
                os.makedirs(d, exist_ok=True)
                wavfile.write(os.path.join(d, f"p001_{u:03d}.wav"), 16000, x.astype(np.float32))
    out = os.path.join(tmp, tag)
    torch.manual_seed(0)                                      # +allow_random_init draws the network from torch's generator: the same weights in every run
    t = cli.main(["--config-name=conf_VCTK.yaml", "tester=informed_dereverberation_DPS", *SMALL, f"model_dir={out}", f"dset.test.path={data}",
                  "dset.test.num_examples=2", "+batch_size=2", *extra])
    return t, os.path.join(out, "run", "informed_dereverberation", "VCTK_16k_4s_time")


def _files(base):
    return {os.path.relpath(os.path.join(dp, f), base): open(os.path.join(dp, f), "rb").read() for dp, _, fs in os.walk(base) for f in fs
            if f.endswith((".csv", ".wav"))}


def _same(a, b):
    return (isinstance(a, float) and math.isnan(a) and math.isnan(b)) or a == b


def _tool():
    spec = importlib.util.spec_from_file_location("buddy_tools_spectral", os.path.join(ROOT, "tools", "spectral.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _check_rows(base, rows, align=None):
    """spectral.csv rows against evaluate on the written wavs read back"""
    names = [r["file"] for r in rows]
    rd = {s: torch.from_numpy(np.stack([wavfile.read(os.path.join(base, s, n + ".wav"))[1] for n in names])).cuda() for s in ("original", "degraded", "reconstructed")}
    inp, out = S.evaluate(rd["degraded"], rd["original"], 16000, align=align), S.evaluate(rd["reconstructed"], rd["original"], 16000, align=align)
    for b, r in enumerate(rows):
        assert r["samples"] == int(out.samples[b]) and r["flags_in"] == int(inp.flags[b]) == 7 and r["flags_out"] == int(out.flags[b]) == 7
        assert r["frames"] == int(out.frames[b]) and (align is not None or r["frames"] == 98)
        assert r["llr_frames_in"] == int(inp.llr_frames[b]) and r["llr_frames_out"] == int(out.llr_frames[b]) > 0
        assert r["fwsegsnr_frames_in"] == int(inp.fwsegsnr_frames[b]) and r["fwsegsnr_frames_out"] == int(out.fwsegsnr_frames[b]) > 0
        for q, m in enumerate(S.VALUES):
            assert _same(r[m + "_in"], float(inp.values[b, q])) and _same(r[m + "_out"], float(out.values[b, q])), (b, m)
            assert _same(r[m + "_delta"], r[m + "_out"] - r[m + "_in"]) and math.isfinite(r[m + "_out"]), (b, m)
        assert 0.0 < r["cd_in"] <= 10.0 and 0.0 < r["llr_in"] <= 2.0 and -10.0 <= r["fwsegsnr_in"] < 35.0
    return inp, out


def test_tester_spectral_report_and_tool(tmp_path):
    """with tester.spectral.use the run writes spectral.csv and spectral_summary.csv, whose rows equal evaluate on the written wavs; with use=false, or
    with no spectral block at all, neither file exists and every other csv (metrics.csv and srmr.csv were asked for) and wav is the same, byte for
    byte; tools/spectral.py on the mode directory gives the tester's rows, and on two folders the _out columns alone"""
    tmp = str(tmp_path)
    both = ["tester.metrics.use=true", "tester.srmr.use=true"]
    t_on, on = _run_tester(tmp, "on", both + ["tester.spectral.use=true"])
    rows = R.read_csv(os.path.join(on, "spectral.csv"))
    assert list(rows[0]) == COLUMNS == list(t_on.spectral_report[0]) and [r["file"] for r in rows] == [r["file"] for r in t_on.spectral_report] and len(rows) == 2
    _check_rows(on, rows)
    summ = R.read_csv(os.path.join(on, "spectral_summary.csv"))
    assert [s["value"] for s in summ] == [f"{m}_{k}" for m in S.VALUES for k in ("in", "out", "delta")]
    for s in summ:
        v = np.array([r[s["value"]] for r in rows])
        assert s["n"] == 2 and s["mean"] == float(np.mean(v)) and s["median"] == float(np.median(v)) and s["std"] == float(np.std(v)), s
    _, off = _run_tester(tmp, "off", both + ["tester.spectral.use=false"])
    _, bare = _run_tester(tmp, "bare", both + ["tester.spectral=null"])
    f_on, f_off, f_bare = _files(on), _files(off), _files(bare)
    assert f_off == f_bare and "metrics.csv" in f_off and "srmr.csv" in f_off and not [f for f in f_off if "spectral" in f]
    assert sorted(set(f_on) - set(f_off)) == ["spectral.csv", "spectral_summary.csv"]
    assert all(f_on[f] == data for f, data in f_off.items())                             # the other reports and every wav do not depend on this one
    # the tool, in a child process: the mode directory gives the tester's rows
    saved = open(os.path.join(on, "spectral.csv")).read()
    os.remove(os.path.join(on, "spectral.csv"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "spectral.py"), on], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "fwsegsnr_out" in p.stdout
    again = open(os.path.join(on, "spectral.csv")).read()    # the same header and lines, the files in name order
    assert again.splitlines()[0] == saved.splitlines()[0] and sorted(again.splitlines()[1:]) == sorted(saved.splitlines()[1:]) == again.splitlines()[1:]
    # two folders, no input: the _in and _delta columns stay empty
    tool = _tool()
    outd = str(tmp_path / "scored")
    only = tool.main(["--reference", os.path.join(on, "original"), "--estimate", os.path.join(on, "reconstructed"), "--out", outd, "--values", "cd,llr"])
    back = R.read_csv(os.path.join(outd, "spectral.csv"))
    assert list(back[0]) == [c for c in COLUMNS if not c.startswith(("fwsegsnr_in", "fwsegsnr_out", "fwsegsnr_delta"))] and len(only) == 2
    by = {r["file"]: r for r in rows}
    for r in back:
        assert _same(r["cd_out"], by[r["file"]]["cd_out"]) and _same(r["llr_out"], by[r["file"]]["llr_out"]) and math.isnan(r["cd_in"]) and math.isnan(r["llr_delta"])
        assert r["flags_in"] == 0 and r["flags_out"] == 3 and r["llr_frames_in"] == 0 and r["fwsegsnr_frames_out"] == 0
    with pytest.raises(SystemExit):                          # half a call form
        tool.main(["--reference", outd])
    with pytest.raises(SystemExit, match="no wav name"):
        tool.main(["--reference", outd, "--estimate", os.path.join(on, "reconstructed")])


def test_tester_spectral_report_aligned(tmp_path):
    """with tester.metrics.align.use both reports score the same trimmed pairs: spectral.csv carries the eight lag columns of metrics.csv with the same
    values, its rows equal evaluate(..., align=50) on the written wavs, and tools/spectral.py --align reproduces them"""
    t_on, on = _run_tester(str(tmp_path), "on", ["tester.metrics.use=true", "tester.metrics.align.use=true", "tester.spectral.use=true"])
    rows, mrows = R.read_csv(os.path.join(on, "spectral.csv")), R.read_csv(os.path.join(on, "metrics.csv"))
    assert list(rows[0]) == COLUMNS + LAGS == list(t_on.spectral_report[0]) and [r["file"] for r in rows] == [r["file"] for r in mrows]
    for r, m in zip(rows, mrows):
        assert all(_same(r[c], m[c]) for c in LAGS + ["samples"]), (r, m)
        assert abs(r["lag_out"]) <= 800 and r["samples"] == 16000 - abs(r["lag_out"]) and r["align_flags_in"] & 1
    inp, out = _check_rows(on, rows, align=50)
    assert [r["lag_in"] for r in rows] == inp.alignment.lag.tolist() and [r["lag_out"] for r in rows] == out.alignment.lag.tolist()
    summ = [s["value"] for s in R.read_csv(os.path.join(on, "spectral_summary.csv"))]
    assert summ == [f"{m}_{k}" for m in S.VALUES for k in ("in", "out", "delta")] + ["lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out"]
    outd = str(tmp_path / "scored")
    again = _tool().main([on, "--align", "--out", outd])
    by = {r["file"]: r for r in t_on.spectral_report}
    assert len(again) == 2 and all(list(r) == COLUMNS + LAGS and all(_same(r[c], by[r["file"]][c]) for c in r) for r in again)
