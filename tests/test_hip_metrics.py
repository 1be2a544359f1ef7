"""GPU: the evaluation metrics (csrc/metrics.hip, buddy_amd/utils/metrics.py) against the float64 oracle tests/_metrics_ref.py: each C entry alone on
ragged rows with NaN behind every row and guard words behind every output, the whole call at 16 kHz, the tester writing its CSV files and the
stand-alone tool reading them back."""
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
import _metrics_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_clean, synth_rir  # noqa: E402
from buddy_amd.utils import metrics as M  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 12345.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24


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


def gap10(u):
    """gap signal u at 10 kHz, as the device's resampler would hand it on (fp32)"""
    return R.to_10k(R.gap_signal(u), 16000, np.float32).astype(np.float32)


# ---- 1. moments and SI-SDR -------------------------------------------------------------------------------------------------------------------
def test_pair_moments_vs_oracle(lib):
    """moments within 1e-12 relative, SI-SDR within 1e-9 dB (at most 2^20 double adds at 2^-53 each, as test_decay_metrics_vs_oracle derives it);
    flags equal.  Row 1 has a silent clean signal, row 3 an estimate that is the clean signal under a gain and an offset."""
    T = lib.buddy_metrics_tile()
    lens = [1, T - 1, T + 1, 2 * T + 3]
    rs = np.random.RandomState(11)
    xs = [synth_clean(20 + b, max(L, 64))[:L] for b, L in enumerate(lens)]
    es = [(x + 0.02 * rs.standard_normal(len(x))).astype(np.float32) for x in xs]
    xs[1] = np.zeros(lens[1], np.float32)
    es[3] = (np.float32(2.5) * xs[3] + np.float32(0.1)).astype(np.float32)
    ld = max(lens) + 5
    e_d, x_d, lens_d = padded(es, ld), padded(xs, ld), dev_i32(lens)
    out, flags = guarded(4 * 4, torch.float64, SENTINEL), guarded(4, torch.int32, -77)
    rc = lib.buddy_pair_moments(_lib.ptr(e_d), _lib.ptr(x_d), lens_d.data_ptr(), 4, ld, out.data_ptr(), flags.data_ptr(), _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    got, got_flags = split(out, 16, SENTINEL).reshape(4, 4), split(flags, 4, -77)
    want = [R.moments(e, x) for e, x in zip(es, xs)]
    assert got_flags.tolist() == [w[4] for w in want] == [0, 0, 1, 1]
    for b, w in enumerate(want):
        for q in range(3):
            err = abs(got[b, q] - w[q])
            print(f"pair_moments row {b} L {lens[b]} moment {q}: got {got[b, q]:.17g} want {w[q]:.17g} rel {err / max(abs(w[q]), 1e-300):.2e}")
            assert err <= 1e-12 * abs(w[q]), (b, q)
        print(f"pair_moments row {b}: SI-SDR got {got[b, 3]!r} want {w[3]!r} diff {abs(got[b, 3] - w[3]) if math.isfinite(w[3]) else 0.0:.2e} dB")
        assert got[b, 3] == w[3] if not math.isfinite(w[3]) else abs(got[b, 3] - w[3]) <= 1e-9, b
    assert want[1][3] == -math.inf and want[3][3] > 100.0
    assert abs(want[2][3] - float(M.si_sdr(torch.from_numpy(es[2]), torch.from_numpy(xs[2])))) < 1e-9


# ---- 2. silent-frame removal -----------------------------------------------------------------------------------------------------------------
def select_rows():
    """10 kHz rows: the five lengths around the frame grid, the three gap signals (interior silence), leading and trailing silence, one frame kept"""
    rows = [synth_clean(30 + i, L) for i, L in enumerate((255, 256, 383, 384, 256 + 128 * 9 + 77))]
    rows += [gap10(u) for u in range(3)]
    lead = synth_clean(40, 256 + 128 * 11)
    lead[:128 * 4 + 256] *= np.float32(1e-4)
    trail = synth_clean(41, 256 + 128 * 11 + 50)
    trail[128 * 7:] *= np.float32(1e-4)
    one = (np.float32(1e-4) * synth_clean(42, 256 + 128 * 6)).astype(np.float32)
    one[508:516] = np.float32(0.05)      # eight loud samples at the centre of frame 3: its neighbours see them under window values below 0.003
    return rows + [lead, trail, one]


def test_stoi_select_vs_oracle(lib):
    """K, F, src and lens_out equal; the rebuilt signals within 4 * 2^-24 * max|x| (two fp32 products and one add per sample); condition, asserted
    before the call: no E[f] within 1e-3 dB of its row's threshold"""
    rows = select_rows()
    B = len(rows)
    rs = np.random.RandomState(5)
    est = [(r + 0.01 * rs.standard_normal(len(r))).astype(np.float32) for r in rows]
    lens = [len(r) for r in rows]
    want_src = [R.kept_frames(r) for r in rows]
    assert min(R.threshold_margin_db(r) for r in rows) > 1e-3
    want_K, want_F = [len(s) for s in want_src], [R.frames_of(n) for n in lens]
    assert want_F[:5] == [0, 1, 1, 2, 10] and want_K[:5] == want_F[:5] and want_K[5:8] == [103, 103, 102] and want_F[5:8] == [116] * 3
    assert want_src[8][0] > 0 and want_src[9][-1] < want_F[9] - 1 and want_K[10] == 1          # leading / trailing silence, exactly one frame kept
    ld, ldf = max(lens) + 3, max(want_F) + 2
    ldo = (max(want_F) - 1) * 128 + 256 + 1
    x_d, e_d, lens_d = padded(rows, ld), padded(est, ld), dev_i32(lens)
    xo, eo = guarded(B * ldo, torch.float32, SENTINEL), guarded(B * ldo, torch.float32, SENTINEL)
    lo, K, F = (guarded(B, torch.int32, -77) for _ in range(3))
    src = guarded(B * ldf, torch.int32, -77)
    ws = torch.empty(B * ldf, dtype=torch.float64, device="cuda")
    assert lib.buddy_stoi_select_workspace(B, max(lens)) == 8 * B * max(want_F)
    rc = lib.buddy_stoi_select(_lib.ptr(x_d), _lib.ptr(e_d), lens_d.data_ptr(), B, ld, _lib.ptr(xo), _lib.ptr(eo), ldo, lo.data_ptr(), K.data_ptr(),
                               F.data_ptr(), src.data_ptr(), ldf, ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    xo, eo = split(xo, B * ldo, SENTINEL).reshape(B, ldo), split(eo, B * ldo, SENTINEL).reshape(B, ldo)
    src = split(src, B * ldf, -77).reshape(B, ldf)
    assert split(K, B, -77).tolist() == want_K and split(F, B, -77).tolist() == want_F
    assert split(lo, B, -77).tolist() == [(k - 1) * 128 + 256 if k else 0 for k in want_K]
    worst = 0.0
    for b in range(B):
        k = want_K[b]
        assert src[b, :k].tolist() == want_src[b].tolist() and np.all(src[b, k:] == -77), b
        n = (k - 1) * 128 + 256 if k else 0
        for got, sig in ((xo[b], rows[b]), (eo[b], est[b])):
            assert np.all(got[n:] == SENTINEL), b                                      # nothing written behind the rebuilt row
            if k:
                err = np.abs(got[:n].astype(np.float64) - R.rebuild(sig, want_src[b])).max()
                tol = 4 * U24 * np.abs(sig).max()
                worst = max(worst, err / tol)
                assert err <= tol, (b, err, tol)
    print(f"stoi_select: worst rebuilt-signal error / bound {worst:.3f}")


# ---- 3. band spectra -------------------------------------------------------------------------------------------------------------------------
def tone(k, n):
    return (0.3 * np.cos(2 * np.pi * k * np.arange(n) / 512.0 + 0.4)).astype(np.float32)


def test_band_spectra_vs_oracle(lib):
    """per (band, frame): |got - want| <= 45 * 2^-24 * sqrt(512) * ||w x_m||_2 -- nine radix-2 stages at about 5u relative each in the 2-norm give
    ||dX|| <= 45 u ||X||, ||X|| = sqrt(512) ||frame|| by Parseval, and the band root-sum-square is 1-Lipschitz in X.  Rows of 1, 29, 30 and 31
    frames in one ragged batch, each also alone; pure tones at the band-edge bins 9 and 219 and at bins 0 and 256."""
    lens = [256, 256 + 128 * 28 + 100, 256 + 128 * 29, 256 + 128 * 30 + 127]
    rows = [synth_clean(50 + i, L) for i, L in enumerate(lens)] + [tone(k, 256 + 128 * 2) for k in (9, 219, 0, 256)]
    J = len(R.BANDS)
    lo, hi = (_lib.C.c_int * J)(*[b[0] for b in R.BANDS]), (_lib.C.c_int * J)(*[b[1] for b in R.BANDS])

    def run(rws):
        B, ln = len(rws), [len(r) for r in rws]
        ld, ldm = max(ln) + 7, max(R.frames_of(n) for n in ln) + 3
        x_d, lens_d = padded(rws, ld), dev_i32(ln)
        out = guarded(B * J * ldm, torch.float32, SENTINEL)
        rc = lib.buddy_band_spectra(_lib.ptr(x_d), lens_d.data_ptr(), B, ld, lo, hi, J, _lib.ptr(out), ldm, _lib.stream_ptr())
        assert rc == 0, lib.buddy_last_error().decode()
        torch.cuda.synchronize()
        return split(out, B * J * ldm, SENTINEL).reshape(B, J, ldm)

    got = run(rows)
    assert [R.frames_of(len(r)) for r in rows[:4]] == [1, 29, 30, 31]
    worst = 0.0
    for b, r in enumerate(rows):
        Mb = R.frames_of(len(r))
        assert np.all(got[b, :, Mb:] == SENTINEL), b                                    # nothing written behind the row's frames
        want = R.band_spectra(r)
        fr = R.framed(r)
        tol = 45 * U24 * math.sqrt(512.0) * np.sqrt(np.sum(fr * fr, axis=1))          # per frame
        err = np.abs(got[b, :, :Mb].astype(np.float64) - want)
        worst = max(worst, float((err / tol[None, :]).max()))
        assert np.all(err <= tol[None, :]), (b, float((err / tol[None, :]).max()))
    print(f"band_spectra: worst error / bound {worst:.4f}")
    # the tones (inside the bound above like every row): bin 9 is the first bin of band 1 ([9, 11)) and outside band 0 ([7, 9)), which sees the
    # leakage of the zero-padded window only; bin 219 lies just outside the last band ([174, 219)); bins 0 and 256 belong to no band.  A band
    # shifted by one bin would move these values by far more than the bound
    for b, j in ((4, 1), (5, 14)):
        want = R.band_spectra(rows[b])[:, 1]
        assert np.argmax(got[b, :, 1]) == np.argmax(want) == j
        shifted = R.band_spectra(rows[b], bands=tuple((lo_ + 1, hi_ + 1) for lo_, hi_ in R.BANDS))[:, 1]
        assert abs(shifted[j] - want[j]) > 1e3 * 45 * U24 * math.sqrt(512.0) * np.linalg.norm(R.framed(rows[b])[1])
    alone = run(rows[1:2])
    assert np.array_equal(alone[0, :, :29].view(np.uint32), got[1, :, :29].view(np.uint32))   # a row's result does not depend on its batch


# ---- 4. the scores ---------------------------------------------------------------------------------------------------------------------------
def test_stoi_scores_vs_oracle(lib):
    """given fp32 band spectra of 29 (undefined), 30, 31 and 74 frames: STOI and ESTOI within 1e-10 of the oracle on the same arrays (double on
    both sides, 450 numbers per segment).  Row 2 has an all-zero clean band row in every segment and row 3 an all-zero estimated one: the eps path."""
    Ms = [29, 30, 31, 74]
    B, J = len(Ms), 15
    ldm = max(Ms) + 5
    rs = np.random.RandomState(7)
    X = np.full((B, J, ldm), np.nan, np.float32)
    Y = np.full((B, J, ldm), np.nan, np.float32)
    for b, m in enumerate(Ms):
        base = np.abs(rs.standard_normal((J, m))) + 0.1
        X[b, :, :m] = base
        Y[b, :, :m] = np.abs(base * (1.0 + 0.5 * rs.standard_normal((J, m))) + 0.2 * rs.standard_normal((J, m)))
    X[2, 4, :Ms[2]] = 0.0
    Y[3, 9, :Ms[3]] = 0.0
    Y[3, 2, 10:20] *= 50.0                                       # the clip of step (h) at work
    X_d, Y_d, lens_d = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), dev_i32(Ms)
    out, flags = guarded(B * 2, torch.float64, SENTINEL), guarded(B, torch.int32, -77)
    nws = lib.buddy_stoi_scores_workspace(B, max(Ms))
    assert nws == 16 * B * (max(Ms) - 29)
    ws = guarded(nws // 8, torch.float64, SENTINEL)
    rc = lib.buddy_stoi_scores(_lib.ptr(X_d), _lib.ptr(Y_d), lens_d.data_ptr(), B, J, ldm, out.data_ptr(), flags.data_ptr(), ws.data_ptr(), nws,
                               _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    split(ws, nws // 8, SENTINEL)
    got, got_flags = split(out, B * 2, SENTINEL).reshape(B, 2), split(flags, B, -77)
    assert got_flags.tolist() == [0, 1, 1, 1] and np.isnan(got[0]).all()
    for b in range(1, B):
        s, es, fl = R.stoi_scores(X[b, :, :Ms[b]], Y[b, :, :Ms[b]])
        print(f"stoi_scores M {Ms[b]}: STOI got {got[b, 0]:.15f} want {s:.15f} ({abs(got[b, 0] - s):.1e})  ESTOI got {got[b, 1]:.15f} want {es:.15f} "
              f"({abs(got[b, 1] - es):.1e})")
        assert fl == 1 and abs(got[b, 0] - s) <= 1e-10 and abs(got[b, 1] - es) <= 1e-10, b


# ---- 5. the whole call -----------------------------------------------------------------------------------------------------------------------
def whole_call_pairs():
    xs = [R.gap_signal(u) for u in range(3)]
    es = [signal.fftconvolve(x.astype(np.float64), synth_rir(u, 3000).astype(np.float64))[:len(x)].astype(np.float32) for u, x in enumerate(xs)]
    return xs + [xs[0]], es + [es[0]], [24000, 24000, 24000, 12000]


def test_evaluate_vs_oracle():
    """evaluate at 16 kHz on the three gap signals under a synthetic RIR plus one row cut to 12 000 samples through ``lens``.  For STOI, ESTOI and LSD
    |got - oracle64| <= max(32 d32, 2^-20), d32 the difference of the oracle's own fp32 run of the same case (another FFT factorisation and
    summation order has other error constants, and one signal's d32 is a single draw of a cancelling sum; 2^-20 is three decades below the digit
    these scores are read in).  Asserted on the CPU first: leaving one kept frame out of the oracle moves STOI and ESTOI by more than 100 times the
    bound, so the bound cannot hide an indexing error.  kept_frames and frames equal; a row evaluated alone equals its batched result bit for bit."""
    xs, es, lens = whole_call_pairs()
    fs, B, L = 16000, 4, 24000
    want, want32, bound = [], [], []
    for b in range(B):
        e, x = es[b][:lens[b]], xs[b][:lens[b]]
        w64, w32 = R.evaluate(e, x, fs), R.evaluate(e, x, fs, np.float32)
        want.append(w64)
        want32.append(w32)
        d32 = np.abs(w64[0] - w32[0])
        bd = np.maximum(32.0 * d32, 2.0 ** -20)
        bound.append(bd)
        s1, es1 = R.stoi(e, x, fs, drop=0)[:2]                # the first kept frame: every segment boundary behind it moves
        assert abs(s1 - w64[0][1]) > 100 * bd[1] and abs(es1 - w64[0][2]) > 100 * bd[2], (b, s1, es1)
    for b, (s, t) in enumerate(((0.666, 0.188), (0.636, 0.223), (0.604, 0.135))):
        assert abs(want[b][0][1] - s) < 5e-4 and abs(want[b][0][2] - t) < 5e-4
    e_d, x_d = padded(es, L + 9), padded(xs, L + 9)
    e_d[3, lens[3]:] = float("nan")
    x_d[3, lens[3]:] = float("nan")
    res = M.evaluate(e_d, x_d, fs, lens=lens)
    got = res.values.numpy()
    lines = ["evaluate at 16 kHz against the float64 oracle (tests/test_hip_metrics.py::test_evaluate_vs_oracle); bound = max(32 d32, 2^-20)", ""]
    ok = True
    for b in range(B):
        assert int(res.flags[b]) == want[b][1] == 15 and int(res.kept_frames[b]) == want[b][2] and int(res.frames[b]) == want[b][3], b
        assert int(res.samples[b]) == lens[b]
        for q, name in enumerate(M.VALUES):
            err = abs(got[b, q] - want[b][0][q])
            line = (f"row {b} {name:>6}: got {got[b, q]:.12f} oracle64 {want[b][0][q]:.12f} diff {err:.3e} d32 {abs(want[b][0][q] - want32[b][0][q]):.3e} "
                    f"bound {bound[b][q]:.3e}" + ("" if q else " (SI-SDR: 1e-9 dB)"))
            print(line)
            lines.append(line)
            ok = ok and (err <= bound[b][q] if q else err <= 1e-9)
    assert ok, "\n".join(lines)                                # the printed lines are what profiles/metrics_accuracy.txt records
    assert res.kept_frames.tolist()[:3] == [103, 103, 102] and res.frames.tolist()[:3] == [116] * 3
    for b in (1, 3):
        alone = M.evaluate(e_d[b:b + 1, :lens[b]].contiguous(), x_d[b:b + 1, :lens[b]].contiguous(), fs)
        assert np.array_equal(alone.values.numpy().view(np.uint64), res.values[b:b + 1].numpy().view(np.uint64)), b
        assert int(alone.flags[0]) == int(res.flags[b]) and int(alone.kept_frames[0]) == int(res.kept_frames[b])
    part = M.evaluate(e_d, x_d, fs, lens=lens, values=("stoi",))
    assert torch.equal(part.values[:, 1], res.values[:, 1]) and torch.isnan(part.values[:, [0, 2, 3]]).all() and part.flags.tolist() == [2] * 4
    with pytest.raises(ValueError):
        M.evaluate(e_d, x_d, 8000)
    with pytest.raises(ValueError):
        M.evaluate(e_d, x_d, fs, values=("pesq",))
    short = M.evaluate(e_d[:1, :3000].contiguous(), x_d[:1, :3000].contiguous(), fs)      # 1875 samples at 10 kHz: 13 frames, no segment
    assert int(short.flags[0]) == 0b1001 and torch.isnan(short.values[0, 1:3]).all() and int(short.frames[0]) == 13


# ---- 6. the tester ---------------------------------------------------------------------------------------------------------------------------
SMALL = ["tester.sampling_params.T=3", "tester.posterior_sampling.blind_hp.op_updates_per_step=2",
         "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "network.nf=32", "tester.noise.generator=philox", "tester.sub_batches=1",
         "+gpu=0", "tester.overriden_name=run", "+allow_random_init=true"]
MODES = {"blind": ("blind_dereverberation_BUDDy", "blind_dereverberation"), "informed": ("informed_dereverberation_DPS", "informed_dereverberation")}


def _tree(base):
    out = {}
    for dp, _, fs in os.walk(base):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, base)] = open(p, "rb").read()
    return out


def _same(a, b):
    return (isinstance(a, float) and math.isnan(a) and math.isnan(b)) or a == b


def _run_tester(tmp, kind, tag, extra):
    import test as cli
    data = os.path.join(tmp, "data")
    if not os.path.exists(data):
        for u, n_rir in enumerate((3000, 2400)):
            for sub, x in (("clean", synth_clean(u, 16000)), ("rir", np.concatenate([np.zeros(37, np.float32), synth_rir(u, n_rir)]))):
                d = os.path.join(data, sub, "p001")
                os.makedirs(d, exist_ok=True)
                wavfile.write(os.path.join(d, f"p001_{u:03d}.wav"), 16000, x.astype(np.float32))
    out = os.path.join(tmp, tag)
    torch.manual_seed(0)                                      # +allow_random_init draws the network from torch's generator: the same weights in both runs
    t = cli.main(["--config-name=conf_VCTK.yaml", f"tester={MODES[kind][0]}", *SMALL, f"model_dir={out}", f"dset.test.path={data}",
                  "dset.test.num_examples=2", "+batch_size=2", *extra])
    return t, os.path.join(out, "run", MODES[kind][1], "VCTK_16k_4s_time")


def _check_metrics(base, rows):
    """metrics.csv rows against evaluate on the written wavs read back, and the summary against numpy"""
    names = sorted(f[:-4] for f in os.listdir(os.path.join(base, "reconstructed")) if f.endswith(".wav"))
    assert sorted(r["file"] for r in rows) == names and len(names) == 2                # one line per written wav
    rd = {s: torch.from_numpy(np.stack([wavfile.read(os.path.join(base, s, n + ".wav"))[1] for n in names])).cuda()
          for s in ("original", "degraded", "reconstructed")}
    inp, out = M.evaluate(rd["degraded"], rd["original"], 16000), M.evaluate(rd["reconstructed"], rd["original"], 16000)
    by = {r["file"]: r for r in rows}
    for b, n in enumerate(names):
        r = by[n]
        assert r["samples"] == 16000 and r["flags_in"] == int(inp.flags[b]) and r["flags_out"] == int(out.flags[b])
        assert r["kept_frames"] == int(out.kept_frames[b]) and r["frames"] == int(out.frames[b]) == 77
        for q, m in enumerate(M.VALUES):
            assert _same(r[m + "_in"], float(inp.values[b, q])) and _same(r[m + "_out"], float(out.values[b, q])), (n, m)
            assert _same(r[m + "_delta"], r[m + "_out"] - r[m + "_in"]), (n, m)
        assert math.isfinite(r["si_sdr_out"]) and math.isfinite(r["lsd_out"]) and 0.0 < r["stoi_in"] <= 1.0
    summ = R.read_csv(os.path.join(base, "metrics_summary.csv"))
    assert [s["value"] for s in summ] == [f"{m}_{k}" for m in M.VALUES for k in ("in", "out", "delta")]
    for s in summ:
        v = np.array([r[s["value"]] for r in rows])
        v = v[~np.isnan(v)]
        assert s["n"] == len(v) == 2 and s["mean"] == float(np.mean(v)) and s["median"] == float(np.median(v)) and s["std"] == float(np.std(v)), s


@pytest.mark.parametrize("kind", ["blind", "informed"])
def test_tester_metrics_report(tmp_path, kind):
    t_on, on = _run_tester(str(tmp_path), kind, "on", ["tester.metrics.use=true"])
    rows = R.read_csv(os.path.join(on, "metrics.csv"))
    assert [r["file"] for r in rows] == [r["file"] for r in t_on.metrics_report] and rows[0].keys() == t_on.metrics_report[0].keys()
    _check_metrics(on, rows)
    _, off = _run_tester(str(tmp_path), kind, "off", [])
    tree_on, tree_off = _tree(on), _tree(off)
    assert not [f for f in tree_off if f.endswith(".csv")]
    assert sorted(set(tree_on) - set(tree_off)) == ["metrics.csv", "metrics_summary.csv"]
    for f, data_off in tree_off.items():
        if f.endswith(".wav"):
            assert tree_on[f] == data_off, f                 # every wav of the run is byte-identical with the report on
    if kind != "blind":
        return
    # 7. the tool, in a child process: the mode directory gives the tester's rows; then a folder with an int16 wav and a pair of unequal lengths
    saved = open(os.path.join(on, "metrics.csv")).read()
    os.remove(os.path.join(on, "metrics.csv"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), on], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "si_sdr_out" in p.stdout
    again = open(os.path.join(on, "metrics.csv")).read()     # the same header and lines, the files in name order instead of the run's order
    assert again.splitlines()[0] == saved.splitlines()[0] and sorted(again.splitlines()[1:]) == sorted(saved.splitlines()[1:]) == again.splitlines()[1:]
    ref, est = str(tmp_path / "ref"), str(tmp_path / "est")
    os.makedirs(ref), os.makedirs(est)
    x0, x1 = synth_clean(0, 9000), synth_clean(1, 9000)
    e0, e1 = signal.fftconvolve(x0, synth_rir(0, 800))[:9000], signal.fftconvolve(x1, synth_rir(1, 800))[:8000]
    q = lambda a: np.round(np.clip(a, -1.0, 1.0 - 2.0 ** -15) * 32768.0).astype(np.int16)
    wavfile.write(os.path.join(ref, "a.wav"), 16000, q(x0))
    wavfile.write(os.path.join(est, "a.wav"), 16000, e0.astype(np.float32))
    wavfile.write(os.path.join(ref, "b.wav"), 16000, x1)
    wavfile.write(os.path.join(est, "b.wav"), 16000, e1.astype(np.float32))
    wavfile.write(os.path.join(est, "unmatched.wav"), 16000, x1)
    outd = str(tmp_path / "scored")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), "--reference", ref, "--estimate", est, "--out", outd], capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = R.read_csv(os.path.join(outd, "metrics.csv"))
    assert [(r["file"], r["samples"]) for r in rows] == [("a", 9000), ("b", 8000)]
    xa = torch.from_numpy(q(x0).astype(np.float64) / 32768.0).float()[None].cuda()
    wa = M.evaluate(torch.from_numpy(e0.astype(np.float32))[None].cuda(), xa, 16000)
    wb = M.evaluate(torch.from_numpy(e1.astype(np.float32))[None].cuda(), torch.from_numpy(x1[:8000])[None].cuda(), 16000)
    for r, w in zip(rows, (wa, wb)):
        for k, m in enumerate(M.VALUES):
            assert _same(r[m + "_out"], float(w.values[0, k])) and math.isnan(r[m + "_in"]) and math.isnan(r[m + "_delta"]), (r["file"], m)
    import importlib.util
    spec = importlib.util.spec_from_file_location("buddy_tools_evaluate", os.path.join(ROOT, "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with pytest.raises(SystemExit):                          # half a call form
        tool.main(["--reference", ref])
    wavfile.write(os.path.join(est, "a.wav"), 8000, e0.astype(np.float32))
    with pytest.raises(SystemExit, match="rates"):           # two rates within a pair are refused
        tool.main(["--reference", ref, "--estimate", est, "--out", outd])
