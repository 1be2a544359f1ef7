"""GPU: the room-acoustics report (csrc/acoustics.hip, buddy_amd/utils/acoustics.py) against the float64 oracle tests/_acoustics_ref.py: the decay
analysis alone on given band signals, the FIR bank alone, the direct-path search, the whole call, and the tester writing its CSV files.  Rows are
ragged around the backward sweep's tile S (buddy_decay_tile); every output buffer carries guard words."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acoustics_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import acoustics as A  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 12345.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.require_gpu()


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def padded(rows, ld, fill):
    """rows of their own lengths -> (B, ld) float32 with ``fill`` behind every row"""
    out = np.full((len(rows), ld), fill, np.float32)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


# ---- 1. the analysis stage alone ------------------------------------------------------------------------------------------------------------
def decay_cases(S):
    """(lengths, n0, seeds): B = 3, nb = 2, band signals given directly.  Seeds chosen on the CPU so that no D[n] lies within 1e-6 dB of a range
    limit (asserted below).  Band 1 of row 0 is all zero in every case."""
    return {"ragged": ([S - 1, S + 1, 2 * S + 3], [0, (S + 1) // 2, 2 * S + 2], 100),
            "length2": ([2, 2, S + 1], [0, 1, S // 3], 200)}


@pytest.mark.parametrize("case", ["ragged", "length2"])
def test_decay_metrics_vs_oracle(lib, case):
    """the six doubles within 1e-8 relative (1e-8 dB for the two ratios): n <= 2^20 terms at 2^-53 per add plus a double log10, about 20x margin;
    edc_db within 1e-4 dB (stored as fp32); flags equal; guard words intact"""
    S = lib.buddy_decay_tile()
    fs = 8000
    lens, n0, seed = decay_cases(S)[case]
    B, nb = 3, 2
    g_rows = []
    for b, L in enumerate(lens):
        bands = [R.decaying_noise(seed + 10 * b + k, L, n0[b], 80.0 + 15.0 * k) for k in range(nb)]
        if b == 0:
            bands[1] = np.zeros(L, np.float32)
        g_rows.append(bands)
    want, want_flags, curves = R.analyse_bands(g_rows, n0, fs)
    margin = min(R.limit_margin_db(D) for row in curves for D in row)
    print(f"decay {case}: smallest distance of a D[n] to a range limit {margin:.3e} dB")
    assert margin > 1e-6                                     # the fitted sets are the same on both sides
    assert want_flags[0, 1] == 0 and np.isnan(want[0, 1]).all()

    ldg = max(lens) + 5
    g = np.full((B, nb, ldg), np.nan, np.float32)            # NaN behind every row: a read past the end would show
    for b in range(B):
        for k in range(nb):
            g[b, k, :lens[b]] = g_rows[b][k]
    gd = torch.from_numpy(g).cuda()
    out = torch.full((B * nb * 6 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    flags = torch.full((B * nb + GUARD,), -77, dtype=torch.int32, device="cuda")
    edc = torch.full((B * nb * ldg + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    lens_d, n0_d = dev_i32(lens), dev_i32(n0)                # named: a temporary would be freed, and its block reused, before the call reads it
    rc = lib.buddy_decay_metrics(_lib.ptr(gd), lens_d.data_ptr(), n0_d.data_ptr(), B, nb, ldg, fs, out.data_ptr(), flags.data_ptr(), _lib.ptr(edc),
                                 _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    out, flags, edc = out.cpu().numpy(), flags.cpu().numpy(), edc.cpu().numpy()
    assert np.all(out[B * nb * 6:] == SENTINEL) and np.all(flags[B * nb:] == -77) and np.all(edc[B * nb * ldg:] == SENTINEL)
    got, got_flags, edc = out[:B * nb * 6].reshape(B, nb, 6), flags[:B * nb].reshape(B, nb), edc[:B * nb * ldg].reshape(B, nb, ldg)
    assert np.array_equal(got_flags, want_flags), (got_flags, want_flags)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    w = R.half_up(0.0025 * fs)
    worst = np.zeros(6)
    worst_edc = 0.0
    for b in range(B):
        ns = max(n0[b] - w, 0)
        for k in range(nb):
            row, D = edc[b, k], curves[b][k]
            assert np.all(row[lens[b]:] == SENTINEL), (b, k)                       # nothing written behind the row
            assert np.isnan(row[:ns]).all(), (b, k)                                # not defined before the analysis start
            fin = np.isfinite(D)
            assert np.array_equal(np.isfinite(row[ns:lens[b]]), fin), (b, k)
            if fin.any():
                worst_edc = max(worst_edc, float(np.abs(row[ns:lens[b]][fin].astype(np.float64) - D[fin]).max()))
            for q in range(6):
                if np.isfinite(want[b, k, q]):
                    d = abs(got[b, k, q] - want[b, k, q])
                    worst[q] = max(worst[q], d if q in (R.C50, R.DRR) else d / abs(want[b, k, q]))
    print(f"decay {case}: worst EDT T20 T30 C50[dB] DRR[dB] Ts = " + " ".join(f"{v:.2e}" for v in worst) + f"; edc_db {worst_edc:.2e} dB")
    assert worst_edc <= 1e-4
    assert np.all(worst <= 1e-8), worst


def test_decay_metrics_without_the_curve(lib):
    """edc_db = NULL: the same values"""
    S = lib.buddy_decay_tile()
    L, fs = S + 1, 8000
    g = torch.from_numpy(R.decaying_noise(5, L, 3, 90.0)).cuda()
    lens_d, n0_d = dev_i32([L]), dev_i32([3])
    res = []
    for with_curve in (False, True):
        out = torch.empty(6, dtype=torch.float64, device="cuda")
        fl = torch.empty(1, dtype=torch.int32, device="cuda")
        e = torch.empty(L, device="cuda") if with_curve else None
        assert lib.buddy_decay_metrics(_lib.ptr(g), lens_d.data_ptr(), n0_d.data_ptr(), 1, 1, L, fs, out.data_ptr(), fl.data_ptr(), _lib.ptr(e),
                                       _lib.stream_ptr()) == 0
        res.append((out.cpu(), int(fl.cpu())))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1] == 0b111111111


# ---- 2. the bank stage alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("Nh", [1, 3, 129])
def test_fir_bank_vs_float64(lib, Nh, nb):
    """|g - g64| <= (Nh + 3) 2^-23 sum_j |bank[k][j]| max|h|: the resampler test's derivation with up = 1 (Nh products of relative error 2^-24 summed
    in fp32, each partial sum bounded by sum|bank| max|h|).  Band 0, the unit impulse, equals h bit for bit."""
    S = lib.buddy_decay_tile()
    lens = [S - 1, S + 1, 2 * S + 3]
    B, P = len(lens), (Nh - 1) // 2
    rs = np.random.RandomState(1000 + 10 * Nh + nb)
    rows = [rs.standard_normal(L).astype(np.float32) for L in lens]
    bank = np.zeros((nb, Nh), np.float32)
    bank[0, P] = 1.0
    for k in range(1, nb):
        bank[k] = rs.standard_normal(Nh).astype(np.float32)
    if nb > 2 and Nh > 3:
        bank[2, :P // 2] = 0.0                               # a shorter filter, centred and zero-padded
        bank[2, Nh - P // 2:] = 0.0
    ldh, ldg = max(lens) + 7, max(lens) + P + 3
    hd = torch.from_numpy(padded(rows, ldh, np.nan)).cuda()  # NaN behind every row: a read past lens[b] would show in g
    gbuf = torch.full((B * nb * ldg + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    lens_d, bank_d = dev_i32(lens), torch.from_numpy(bank).cuda()
    rc = lib.buddy_fir_bank(_lib.ptr(hd), lens_d.data_ptr(), B, ldh, _lib.ptr(bank_d), nb, Nh, _lib.ptr(gbuf), ldg, _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    gbuf = gbuf.cpu().numpy()
    assert np.all(gbuf[B * nb * ldg:] == SENTINEL)
    g = gbuf[:B * nb * ldg].reshape(B, nb, ldg)
    worst = 0.0
    for b, L in enumerate(lens):
        g64 = R.band_signals(rows[b], bank)
        assert g64.shape == (nb, L + P)
        for k in range(nb):
            assert np.all(g[b, k, L + P:] == SENTINEL), (b, k)                     # nothing written past g[b][k][lens[b] + P - 1]
            tol = (Nh + 3) * 2.0 ** -23 * np.abs(bank[k].astype(np.float64)).sum() * np.abs(rows[b]).max()
            err = np.abs(g[b, k, :L + P].astype(np.float64) - g64[k]).max()
            worst = max(worst, err / tol)
            assert err <= tol, (b, k, err, tol)
        assert np.array_equal(g[b, 0, :L].view(np.uint32), rows[b].view(np.uint32)) and np.all(g[b, 0, L:L + P] == 0)
    print(f"fir_bank Nh {Nh} nb {nb}: worst error / bound {worst:.3f}")


# ---- 3. the direct-path search --------------------------------------------------------------------------------------------------------------
def test_row_argmax_abs(lib):
    """ties -> the first index (also across threads and waves), a negative peak, a peak in the last valid sample, garbage behind lens[b] ignored"""
    rs = np.random.RandomState(3)
    lens = [1000, 777, 300, 1, 2000]
    rows = [(0.1 * rs.standard_normal(L)).astype(np.float32) for L in lens]
    rows[0][[700, 300, 301]] = [2.0, 2.0, -2.0]              # three equal magnitudes: 300 is the first (thread 44 against threads 188 and 45)
    rows[1][500] = -3.0                                      # a negative peak
    rows[2][299] = 1.5                                       # the last valid sample
    rows[4][:] = 0.0                                         # all equal: index 0
    want = [300, 500, 299, 0, 0]
    ldh = 2100
    h = padded(rows, ldh, 0.0)
    h[0, 1000:] = 1e9                                        # garbage behind the rows: larger than every peak, and NaN
    h[1, 777:] = np.nan
    h[2, 300] = -99.0
    h[3, 1:] = 7.0
    n0 = torch.full((len(lens) + GUARD,), -5, dtype=torch.int32, device="cuda")
    hd, lens_d = torch.from_numpy(h).cuda(), dev_i32(lens)
    rc = lib.buddy_row_argmax_abs(_lib.ptr(hd), lens_d.data_ptr(), len(lens), ldh, n0.data_ptr(), _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    n0 = n0.cpu().tolist()
    assert n0[:len(lens)] == want == [R.argmax_abs(r) for r in rows] and set(n0[len(lens):]) == {-5}


# ---- 4. the whole call ----------------------------------------------------------------------------------------------------------------------
def test_whole_call_vs_oracle():
    """rir_acoustics at 16 kHz with the default bank on the exponential of the host test and two decaying-noise RIRs, against the oracle in float64
    throughout.  The tolerance per value is 4x the largest difference the oracle itself shows between a float32 and a float64 FIR accumulation
    over exactly these inputs (measured here; recorded with the GPU's own differences in profiles/acoustics_accuracy.txt).  Flags equal."""
    fs = 16000
    rows = R.whole_call_rows(fs)
    bank = A.analysis_bank(fs)
    bank32 = bank.astype(np.float32)                          # the taps the device holds
    want, want_flags, want_n0 = R.analyse(rows, fs, bank32, np.float64)
    single, single_flags, _ = R.analyse(rows, fs, bank32, np.float32)
    assert np.array_equal(single_flags, want_flags)
    measured = R.value_differences(single, want)
    limits = 4.0 * measured
    lens = [len(r) for r in rows]
    h = torch.from_numpy(padded(rows, max(lens), 0.0)).cuda()
    res = A.rir_acoustics(h, fs, lens=lens, return_edc=True)
    assert res.bands == (0.0,) + tuple(float(c) for c in A.OCTAVES) and res.values.shape == (3, 7, 6) and res.values.dtype == torch.float64
    assert res.n0.tolist() == want_n0.tolist() == [0, 37, 0]
    got = res.values.numpy()
    gpu = R.value_differences(got, want)
    for q, name in enumerate(A.VALUES):
        unit = "dB" if q in (R.C50, R.DRR) else "relative"
        print(f"whole call {name:>3} ({unit}): oracle float32 FIR vs float64 FIR {measured[q]:.3e}  limit {limits[q]:.3e}  GPU vs float64 oracle {gpu[q]:.3e}")
    assert np.array_equal(res.flags.numpy(), want_flags), (res.flags.numpy(), want_flags)
    assert np.all(gpu <= limits), (gpu, limits)
    assert abs(got[0, 0, R.T30] / 0.5 - 1.0) < 1e-5          # the exponential's broadband T30 against the closed form
    P = (bank.shape[1] - 1) // 2
    assert res.edc_db.shape == (3, 7, max(lens) + P) and float(res.edc_db[0, 0, 0]) == 0.0
    assert torch.isnan(res.edc_db[2, :, lens[2] + P:]).all()  # behind a short row
    # a row's result does not depend on its neighbours
    alone = A.rir_acoustics(h[1:2, :lens[1]].contiguous(), fs)
    assert torch.equal(alone.values[0].nan_to_num(nan=-1.0), res.values[1].nan_to_num(nan=-1.0)) and torch.equal(alone.flags[0], res.flags[1])


# ---- 5. the tester ---------------------------------------------------------------------------------------------------------------------------
SMALL = ["tester.sampling_params.T=3", "tester.posterior_sampling.blind_hp.op_updates_per_step=2",
         "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "network.nf=32", "tester.noise.generator=philox", "tester.sub_batches=1",
         "+gpu=0", "tester.overriden_name=run", "+allow_random_init=true"]


def _tree(base):
    """{relative path: bytes} of every file under ``base``"""
    out = {}
    for dp, _, fs in os.walk(base):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, base)] = open(p, "rb").read()
    return out


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check_report(base, tester, paired):
    """acoustics.csv / parameters.csv under ``base``/estimated_rir against rir_acoustics of the written RIR wavs and the run's operator"""
    rdir = os.path.join(base, "estimated_rir")
    wavs = sorted(f[:-4] for f in os.listdir(rdir) if f.endswith(".wav"))
    rows = R.read_csv(os.path.join(rdir, "acoustics.csv"))
    names = list(dict.fromkeys(r["file"] for r in rows))
    assert sorted(names) == wavs                              # one line set per written RIR wav
    bands = ["broadband"] + [f"{c:g}" for c in A.OCTAVES]
    assert [r["band"] for r in rows] == bands * len(names)
    est = torch.from_numpy(np.stack([wavfile.read(os.path.join(rdir, n + ".wav"))[1] for n in names])).cuda()
    want = A.rir_acoustics(est, 16000)
    true = None
    if paired:
        tr = [wavfile.read(os.path.join(base, "true_rir", n + ".wav"))[1] for n in names]
        lens = [len(r) for r in tr]
        assert len(set(lens)) > 1                             # true RIRs of different lengths go through `lens`
        true = A.rir_acoustics(torch.from_numpy(padded(tr, max(lens), 0.0)).cuda(), 16000, lens=lens)
    for i, r in enumerate(rows):
        b, k = divmod(i, len(bands))
        for q, v in enumerate(A.VALUES):
            assert _same(r[v], float(want.values[b, k, q])), (r["file"], r["band"], v)
            if paired:
                assert _same(r["true_" + v], float(true.values[b, k, q])), (r["file"], r["band"], v)
                if v in A.ERROR_VALUES:
                    assert _same(r["err_" + v], float(want.values[b, k, q]) - float(true.values[b, k, q]))
        assert r["flags"] == int(want.flags[b, k]) and (not paired or r["true_flags"] == int(true.flags[b, k]))
        assert ("true_EDT" in r) == paired
    assert np.isfinite([r["Ts"] for r in rows]).all()
    # the operator of the run: one batch, one operator, rows in the order of the batch
    par = tester.sampler.operator.acoustic_parameters()
    prow = R.read_csv(os.path.join(rdir, "parameters.csv"))
    U, E, NB = par["T60"].shape
    assert NB == len(par["freqs"]) == 25 and (par["T60"] > 0).all()
    by_name = {}
    for r in prow:
        by_name.setdefault(r["file"], []).append(r)
    assert sorted(by_name) == wavs
    return by_name, par


def test_tester_paired_blind_report(tmp_path):
    import test as cli
    from buddy_amd.synth import synth_clean, synth_rir
    data = str(tmp_path / "data")
    for u, n_rir in enumerate((3000, 2400)):
        for sub, x in (("clean", synth_clean(u, 16000)), ("rir", np.concatenate([np.zeros(37, np.float32), synth_rir(u, n_rir)]))):
            d = os.path.join(data, sub, "p001")
            os.makedirs(d, exist_ok=True)
            wavfile.write(os.path.join(d, f"p001_{u:03d}.wav"), 16000, x.astype(np.float32))

    def run(tag, extra):
        out = str(tmp_path / tag)
        torch.manual_seed(0)                                  # +allow_random_init draws the network from torch's generator: the same weights in both runs
        t = cli.main(["--config-name=conf_VCTK.yaml", "tester=blind_dereverberation_BUDDy", *SMALL, f"model_dir={out}", f"dset.test.path={data}",
                      "dset.test.num_examples=2", "+batch_size=2", *extra])
        return t, os.path.join(out, "run", "blind_dereverberation", "VCTK_16k_4s_time")

    t_on, on = run("on", ["tester.rir_report.use=true"])
    by_name, par = _check_report(on, t_on, paired=True)
    names = sorted(by_name)
    for b, n in enumerate(names):                            # operator row b is utterance b of the one batch
        got = by_name[n]
        assert [(r["exponential"], r["freq_hz"]) for r in got] == [(e, f) for e in range(par["T60"].shape[1]) for f in par["freqs"]]
        assert [r["T60"] for r in got] == par["T60"][b].flatten().tolist() and [r["weight"] for r in got] == par["weights"][b].flatten().tolist()
    _, off = run("off", [])
    tree_on, tree_off = _tree(on), _tree(off)
    assert not [f for f in tree_off if f.endswith(".csv")]
    extra = sorted(set(tree_on) - set(tree_off))
    assert extra == ["estimated_rir/acoustics.csv", "estimated_rir/parameters.csv"]
    for f, data_off in tree_off.items():
        if f.endswith(".wav"):
            assert tree_on[f] == data_off, f                 # every wav of the run is byte-identical with the report on


@pytest.mark.parametrize("shared", [False, True])
def test_tester_real_recordings_report(tmp_path, shared):
    import test as cli
    from scipy import signal
    from buddy_amd.synth import synth_clean, synth_rir
    data = str(tmp_path / "recordings")
    os.makedirs(data)
    for u, (name, fs, sec) in enumerate((("A", 16000, 2.0), ("B", 48000, 1.2))):       # three and two chunks of 16 384 samples: one batch of five
        n = int(round(sec * fs))
        y = signal.fftconvolve(synth_clean(u, n).astype(np.float64), synth_rir(u, 2000).astype(np.float64))[:n]
        wavfile.write(os.path.join(data, name + ".wav"), fs, (0.3 * y / np.abs(y).max()).astype(np.float32))

    def run(tag, extra):
        out = str(tmp_path / tag)
        torch.manual_seed(0)                                  # +allow_random_init draws the network from torch's generator: the same weights in both runs
        t = cli.main(["--config-name=conf_VCTK.yaml", "tester=real_dereverberation_BUDDy", *SMALL, "tester.real_recordings.chunk_seconds=1.024",
                      "tester.real_recordings.overlap_seconds=0.128", f"tester.real_recordings.shared_rir={'true' if shared else 'false'}",
                      f"model_dir={out}", f"dset.test.path={data}", "+batch_size=8", *extra])
        return t, os.path.join(out, "run", "real_blind_dereverberation", "VCTK_16k_4s_time")

    t_on, on = run("on", ["tester.rir_report.use=true"])
    by_name, par = _check_report(on, t_on, paired=False)
    want_names = ["A", "B"] if shared else ["A_c0", "A_c1", "A_c2", "B_c0", "B_c1"]
    assert sorted(by_name) == want_names
    assert par["T60"].shape[0] == 5
    # one batch of five chunk rows in file-then-chunk order; with shared_rir the rows of a file hold one parameter set and the file reports its first
    row_of = {"A": 0, "B": 3} if shared else {n: b for b, n in enumerate(want_names)}
    for n, b in row_of.items():
        assert [r["T60"] for r in by_name[n]] == par["T60"][b].flatten().tolist() and [r["weight"] for r in by_name[n]] == par["weights"][b].flatten().tolist()
    _, off = run("off", ["tester.rir_report.use=false"])
    tree_on, tree_off = _tree(on), _tree(off)
    assert not [f for f in tree_off if f.endswith(".csv")]
    assert sorted(set(tree_on) - set(tree_off)) == ["estimated_rir/acoustics.csv", "estimated_rir/parameters.csv"]
    for f, data_off in tree_off.items():
        if f.endswith(".wav"):
            assert tree_on[f] == data_off, f
