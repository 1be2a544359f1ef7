"""GPU: the blind decay time (csrc/decay.hip, buddy_amd/utils/decay.py) against the float64 restatement tests/_decay_ref.py: the band energies on ragged
rows within the bound of an fp32 transform, the regions and the select on crafted energies fed to both sides (starts, lengths, counts and flags bit for
bit, the times within the bound of the double sums), the chain on the library's own energies, the functional condition, other rates, refused arguments,
and the tester and the stand-alone tool writing and reading back their CSV files."""
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
import _decay_ref as R  # noqa: E402
from _srmr_ref import read_csv  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.synth import synth_clean, synth_rir  # noqa: E402
from buddy_amd.utils import decay as D  # noqa: E402
from buddy_amd.utils import resample as RS  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 12345.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS_FFT = 2.0 ** -18          # the relative 2-norm error of the fp32 window and nine radix-2 stages, 62 u rounded up to 64 u
NOMINAL = (0.2, 0.3, 0.5, 0.7, 1.0)
NB = 7


@pytest.fixture(scope="module")
def lib():
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def condition_rows():
    """the functional condition's signals, made once: seeds 0..5 at five decay times, then the six dry sources; float32 as the library takes them"""
    rows = [R.reverberant(seed, t60).astype(np.float32) for seed in range(6) for t60 in NOMINAL] + [R.burst_source(seed).astype(np.float32) for seed in range(6)]
    for r in rows:
        r.setflags(write=False)
    return rows


def dev_i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def c_ints(v):
    return (_lib.C.c_int * len(v))(*[int(a) for a in v])


def padded(rows, ld, fill=np.nan, dtype=np.float32):
    """rows of their own lengths -> (B, ld) on the device with ``fill`` behind every row (NaN: a read past the end would show)"""
    out = np.full((len(rows), ld), fill, dtype)
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


def run_energies(lib, rows, fs=16000, extra=2):
    """E (B, 7, ldm) and frames (B,) of ragged rows at 16 kHz, downloaded; nothing is written behind a row's frames"""
    B, lens = len(rows), [len(r) for r in rows]
    ld, ldm = max(lens) + 5, max(max(R.frames_of(n) for n in lens), 1) + extra
    lo, hi, _ = D.bin_ranges(fs)
    x_d, lens_d = padded(rows, ld), dev_i32(lens)
    E, fr = guarded(B * NB * ldm, torch.float64, SENTINEL), guarded(B, torch.int32, -77)
    rc = lib.buddy_decay_energies(_lib.ptr(x_d), lens_d.data_ptr(), B, ld, c_ints(lo), c_ints(hi), NB, E.data_ptr(), ldm, fr.data_ptr(), _lib.stream_ptr())
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    got, frames = split(E, B * NB * ldm, SENTINEL).reshape(B, NB, ldm), split(fr, B, -77)
    assert frames.tolist() == [R.frames_of(n) for n in lens]
    for b, M in enumerate(frames):
        assert np.all(got[b, :, M:] == SENTINEL), b
    return got, frames


def run_regions(lib, E_rows, q, nb=1, lmin=6, floor_rel=1e-6, extra=3):
    """steps 2-5 on given energies: ``E_rows`` is a list of (nb, M_b) arrays.  -> per row (T (nb, M), len (nb, M), out (nb, 3), counts (nb,)),
    downloaded; every word at or behind a row's frames still holds its sentinel"""
    B, Ms = len(E_rows), [e.shape[1] for e in E_rows]
    ldm = max(max(Ms), 1) + extra
    E = np.full((B, nb, ldm), np.nan)
    for b, e in enumerate(E_rows):
        E[b, :, :Ms[b]] = e
    E_d, fr_d = torch.from_numpy(E).cuda(), dev_i32(Ms)
    T, ln = guarded(B * nb * ldm, torch.float64, SENTINEL), guarded(B * nb * ldm, torch.int32, -77)
    st = _lib.stream_ptr()
    rc = lib.buddy_decay_regions(E_d.data_ptr(), fr_d.data_ptr(), B, nb, ldm, R.K, lmin, q, floor_rel, T.data_ptr(), ln.data_ptr(), st)
    assert rc == 0, lib.buddy_last_error().decode()
    out, cnt = guarded(B * nb * 3, torch.float64, SENTINEL), guarded(B * nb, torch.int32, -77)
    rc = lib.buddy_decay_select(T.data_ptr(), fr_d.data_ptr(), B, nb, ldm, out.data_ptr(), cnt.data_ptr(), st)
    assert rc == 0, lib.buddy_last_error().decode()
    torch.cuda.synchronize()
    Tg, lg = split(T, B * nb * ldm, SENTINEL).reshape(B, nb, ldm), split(ln, B * nb * ldm, -77).reshape(B, nb, ldm)
    og, cg = split(out, B * nb * 3, SENTINEL).reshape(B, nb, 3), split(cnt, B * nb, -77).reshape(B, nb)
    res = []
    for b, M in enumerate(Ms):
        assert np.all(Tg[b, :, M:] == SENTINEL) and np.all(lg[b, :, M:] == -77), b
        res.append((Tg[b, :, :M], lg[b, :, :M], og[b], cg[b]))
    return res


def check_band(name, got, E, q, lmin=6, floor_rel=1e-6, want=None):
    """one (row, band) of ``run_regions`` against steps 2-5 of the restatement on the same doubles: starts, lengths and the count bit for bit, every
    time and the three order statistics within ``R.time_bound``.  -> the largest share of the bound met"""
    T, ln, out, cnt = got
    ref = R.regions(E, q, floor_rel, lmin)
    if want is not None:
        assert [(v[0], v[1]) for v in ref] == want, name
    starts = np.flatnonzero(~np.isnan(T))
    assert starts.tolist() == [v[0] for v in ref] and ln[starts].tolist() == [v[1] for v in ref], (name, starts.tolist(), ln[starts].tolist(), [v[:2] for v in ref])
    assert np.all(ln[np.isnan(T)] == 0) and int(cnt) == len(ref), name
    share, widest = 0.0, 0.0
    for m0, n, t, cond in ref:
        bound = R.time_bound(n, cond)
        share = max(share, abs(T[m0] / t - 1.0) / bound)
        widest = max(widest, bound)
    assert share <= 1.0, (name, share)
    sel = R.select([v[2] for v in ref])
    for k in range(3):
        if not ref:
            assert math.isnan(out[k]), name
        else:                                                       # a rank's value moves by at most the largest move of any element
            assert abs(out[k] / sel[k] - 1.0) <= widest, (name, k, out[k], sel[k])
            assert out[k] in T[starts], name                        # and it is one of the regions' own times: the select is exact
    if ref:
        order = np.sort(T[starts])
        assert [out[0], out[1], out[2]] == [order[(len(ref) - 1) // 2], order[(len(ref) - 1) // 4], order[3 * (len(ref) - 1) // 4]], name
    return share


# ---- 1. band energies ----------------------------------------------------------------------------------------------------------------------
def test_energies_vs_restatement(lib, condition_rows):
    """rows of 511 (no frame), 512, 513, 640, 512 + 128 * 255 (256 frames), 512 + 128 * 256 + 1 and 64 000 samples in one batch.  Every E[band][m] within
    2 eps sqrt(E Etot) + eps^2 Etot of the float64 restatement, eps = 2^-18 and Etot the frame's whole spectral energy: an fp32 transform with an fp32
    window moves the spectrum by at most eps in the 2-norm, and a band's energy by that much against its own root.  A row alone
    equals the row in a batch of five bit for bit"""
    lens = [511, 512, 513, 640, 512 + 128 * 255, 512 + 128 * 256 + 1, 64000]
    src = condition_rows[12]                                                             # seed 2, T60 0.5 s: bursts, tails and silence
    rows = [np.ascontiguousarray(src[3000 + 17 * i:3000 + 17 * i + n]) for i, n in enumerate(lens)]
    got, frames = run_energies(lib, rows)
    worst = 0.0
    for b, r in enumerate(rows):
        M = int(frames[b])
        if M == 0:
            continue
        want, tot = R.energies(r.astype(np.float64))
        bound = 2.0 * EPS_FFT * np.sqrt(want * tot[None, :]) + EPS_FFT ** 2 * tot[None, :]
        err = np.abs(got[b, :, :M] - want)
        share = float((err / bound).max())
        print(f"energies: {len(r):6d} samples {M:4d} frames: largest error / bound {share:.4f}")
        worst = max(worst, share)
        assert np.all(err <= bound), (len(r), share)
    print(f"energies: largest share of the fp32-transform bound {worst:.4f}")
    assert 0.0 < worst <= 1.0
    five, f5 = run_energies(lib, [rows[3], rows[6], rows[1], rows[5], rows[4]], extra=7)
    for b5, b in enumerate((3, 6, 1, 5, 4)):
        M = int(frames[b])
        assert np.array_equal(five[b5, :, :M].view(np.uint64), got[b, :, :M].view(np.uint64)), b
        alone, _ = run_energies(lib, [rows[b]], extra=0)
        assert np.array_equal(alone[0, :, :M].view(np.uint64), got[b, :, :M].view(np.uint64)), b


def test_energies_of_a_sinusoid_land_in_its_band(lib):
    """1 kHz lies in the 1 kHz octave and in the broadband range and nowhere else: the other octaves hold leakage only"""
    n = np.arange(4096)
    got, frames = run_energies(lib, [np.sin(2.0 * np.pi * 1000.0 * n / 16000.0).astype(np.float32)])
    e = got[0, :, :int(frames[0])].mean(axis=1)
    assert e[4] > 0.999 * e[0] and e[0] > 0 and all(e[k] < 1e-4 * e[4] for k in (1, 2, 3, 5, 6))


# ---- 2. regions and select on crafted energies ---------------------------------------------------------------------------------------------
def test_regions_and_select_on_crafted_energies(lib):
    """the crafted cases (ties, a run to the last frame, rows of tile - 1, tile, tile + 1 frames, falls across and next to the tile boundary, the whole
    row -- short, and longer than the LDS window --, M in {0, 4, 5, 10, 11}, all-zero, constant, never 10 dB, the floor, a drop exactly on S[m0] q,
    1 to 4 regions) in one batch per q, the same doubles on both sides"""
    tile = lib.buddy_decay_regions_tile()
    cases = R.crafted_cases(tile)
    worst = 0.0
    for q in sorted({c[2] for c in cases}):
        part = [c for c in cases if c[2] == q]
        got = run_regions(lib, [c[1][None, :] for c in part], q)
        for (name, E, _, want), g in zip(part, got):
            share = check_band(name, (g[0][0], g[1][0], g[2][0], g[3][0]), E, q, want=want)
            n = int(g[3][0])
            assert D.flag_word(n, len(E), False, 6) == R.flag_word(n, len(E), False)
            print(f"crafted: {name:34s} M {len(E):4d} regions {n} t60 {g[2][0][0]:.6f} share of the bound {share:.4f}")
            worst = max(worst, share)
    print(f"regions on crafted energies: largest share of the double-sum bound {worst:.4f}")
    # two bands per row, the second the first doubled (exact): the same regions and, S[m0 + j] / S[m0] being the same doubles, the same bits
    pick = [c for c in cases if c[2] != 0.125][:12]
    two = run_regions(lib, [np.stack([c[1], 2.0 * c[1]]) for c in pick], pick[0][2], nb=2)
    for c, g in zip(pick, two):
        assert np.array_equal(g[0][0].view(np.uint64), g[0][1].view(np.uint64)) and np.array_equal(g[1][0], g[1][1]) and g[3][0] == g[3][1], c[0]
        assert np.array_equal(g[2][0].view(np.uint64), g[2][1].view(np.uint64)), c[0]
    # a row alone equals the row in its batch
    i = [c[0] for c in cases].index("a long fall from the second tile")
    alone = run_regions(lib, [cases[i][1][None, :]], cases[i][2], extra=0)[0]
    batch = run_regions(lib, [c[1][None, :] for c in cases if c[2] == cases[i][2]], cases[i][2])[[c[0] for c in cases if c[2] == cases[i][2]].index(cases[i][0])]
    assert np.array_equal(alone[0].view(np.uint64), batch[0].view(np.uint64)) and np.array_equal(alone[2].view(np.uint64), batch[2].view(np.uint64))


def test_lmin_and_floor_parameters(lib):
    """lmin = 7 drops the region of six frames that lmin = 6 keeps; a floor of -20 dB cuts a fall of 3 dB per frame after six steps"""
    E = R.energies_for(np.concatenate([np.full(3, 2.0 ** 40), R.fall(2.0 ** 40, 6, 3.0)[1:], np.full(3, 2.0 ** 40)]))
    for lmin, n in ((6, 1), (7, 0)):
        g = run_regions(lib, [E[None, :]], 0.1, lmin=lmin)[0]
        check_band(f"lmin {lmin}", (g[0][0], g[1][0], g[2][0], g[3][0]), E, 0.1, lmin=lmin)
        assert int(g[3][0]) == n
    E = R.energies_for(np.concatenate([np.full(3, 2.0 ** 40), R.fall(2.0 ** 40, 20, 3.0)[1:], np.full(3, 2.0 ** 40)]))
    g = run_regions(lib, [E[None, :]], 0.1, floor_rel=0.01)[0]
    check_band("floor -20 dB", (g[0][0], g[1][0], g[2][0], g[3][0]), E, 0.1, floor_rel=0.01, want=[(2, 7)])


# ---- 3. the chain, and the functional condition --------------------------------------------------------------------------------------------
def _check_chain(lib, rows, fs, res, tag):
    """steps 2-5 of the restatement on the library's OWN energies reproduce ``res`` (a ``decay_times`` result of the same rows) as in the regions
    group, and the public call equals the three entries run by hand bit for bit.  ``rows``: the rows at 16 kHz"""
    E, frames = run_energies(lib, rows, fs=fs)
    _, _, above = D.bin_ranges(fs)
    got = run_regions(lib, [E[b, :, :int(frames[b])] for b in range(len(rows))], 10.0 ** -1.0, nb=NB)
    worst = 0.0
    for b in range(len(rows)):
        M = int(frames[b])
        assert int(res.frames[b]) == M
        for k in range(NB):
            worst = max(worst, check_band(f"{tag} row {b} band {k}", (got[b][0][k], got[b][1][k], got[b][2][k], got[b][3][k]), E[b, k, :M], 10.0 ** -1.0))
            assert int(res.regions[b, k]) == int(got[b][3][k]) and int(res.flags[b, k]) == R.flag_word(int(got[b][3][k]), M, above[k])
            for v, w in ((res.t60, 0), (res.q1, 1), (res.q3, 2)):
                assert np.array_equal(np.float64(v[b, k]).view(np.uint64), got[b][2][k, w].view(np.uint64)), (tag, b, k, w)
    print(f"chain {tag}: largest share of the double-sum bound {worst:.4f}")
    return worst


def test_functional_condition_and_chain(lib, condition_rows):
    """gated bursts through exponentially decaying responses of 0.2 .. 1.0 s, seeds 0..5, as one ragged batch of 36 rows: the broadband decay time
    within 15 % of the nominal one from at least 6 regions; the dry sources read below 0.2 s.  tests/test_decay_host.py shows the restatement alone
    inside the same condition.  Then the chain on the library's own energies for one seed's rows"""
    lens = [len(r) for r in condition_rows]
    res = D.decay_times(padded(condition_rows, max(lens) + 3), 16000, lens=lens)
    assert res.t60.shape == (36, 7) and res.t60.dtype == torch.float64 and res.samples.tolist() == lens
    ok, i = True, 0
    for seed in range(6):
        for t60 in NOMINAL:
            t, n = float(res.t60[i, 0]), int(res.regions[i, 0])
            print(f"condition: seed {seed} T60 {t60:.1f}: {t:.4f} s ({100.0 * (t / t60 - 1.0):+6.2f} %) from {n:2d} regions; octaves " +
                  " ".join(f"{float(v):.3f}" for v in res.t60[i, 1:]))
            ok = ok and abs(t / t60 - 1.0) <= 0.15 and n >= 6 and int(res.flags[i, 0]) == D.DEFINED
            i += 1
    for seed in range(6):
        t = float(res.t60[30 + seed, 0])
        print(f"condition: seed {seed} dry: {t:.4f} s from {int(res.regions[30 + seed, 0])} regions")
        ok = ok and t < 0.2
    assert ok
    assert bool(torch.all(res.q1[:, 0] <= res.t60[:, 0])) and bool(torch.all(res.t60[:, 0] <= res.q3[:, 0]))
    part = [0, 2, 4, 30]                                                                 # seed 0 at 0.2, 0.5 and 1.0 s and dry
    sub = D.decay_times(padded([condition_rows[i] for i in part], max(lens) + 1), 16000, lens=[lens[i] for i in part])
    for b, i in enumerate(part):                                                         # a row's result does not depend on its batch
        assert np.array_equal(sub.t60[b].numpy().view(np.uint64), res.t60[i].numpy().view(np.uint64)) and torch.equal(sub.regions[b], res.regions[i])
    _check_chain(lib, [condition_rows[i] for i in part], 16000, sub, "16 kHz")


def test_short_silent_and_bad_calls(lib):
    x = padded([np.zeros(16000, np.float32), np.ones(1663, np.float32), np.ones(400, np.float32)], 16000, fill=0.0)
    res = D.decay_times(x, 16000, lens=[16000, 1663, 400])
    assert res.frames.tolist() == [122, 9, 0] and bool(torch.isnan(res.t60).all()) and int(res.regions.sum()) == 0
    assert res.flags[0].tolist() == [D.FEW] * 7 and res.flags[1].tolist() == [D.FEW | D.SHORT] * 7 and res.flags[2].tolist() == [D.FEW | D.SHORT] * 7
    for bad in (7999, 16000.5):
        with pytest.raises(ValueError):
            D.decay_times(x, bad)
    for kw in (dict(drop_db=0.0), dict(floor_db=0.0), dict(lmin=1)):
        with pytest.raises(ValueError):
            D.decay_times(x, 16000, **kw)


def test_entries_refuse_bad_arguments(lib):
    """BUDDY_ERR_ARG with nothing launched (the outputs keep their sentinel)"""
    st = _lib.stream_ptr()
    x, lens = padded([np.ones(5000, np.float32)], 5000), dev_i32([5000])
    M = R.frames_of(5000)
    lo, hi, _ = D.bin_ranges(16000)
    E, fr = guarded(NB * M, torch.float64, SENTINEL), guarded(1, torch.int32, -77)
    args = lambda **kw: [kw.get("x", _lib.ptr(x)), lens.data_ptr(), kw.get("B", 1), kw.get("ld", 5000), kw.get("lo", c_ints(lo)), kw.get("hi", c_ints(hi)),
                         kw.get("NB", NB), E.data_ptr(), kw.get("ldm", M), fr.data_ptr(), st]
    for kw in (dict(x=None), dict(B=0), dict(ld=4999), dict(ldm=M - 1), dict(NB=0), dict(NB=9), dict(hi=c_ints([258] + hi[1:])), dict(lo=c_ints([-1] + lo[1:])),
               dict(lo=c_ints([183] + lo[1:]))):
        assert lib.buddy_decay_energies(*args(**kw)) == 2, kw
    frames = dev_i32([M])
    T, ln = guarded(NB * M, torch.float64, SENTINEL), guarded(NB * M, torch.int32, -77)
    rargs = lambda **kw: [kw.get("E", E.data_ptr()), frames.data_ptr(), kw.get("B", 1), kw.get("NB", NB), kw.get("ldm", M), kw.get("K", 5), kw.get("lmin", 6),
                          kw.get("q", 0.1), kw.get("floor", 1e-6), T.data_ptr(), ln.data_ptr(), st]
    for kw in (dict(E=None), dict(B=0), dict(NB=9), dict(ldm=M - 1), dict(K=0), dict(K=9), dict(lmin=1), dict(q=0.0), dict(q=1.5), dict(q=float("nan")),
               dict(floor=-0.1), dict(floor=1.0)):
        assert lib.buddy_decay_regions(*rargs(**kw)) == 2, kw
    out, cnt = guarded(NB * 3, torch.float64, SENTINEL), guarded(NB, torch.int32, -77)
    for kw in (dict(T=None), dict(B=0), dict(NB=0), dict(ldm=M - 1)):
        rc = lib.buddy_decay_select(kw.get("T", T.data_ptr()), frames.data_ptr(), kw.get("B", 1), kw.get("NB", NB), kw.get("ldm", M), out.data_ptr(), cnt.data_ptr(), st)
        assert rc == 2, kw
    torch.cuda.synchronize()
    for buf, n, fill in ((E, NB * M, SENTINEL), (fr, 1, -77), (T, NB * M, SENTINEL), (ln, NB * M, -77), (out, NB * 3, SENTINEL), (cnt, NB, -77)):
        assert np.all(split(buf, n, fill) == fill)


# ---- 4. other rates ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [8000, 22050, 48000])
def test_other_rates_through_the_resampler(lib, condition_rows, fs):
    """the call at another rate is the project's resampler to 16 kHz and then the chain with that rate's bands: at 8 kHz the 4 kHz octave is flagged
    ABOVE_RATE and undefined and the broadband range ends at 3.6 kHz; the energies hold the fp32 bound against the restatement on the resampled rows"""
    up, down = (fs // 50, 320) if fs != 22050 else (441, 320)
    rows = [signal.resample_poly(condition_rows[i].astype(np.float64)[:n16], up, down).astype(np.float32) for i, n16 in ((12, 64000), (3, 48011))]
    lens = [len(r) for r in rows]
    x = padded(rows, max(lens) + 2, fill=0.0)
    res = D.decay_times(x, fs, lens=lens)
    assert res.samples.tolist() == lens
    x16 = RS.resample(x, fs, 16000).cpu().numpy()
    u, d = RS.ratio(fs, 16000)
    rows16 = [np.ascontiguousarray(x16[b, :RS.out_length(n, u, d)]) for b, n in enumerate(lens)]
    _check_chain(lib, rows16, fs, res, f"{fs} Hz")
    E, frames = run_energies(lib, rows16, fs=fs)
    for b, r in enumerate(rows16):
        want, tot = R.energies(r.astype(np.float64), fs)
        bound = 2.0 * EPS_FFT * np.sqrt(want * tot[None, :]) + EPS_FFT ** 2 * tot[None, :]
        assert np.all(np.abs(E[b, :, :int(frames[b])] - want) <= bound), b
    print(f"{fs} Hz: broadband {res.t60[:, 0].tolist()} regions {res.regions[:, 0].tolist()} flags {res.flags.tolist()}")
    if fs == 8000:
        assert res.flags[:, 6].tolist() == [D.FEW | D.ABOVE_RATE] * 2 and bool(torch.isnan(res.t60[:, 6]).all()) and res.regions[:, 6].tolist() == [0, 0]
        assert np.all(E[:, 6, :int(frames.min())] == 0.0)
    else:
        assert not bool((res.flags & D.ABOVE_RATE).any())
    assert bool((res.flags[:, 0] & D.DEFINED).all()) and int(res.regions[:, 0].min()) >= 3


# ---- 5. the tester and the tool ------------------------------------------------------------------------------------------------------------
SMALL = ["tester.sampling_params.T=3", "tester.posterior_sampling.blind_hp.op_updates_per_step=2",
         "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "network.nf=32", "tester.noise.generator=philox", "tester.sub_batches=1",
         "+gpu=0", "tester.overriden_name=run", "+allow_random_init=true"]
BANDS = ["", "_125", "_250", "_500", "_1000", "_2000", "_4000"]
COLUMNS = (["file", "samples_in", "samples_out", "frames_in", "frames_out"] + [f"t60{b}_{s}" for b in BANDS for s in ("in", "out", "delta")]
           + [f"{c}{b}_{s}" for c in ("regions", "spread", "flags") for b in BANDS for s in ("in", "out")])
CLEAN = [f"t60{b}_clean" for b in BANDS] + [f"regions{b}_clean" for b in BANDS]


def _tree(base):
    out = {}
    for dp, _, fs in os.walk(base):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, base)] = open(p, "rb").read()
    return out


def _same(a, b):
    return (isinstance(a, float) and math.isnan(a) and math.isnan(b)) or a == b


def _recording(u, n, fs):
    """bursts in a room at rate ``fs``, scaled like a recording"""
    y = R.reverberant(u, 0.3)[4000:]
    y = signal.resample_poly(y, fs // 16000, 1)[:n] if fs != 16000 else y[:n]
    return (0.3 * y / np.abs(y).max()).astype(np.float32)


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
        cols[s] = D.score_signals(sigs, "cuda")
    return names, cols


def _check_rows(rows, names, cols, clean=False):
    by = {r["file"]: r for r in rows}
    assert sorted(by) == names and len(rows) == len(names)                                # one line per written wav
    for b, n in enumerate(names):
        r = by[n]
        for tag, s in (("in", "degraded"), ("out", "reconstructed")):
            c = cols[s][b]
            assert r[f"frames_{tag}"] == c["frames"] and r[f"samples_{tag}"] == c["samples"], (n, tag)
            for k, band in enumerate(BANDS):
                assert _same(r[f"t60{band}_{tag}"], c["t60"][k]) and r[f"regions{band}_{tag}"] == c["regions"][k] and r[f"flags{band}_{tag}"] == c["flags"][k], (n, tag, k)
                assert _same(r[f"spread{band}_{tag}"], c["q3"][k] - c["q1"][k]), (n, tag, k)
        for band in BANDS:
            assert _same(r[f"t60{band}_delta"], r[f"t60{band}_out"] - r[f"t60{band}_in"])
        if clean:
            for k, band in enumerate(BANDS):
                assert _same(r[f"t60{band}_clean"], cols["original"][b]["t60"][k]) and r[f"regions{band}_clean"] == cols["original"][b]["regions"][k]


def _check_summary(base, rows, values):
    summ = read_csv(os.path.join(base, "decay_summary.csv"))
    assert [s["value"] for s in summ] == values
    for s in summ:
        v = np.array([r[s["value"]] for r in rows])
        v = v[~np.isnan(v)]
        assert s["n"] == len(v)
        if len(v):
            assert s["mean"] == float(np.mean(v)) and s["median"] == float(np.median(v)) and s["std"] == float(np.std(v)), s


def _run_real(tmp, tag, extra):
    import test as cli
    data = os.path.join(tmp, "recordings")
    if not os.path.exists(data):
        os.makedirs(data)
        wavfile.write(os.path.join(data, "A.wav"), 48000, _recording(0, 2 * 24576 * 3 // 2, 48000))       # 1.536 s
        wavfile.write(os.path.join(data, "C.wav"), 16000, _recording(1, 27000, 16000))
    out = os.path.join(tmp, tag)
    torch.manual_seed(0)                                      # +allow_random_init draws the network from torch's generator: the same weights in both runs
    t = cli.main(["--config-name=conf_VCTK.yaml", "tester=real_dereverberation_BUDDy", *SMALL, "tester.real_recordings.chunk_seconds=1.024",
                  "tester.real_recordings.overlap_seconds=0.128", f"model_dir={out}", f"dset.test.path={data}", "+batch_size=4", *extra])
    return t, os.path.join(out, "run", "real_blind_dereverberation", "VCTK_16k_4s_time")


def test_tester_real_recordings_report_and_tool(tmp_path):
    t_on, on = _run_real(str(tmp_path), "on", ["tester.decay.use=true"])
    rows = read_csv(os.path.join(on, "decay.csv"))
    assert [r["file"] for r in rows] == [r["file"] for r in t_on.decay_report] == ["A", "C"] and list(rows[0]) == list(t_on.decay_report[0]) == COLUMNS
    names, cols = _recompute(on, ("degraded", "reconstructed"))
    _check_rows(rows, names, cols)
    by = {r["file"]: r for r in rows}
    assert (by["A"]["samples_in"], by["A"]["samples_out"], by["C"]["samples_in"], by["C"]["samples_out"]) == (24576, 73728, 27000, 27000)
    assert (by["A"]["frames_in"], by["A"]["frames_out"], by["C"]["frames_out"]) == (189, 189, 207)   # degraded/ at the model's rate, reconstructed/ at the input's
    assert by["C"]["regions_in"] >= 1 and 0.0 < by["C"]["t60_in"] < 2.0 and by["C"]["flags_in"] & D.DEFINED
    _check_summary(on, rows, [c for c in COLUMNS if c.startswith("t60")])
    _, off = _run_real(str(tmp_path), "off", [])
    tree_on, tree_off = _tree(on), _tree(off)
    assert not [f for f in tree_off if f.endswith(".csv")]
    assert sorted(set(tree_on) - set(tree_off)) == ["decay.csv", "decay_summary.csv"] and not set(tree_off) - set(tree_on)
    wavs = [f for f in tree_off if f.endswith(".wav")]
    assert len(wavs) >= 6
    for f in wavs:
        assert tree_on[f] == tree_off[f], f                    # every wav of the run is byte-identical with the report on
    # the tool, in a child process: the mode directory gives the tester's rows
    saved = open(os.path.join(on, "decay.csv")).read()
    saved_summary = open(os.path.join(on, "decay_summary.csv")).read()
    os.remove(os.path.join(on, "decay.csv")), os.remove(os.path.join(on, "decay_summary.csv"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "decay.py"), on], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "t60_out" in p.stdout
    assert open(os.path.join(on, "decay.csv")).read() == saved and open(os.path.join(on, "decay_summary.csv")).read() == saved_summary
    # in this process: a list of wavs (an int16 stereo file among them: every channel a row) and a pair of directories
    import importlib.util
    spec = importlib.util.spec_from_file_location("buddy_tools_decay", os.path.join(ROOT, "tools", "decay.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    y = _recording(2, 30000, 16000)
    st = str(tmp_path / "stereo.wav")
    pcm = np.round(np.stack([y, 0.5 * y[::-1]], axis=1) * 32767.0).astype(np.int16)
    wavfile.write(st, 16000, pcm)
    outd = str(tmp_path / "scored")
    got = tool.main([st, os.path.join(on, "degraded", "C.wav"), "--out", outd])
    assert [r["file"] for r in got] == ["stereo.ch0", "stereo.ch1", "C"] and _same(got[2]["t60_out"], by["C"]["t60_in"]) and math.isnan(got[2]["t60_in"])
    chans = D.score_signals([((pcm[:, c].astype(np.float64) / 32768.0).astype(np.float32), 16000) for c in range(2)], "cuda")
    assert _same(got[0]["t60_out"], chans[0]["t60"][0]) and _same(got[1]["t60_out"], chans[1]["t60"][0]) and got[0]["regions_out"] == chans[0]["regions"][0] >= 1
    assert [r["file"] for r in read_csv(os.path.join(outd, "decay.csv"))] == ["stereo.ch0", "stereo.ch1", "C"]
    pair = tool.main(["--input", os.path.join(on, "degraded"), "--estimate", os.path.join(on, "reconstructed"), "--out", outd])
    assert all(_same(a["t60_in"], b["t60_in"]) and _same(a["t60_out"], b["t60_out"]) and a["file"] == b["file"] for a, b in zip(pair, rows)) and len(pair) == len(rows)
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
                  "dset.test.num_examples=2", "+batch_size=2", "tester.decay.use=true"])
    base = os.path.join(out, "run", "blind_dereverberation", "VCTK_16k_4s_time")
    rows = read_csv(os.path.join(base, "decay.csv"))
    assert list(rows[0]) == COLUMNS + CLEAN == list(t.decay_report[0])
    names, cols = _recompute(base, ("degraded", "reconstructed", "original"))
    _check_rows(rows, names, cols, clean=True)
    assert all(r["samples_in"] == r["samples_out"] == 16000 and r["frames_out"] == 122 for r in rows)
    _check_summary(base, rows, [c for c in COLUMNS + CLEAN if c.startswith("t60")])
    assert sorted(f for f in os.listdir(base) if f.endswith(".csv")) == ["decay.csv", "decay_summary.csv"]      # the other report blocks stay off
