"""GPU: banded rooms (csrc/ism.hip shoebox_bands / band_combine, rooms.shoebox_rir_bands) against the float64 restatement
tests/_ism_bands_ref.py under the derived bounds

    |u_gpu[k][n] - u_ref[k][n]| <= (M[n] + 64) 2^-53 A_k[n] + 16 (N + Hw) 2^-53 G_k[n] + 2^-53 E_k[n]
    |h_gpu[n] - h_ref[n]|       <= 2^-23 |h_ref[n]| + sum_k sum_j |bank[k][j]| ub_k[n - j] + (nb Nh + 8) 2^-53 sum_k sum_j |bank[k][j] u_k[n - j]|

(section 20's bound per band without the output rounding, plus the gains' rounding E = sum (o + 24 + 8 air_k d) |A_k sinc w|; one fp32 rounding, the
band bounds pushed through sum |bank|, the double sum), then the tool tools/make_paired_set.py with and without --bands.  T = buddy_ism_tile(),
C = buddy_ism_band_list(), Tc = buddy_band_combine_tile().  Every case prints its largest deviation over the bound (profiles/ism_bands_accuracy.txt
holds them)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acoustics_ref as AR  # noqa: E402
import _ism_bands_ref as BR  # noqa: E402
import _ism_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import acoustics, rooms  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L0, S0, R0 = (4.1, 3.3, 2.7), (1.1, 0.9, 1.3), (2.9, 2.2, 1.6)
BETA2 = ((0.9, -0.7, 0.8, 0.85, -0.6, 0.75), (0.5, 0.0, 0.6, -0.4, 0.7, 0.3))          # unequal; a negative and, in band 1 only, a zero coefficient
AIR2 = (0.0, 0.02)
SENTINEL = 12345.0
RM0 = R.room(L0, S0, R0, 0.123)                                                       # the row's own coefficients are not read


@pytest.fixture(scope="module")
def lib():
    return _lib.require_gpu()


def fixed_bank(nb, Nh, seed=0):
    """an arbitrary FIR bank: the combination is checked as the plain sum it is"""
    return np.random.RandomState(1000 * seed + 10 * Nh + nb).uniform(-1.0, 1.0, (nb, Nh))


@functools.lru_cache(maxsize=None)
def _ref(rm, beta, air, fs, N, order):
    nb = len(beta) // 6
    out = BR.rir_bands(np.array(rm), np.array(beta).reshape(nb, 6), None if air is None else np.array(air), fs, N, order)
    for a in out:
        a.setflags(write=False)
    return out


def ref(rm, beta, air, fs, N, order=-1):
    return _ref(tuple(float(v) for v in rm), tuple(float(v) for v in np.ravel(beta)), None if air is None else tuple(float(v) for v in air), fs, N, order)


def gpu(rm, beta, fs, N, bank, air=None, order=-1):
    rm = np.asarray(rm, dtype=np.float64).reshape(-1, 16)
    beta = np.asarray(beta, dtype=np.float64).reshape(rm.shape[0], -1, 6)
    h, flags, u = rooms.shoebox_rir_bands(rm, beta, fs, N, bank, air=None if air is None else np.asarray(air, dtype=np.float64), max_order=order, return_bands=True)
    return h.cpu().numpy(), flags.numpy(), u.cpu().numpy()


def over(err, bound):
    """the largest err / bound; where the bound is zero the error must be"""
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


def check(tag, rm, beta, air, fs, N, bank, order=-1):
    """one banded room against the restatement: the band responses and the combined one; returns (h_gpu, u_gpu, u_ref, M, h_ref, h's bound)"""
    u, M, A, G, E = ref(rm, beta, air, fs, N, order)
    ub = BR.band_bound(N, M, A, G, E)
    want, S = BR.combine(u, bank)
    hb = BR.h_bound(want, bank, ub, S)
    h, flags, ug = gpu(rm, beta, fs, N, bank, air, order)
    assert flags.tolist() == [1] and h.shape == (1, N) and ug.shape == (1,) + u.shape and h.dtype == np.float32 and ug.dtype == np.float64
    ru, rh = over(np.abs(ug[0] - u), ub), over(np.abs(h[0].astype(np.float64) - want), hb)
    print(f"bands {tag}: N {N} fs {fs} nb {len(u)} Nh {bank.shape[1]} order {order} images/sample <= {int(M.max())} peak {np.abs(want).max():.3e} "
          f"max err/bound u {ru:.3f} h {rh:.3f}")
    assert ru <= 1.0 and rh <= 1.0, (tag, ru, rh)
    return h[0], ug[0], u, M, want, hb


def test_lengths_around_the_tile(lib):
    T = lib.buddy_ism_tile()
    bank = rooms.octave_bank(8000, (500, 1000), 31)
    for N in (1, T - 1, T, T + 1, 2 * T + 3):
        h, ug, u, *_ = check(f"length {N}", RM0, BETA2, AIR2, 8000, N, bank)
        assert N == 1 or (np.abs(ug[0]).max() > 0.02 and np.abs(ug[1]).max() > 0.02)     # the direct sound peaks at sample 92, also in the band with a zero wall
    assert not gpu(RM0, BETA2, 8000, 1, bank, AIR2)[2].any()                            # sample 0 lies Hw before time 0: no image reaches it


@pytest.mark.parametrize("nb", [1, 2, 7, 8])
def test_band_counts(lib, nb):
    assert nb <= lib.buddy_ism_max_bands() == 8
    rs = np.random.RandomState(nb)
    beta, air = rs.uniform(-0.95, 0.95, (nb, 6)), rs.uniform(0.0, 0.05, nb)
    h, ug, u, *_ = check(f"nb {nb}", RM0, beta, air, 8000, lib.buddy_ism_tile() + 1, fixed_bank(nb, 5))
    assert all(np.abs(ug[k]).max() > 0.02 for k in range(nb)) and (nb == 1 or np.abs(ug[0] - ug[nb - 1]).max() > 1e-4)


def test_filter_lengths(lib):
    T, Tc = lib.buddy_ism_tile(), lib.buddy_band_combine_tile()
    for Nh in (1, 3, 2 * Tc + 1):
        check(f"Nh {Nh}", RM0, BETA2, AIR2, 8000, 2 * max(T, Tc) + 3, fixed_bank(2, Nh))


def test_combination_alone_around_its_tile(lib):
    """random double inputs in a padded stride against np.convolve in float64; the bound is the fp32 rounding plus the double sum's"""
    Tc = lib.buddy_band_combine_tile()
    B, nb = 2, 3
    rs = np.random.RandomState(7)
    for N in (1, Tc - 1, Tc, Tc + 1, 2 * Tc + 3):
        for Nh in (1, 9, 2 * Tc + 1):
            ldu, ldh = N + 5, N + 3
            u, bank = rs.standard_normal((B, nb, ldu)), rs.standard_normal((nb, Nh))
            ut, kt = torch.from_numpy(u).cuda(), torch.from_numpy(bank).cuda()
            h = torch.full((B * ldh + 16,), SENTINEL, dtype=torch.float32, device="cuda")
            _lib.check(lib.buddy_band_combine(ut.data_ptr(), B, nb, ldu, N, kt.data_ptr(), Nh, h.data_ptr(), ldh, _lib.stream_ptr()))
            hh = h.cpu().numpy()
            got = hh[:B * ldh].reshape(B, ldh)
            assert np.all(got[:, N:] == SENTINEL) and np.all(hh[B * ldh:] == SENTINEL)
            worst = 0.0
            for b in range(B):
                want, S = BR.combine(u[b, :, :N], bank)
                worst = max(worst, over(np.abs(got[b, :N].astype(np.float64) - want), 2.0 ** -23 * np.abs(want) + (nb * Nh + 8) * 2.0 ** -53 * S))
            print(f"bands combine alone: N {N} Nh {Nh} max err/bound {worst:.3f}")
            assert worst <= 1.0, (N, Nh, worst)


def test_one_band_is_the_broadband_simulator(lib):
    """nb = 1 with the bank [1]: within the sum of both kernels' bounds of buddy_shoebox_rir's response of the same room"""
    N = 700
    rm = R.room(L0, S0, R0, BETA2[0])
    h, ug, u, M, want, hb = check("one band", rm, BETA2[:1], None, 8000, N, np.ones((1, 1)))
    broad = rooms.shoebox_rir(rm[None], 8000, N)[0][0].cpu().numpy().astype(np.float64)
    rb = R.rir(rm, 8000, N)
    assert np.abs(rb[0] - want).max() <= 1e-16
    ratio = over(np.abs(h.astype(np.float64) - broad), R.bound(*rb) + hb)
    print(f"bands one band against shoebox_rir: max |h - h'| / (sum of bounds) {ratio:.3f}")
    assert ratio <= 1.0


def test_equal_bands_are_the_broadband_room_delayed(lib):
    N, fs = 700, 16000
    cs = rooms.BAND_CENTRES
    bank = rooms.octave_bank(fs, cs, 127)
    P = 63
    beta = np.array([BETA2[0]] * len(cs))
    h, ug, u, M, want, hb = check("equal bands", RM0, beta, None, fs, N, bank)
    broad = R.rir(R.room(L0, S0, R0, BETA2[0]), fs, N)[0]
    delayed = np.concatenate([np.zeros(P), broad[:N - P]])
    S = BR.combine(u, bank)[1]
    slack = (bank.size + 8) * 2.0 ** -53 * S                                            # the restatement's own double sum
    assert np.all(np.abs(want - delayed) <= slack) and np.abs(delayed).max() > 0.02
    ratio = over(np.abs(h.astype(np.float64) - delayed), hb + slack)
    print(f"bands equal bands against the delayed broadband room: max err/bound {ratio:.3f}")
    assert ratio <= 1.0


def test_lossless_cube_spills_the_list(lib):
    """beta = +-1 in both bands: the images of one sample alone outnumber the LDS chunk of the banded list"""
    rm = R.room((2.5, 2.5, 2.5), (0.7, 1.1, 0.9), (1.9, 1.4, 1.6), 0.5)
    beta = ((1.0, -1.0, 1.0, 1.0, -1.0, 1.0), (-1.0, 1.0, 1.0, -1.0, 1.0, 1.0))
    h, ug, u, M, *_ = check("lossless cube", rm, beta, None, 8000, 640, fixed_bank(2, 3))
    assert M.max() > lib.buddy_ism_band_list(), (int(M.max()), lib.buddy_ism_band_list())


@pytest.mark.parametrize("peak", [-0.4, 0.4])
def test_direct_sound_on_a_tile_boundary(lib, peak):
    T = lib.buddy_ism_tile()
    d = (T + peak - R.HW) * 343.0 / 8000.0
    rm = R.room((d + 2.0, 5.0, 3.0), (1.0, 2.0, 1.5), (1.0 + d, 2.0, 1.5), 0.5)
    beta = ((0.8, 0.6, 0.7, -0.5, 0.9, 0.4), (0.3, 0.0, -0.2, 0.5, 0.1, 0.6))
    h, ug, *_ = check(f"tile boundary {peak:+.1f}", rm, beta, AIR2, 8000, 2 * T + 88, fixed_bank(2, 3))
    for k in range(2):
        assert max(abs(ug[k, T - 1]), abs(ug[k, T])) > 0.6 * math.exp(-AIR2[k] * d) / (4.0 * np.pi * d) and ug[k, T - 2 * R.HW] == 0.0


@pytest.mark.parametrize("order", [0, 1, 2])
def test_order_caps(lib, order):
    N = 700
    bank = fixed_bank(2, 5)
    h, ug, u, M, want, hb = check(f"order {order}", RM0, BETA2, AIR2, 8000, N, bank, order)
    assert M.max() <= (1, 7, 25)[order]
    if order == 0:            # the closed form: per band one kernel of amplitude exp(-air_k d) / (4 pi d), combined by the bank
        d = math.dist(S0, R0)
        x = np.arange(N) - R.HW - d * 8000 / 343.0
        kern = np.where(np.abs(x) < R.HW, np.sinc(x) * 0.5 * (1.0 + np.cos(np.pi * x / R.HW)), 0.0) / (4.0 * np.pi * d)
        free = np.stack([math.exp(-a * d) * kern for a in AIR2])
        assert np.abs(u - free).max() <= 1e-17
        ub = BR.band_bound(N, *ref(RM0, BETA2, AIR2, 8000, N, 0)[1:])
        closed, S = BR.combine(free, bank)
        ratio = max(over(np.abs(ug - free), ub + 1e-17), over(np.abs(h.astype(np.float64) - closed), hb + 5.0 * 1e-17))
        print(f"bands order 0 against the closed form: max err/bound {ratio:.3f}")
        assert ratio <= 1.0


def test_batches_runs_and_invalid_rows(lib):
    """a row's responses are bit for bit the ones it has alone, in any batch and any run; an invalid row is zeros with flag 0 and disturbs nobody"""
    N = 700
    bank = fixed_bank(2, 5)
    rs = [RM0, R.room((12.0, 9.0, 4.0), (2.0, 3.0, 1.0), (10.0, 7.5, 3.2), 0.7), R.room((1.6, 1.2, 2.0), (0.4, 0.5, 0.6), (1.1, 0.8, 1.5), 0.1)]
    betas = [np.array(BETA2), np.array([[0.7] * 6, [0.4] * 6]), np.array([(0.5, 0.6, -0.4, 0.7, 0.3, 0.6), (0.2, -0.3, 0.4, 0.1, 0.0, 0.5)])]
    airs = np.array([AIR2, (0.01, 0.03), (0.0, 0.0)])
    solo = [gpu(r, bt, 8000, N, bank, a[None]) for r, bt, a in zip(rs, betas, airs)]
    h, flags, u = gpu(np.stack(rs), np.stack(betas), 8000, N, bank, airs)
    assert flags.tolist() == [1, 1, 1]
    for b in range(3):
        assert np.array_equal(h[b], solo[b][0][0]) and np.array_equal(u[b], solo[b][2][0]) and np.abs(h[b]).max() > 0
    again = gpu(np.stack(rs), np.stack(betas), 8000, N, bank, airs)
    assert np.array_equal(h, again[0]) and np.array_equal(u, again[2])
    # the row's own coefficients are not read: garbage there changes nothing
    own = rs[0].copy()
    own[9:15] = (float("nan"), 7.0, -3.0, float("inf"), 0.0, 1.5)
    ho, fo, uo = gpu(own, betas[0], 8000, N, bank, airs[:1])
    assert fo.tolist() == [1] and np.array_equal(ho[0], h[0]) and np.array_equal(uo[0], u[0])
    nan, inf = float("nan"), float("inf")
    bad = []                                                            # (row, beta, air) of one invalid kind each
    def kind(row=None, beta=None, air=None):
        r, bt, a = rs[0].copy(), betas[0].copy(), airs[0].copy()
        for i, v in (row or {}).items():
            r[i] = v
        for i, v in (beta or {}).items():
            bt[i] = v
        for i, v in (air or {}).items():
            a[i] = v
        bad.append((r, bt, a))
    kind(row={1: 0.0})                                                  # Ly = 0
    kind(row={3: L0[0]})                                                # the source on a wall
    kind(row={8: -0.1})                                                 # the receiver outside
    kind(row={15: 0.0})                                                 # c = 0
    kind(row={6: S0[0] + 0.005, 7: S0[1], 8: S0[2]})                    # |s - r| < 0.01 m
    kind(row={4: nan})
    kind(row={0: inf})
    kind(beta={(1, 3): 1.0 + 1e-12})                                    # |beta[k][w]| > 1
    kind(beta={(0, 5): -1.0 - 1e-12})
    kind(beta={(1, 0): nan})
    kind(beta={(0, 2): inf})
    kind(air={1: -1e-12})                                               # air[k] < 0
    kind(air={0: nan})
    kind(air={1: inf})
    for i, (r, bt, a) in enumerate(bad):
        hm, fm, um = gpu(np.stack([rs[1], r, rs[2]]), np.stack([betas[1], bt, betas[2]]), 8000, N, bank, np.stack([airs[1], a, airs[2]]))
        assert fm.tolist() == [1, 0, 1], i
        assert not hm[1].any() and not um[1].any() and np.array_equal(hm[0], h[1]) and np.array_equal(hm[2], h[2]), i
        assert np.array_equal(um[0], u[1]) and np.array_equal(um[2], u[2]), i


def test_padded_strides_keep_their_canaries(lib):
    T = lib.buddy_ism_tile()
    N, B, nb, Nh = T + 5, 2, 2, 5
    ldu, ldh = N + 11, N + 7
    bank = fixed_bank(nb, Nh)
    rm = np.stack([RM0, R.room(L0, R0, S0, 0.5)])
    beta = np.stack([np.array(BETA2), np.array(BETA2)[::-1]])
    air = np.array([AIR2, AIR2])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rt, bt, at, kt = dev(rm), dev(beta), dev(air), dev(bank)
    u = torch.full((B * nb * ldu + 64,), SENTINEL, dtype=torch.float64, device="cuda")
    h = torch.full((B * ldh + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    flags = torch.full((B + 8,), 77, dtype=torch.int32, device="cuda")
    st = _lib.stream_ptr()
    _lib.check(lib.buddy_shoebox_bands(rt.data_ptr(), bt.data_ptr(), at.data_ptr(), B, nb, 8000, N, -1, u.data_ptr(), ldu, flags.data_ptr(), st))
    _lib.check(lib.buddy_band_combine(u.data_ptr(), B, nb, ldu, N, kt.data_ptr(), Nh, h.data_ptr(), ldh, st))
    uu, hh = u.cpu().numpy(), h.cpu().numpy()
    urows, hrows = uu[:B * nb * ldu].reshape(B, nb, ldu), hh[:B * ldh].reshape(B, ldh)
    assert np.all(urows[:, :, N:] == SENTINEL) and np.all(uu[B * nb * ldu:] == SENTINEL)
    assert np.all(hrows[:, N:] == SENTINEL) and np.all(hh[B * ldh:] == SENTINEL) and flags.cpu().tolist() == [1, 1] + [77] * 8
    hp, _, up = gpu(rm, beta, 8000, N, bank, air)
    assert np.array_equal(urows[:, :, :N], up) and np.array_equal(hrows[:, :N], hp)
    # an invalid last row writes its zeros and nothing behind them
    rm[1, 2] = -1.0
    u.fill_(SENTINEL)
    _lib.check(lib.buddy_shoebox_bands(dev(rm).data_ptr(), bt.data_ptr(), None, B, nb, 8000, N, -1, u.data_ptr(), ldu, flags.data_ptr(), st))
    uu = u.cpu().numpy()
    urows = uu[:B * nb * ldu].reshape(B, nb, ldu)
    assert not urows[1, :, :N].any() and np.all(urows[:, :, N:] == SENTINEL) and np.all(uu[B * nb * ldu:] == SENTINEL) and flags.cpu().tolist()[:3] == [1, 0, 77]


def test_high_band_decays_faster(lib):
    """physical sanity, no CPU reference: 5 x 4 x 3 m, 0.5 s at 16 kHz, the 4 kHz band's coefficients well below the 500 Hz band's (the values
    tests/test_rooms_bands_host.py first holds on the restatement at a quarter of the length): the measured T30 is shorter at 4 kHz, both valid"""
    dims, fs = (5.0, 4.0, 3.0), 16000
    cs = (500, 1000, 2000, 4000)
    beta = rooms.eyring_beta_bands(dims, (0.35, 0.35, 0.15, 0.15))
    bank = rooms.octave_bank(fs, cs)
    rm = R.room(dims, (1.2, 1.1, 1.4), (3.9, 2.8, 1.7), 0.5)
    h, flags = rooms.shoebox_rir_bands(rm[None], beta[None], fs, 8000 + (bank.shape[1] - 1) // 2, bank)
    ac = acoustics.rir_acoustics(h, fs, centres=cs)
    lo, hi = ac.bands.index(500.0), ac.bands.index(4000.0)
    t_lo, t_hi = float(ac.values[0, lo, 2]), float(ac.values[0, hi, 2])
    print(f"bands physical: T30 at 500 Hz {t_lo:.3f} s, at 4 kHz {t_hi:.3f} s, flags {int(ac.flags[0, lo]):#x} {int(ac.flags[0, hi]):#x}")
    both = (1 << 2) | (1 << (acoustics.FIT_VALID_BIT + 2))
    assert flags.tolist() == [1] and int(ac.flags[0, lo]) & both == both and int(ac.flags[0, hi]) & both == both
    assert t_hi < t_lo


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------------
def _clean_folder(base, n=16000):
    from buddy_amd.synth import synth_clean
    d = os.path.join(base, "p001")
    os.makedirs(d, exist_ok=True)
    for u in range(2):
        wavfile.write(os.path.join(d, f"p001_{u:03d}.wav"), 16000, synth_clean(u, n).astype(np.float32))
    return base


def _tree(base):
    out = {}
    for dp, _, fs in os.walk(base):
        for f in fs:
            p = os.path.join(dp, f)
            out[os.path.relpath(p, base)] = open(p, "rb").read()
    return out


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_paired_set
    return make_paired_set


def test_tool_with_bands_end_to_end(tmp_path):
    from buddy_amd.datasets.vctk import VCTKTestPaired
    tool = _tool()
    clean = _clean_folder(str(tmp_path / "speech"))
    out, out2 = str(tmp_path / "set"), str(tmp_path / "set2")
    air = [0.0, 0.0, 0.001, 0.002, 0.004, 0.008]
    args = ["--clean", clean, "--seed", "3", "--t60", "0.2", "0.25", "--bands", "--t60-slope", "0.1", "0.2", "--air"] + [str(v) for v in air]
    tool.main(args + ["--out", out])
    cs = rooms.BAND_CENTRES
    names = ["p001/p001_000", "p001/p001_001"]
    drawn, beta, t60s = rooms.draw_band_rooms(names, 3, cs, t60=(0.2, 0.25), slope=(0.1, 0.2))
    bank = rooms.octave_bank(16000, cs)
    P = (bank.shape[1] - 1) // 2
    rows = AR.read_csv(os.path.join(out, "rooms.csv"))
    assert [r["file"] for r in rows] == names
    ds = VCTKTestPaired(path=out, num_examples=2)
    for u, (x, rir, fname) in enumerate(ds):
        assert fname == f"p001_{u:03d}.wav" and len(x) == 16000
        n = int(round(1.5 * t60s[u].max() * 16000)) + P
        h = rooms.shoebox_rir_bands(drawn[u:u + 1], beta[u:u + 1], 16000, n, bank, air=np.array(air))[0][0].cpu().numpy().astype(np.float64)
        want = h[np.argmax(np.abs(h)):]
        assert np.array_equal(rir, want / np.abs(want).max()) and len(rir) > n // 2
        r = rows[u]
        assert r["n"] == n and r["flag"] == 1 and r["fs"] == 16000 and [r[c] for c in rooms.COLUMNS] == drawn[u].tolist()
        assert r["eyring_T60"] == r["eyring_T60_1000"] and 0.2 <= r["eyring_T60"] * (1 + 1e-12) and r["eyring_T60"] <= 0.25 * (1 + 1e-12)
        for k, f in enumerate(cs):
            assert r[f"beta_{f}"] == beta[u, k, 0] and abs(r[f"eyring_T60_{f}"] / t60s[u, k] - 1.0) < 1e-12
            bits = int(r[f"acoustics_flags_{f}"])
            assert r[f"acoustics_flags_{f}"] == bits and 0.05 < r[f"T20_{f}"] < 3.0 and bits & 0b10 == 0b10         # T20 is defined in every band
            assert (0.05 < r[f"T30_{f}"] < 3.0) if bits & 0b100 else math.isnan(r[f"T30_{f}"])
        assert r["eyring_T60_125"] > r["eyring_T60_1000"] > r["eyring_T60_4000"]
    tool.main(args + ["--out", out2])
    a, b = _tree(out), _tree(out2)
    assert sorted(a) == sorted(b) and len(a) == 5 and all(a[f] == b[f] for f in a)


def test_tool_without_bands_is_unchanged(tmp_path, monkeypatch):
    """without --bands: the files of the broadband calls, byte for byte, and no banded entry is touched"""
    tool = _tool()
    lib = _lib.require_gpu()

    def refuse(*a, **k):
        raise AssertionError("a banded entry was called without --bands")
    for name in ("buddy_shoebox_bands", "buddy_band_combine"):
        monkeypatch.setattr(lib, name, refuse)
    monkeypatch.setattr(rooms, "shoebox_rir_bands", refuse)
    monkeypatch.setattr(rooms, "draw_band_rooms", refuse)
    clean = _clean_folder(str(tmp_path / "speech"))
    out = str(tmp_path / "set")
    tool.main(["--clean", clean, "--out", out, "--seed", "3", "--t60", "0.2", "0.3"])
    # the same files through the broadband calls alone
    want = str(tmp_path / "want")
    names = ["p001/p001_000", "p001/p001_001"]
    drawn = rooms.draw_rooms(names, 3, t60=(0.2, 0.3))
    rows = []
    for u, name in enumerate(names):
        n = int(round(1.5 * rooms.eyring_t60(drawn[u, 0:3], drawn[u, 9:15], drawn[u, 15]) * 16000))
        h, flags = rooms.shoebox_rir(torch.from_numpy(drawn[u:u + 1]).cuda(), 16000, n)
        rows += rooms.room_rows([name], drawn[u:u + 1], 16000, n, acoustics.rir_acoustics(h, 16000), flags)
        for sub, v in (("clean", wavfile.read(os.path.join(clean, name + ".wav"))[1]), ("rir", h[0].cpu().numpy())):
            os.makedirs(os.path.join(want, sub, "p001"), exist_ok=True)
            wavfile.write(os.path.join(want, sub, name + ".wav"), 16000, v.astype(np.float32))
    rooms.write_rooms(os.path.join(want, "rooms.csv"), rows)
    a, b = _tree(out), _tree(want)
    assert sorted(a) == sorted(b) and len(a) == 5 and all(a[f] == b[f] for f in a)
    assert "beta_125" not in open(os.path.join(out, "rooms.csv")).readline()
