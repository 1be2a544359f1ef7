"""CPU tests of the banded rooms' host side: the float64 restatement tests/_ism_bands_ref.py against a plain triple loop, the
octave bank, the per-band Eyring conversion, the band draws, the per-band columns of rooms.csv, and every argument check of the Python layer and the C
entries (no GPU needed: nothing is launched and no data pointer is dereferenced)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acoustics_ref as AR  # noqa: E402
import _ism_bands_ref as BR  # noqa: E402
import _ism_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import acoustics as A  # noqa: E402
from buddy_amd.utils import rooms  # noqa: E402

L0, S0, R0 = (4.1, 3.3, 2.7), (1.1, 0.9, 1.3), (2.9, 2.2, 1.6)
BETA2 = ((0.9, -0.7, 0.8, 0.85, -0.6, 0.75), (0.5, 0.0, 0.6, -0.4, 0.7, 0.3))          # unequal; a negative and, in band 1 only, a zero coefficient
AIR2 = (0.0, 0.02)


def test_restatement_equals_the_triple_loop():
    rm = R.room(L0, S0, R0, 0.123)                               # the row's own coefficients are not read
    for order, count in ((0, 1), (1, 7), (2, 25)):
        want = BR.naive_bands(rm, BETA2, AIR2, 8000, 400, order)
        u, M, Aa, G, E = BR.rir_bands(rm, BETA2, AIR2, 8000, 400, order)
        assert len(BR.band_images(rm, BETA2, AIR2, 8000, 700, order)[0]) == count
        assert np.abs(u - want).max() <= 1e-15 and np.abs(want[0]).max() > 0.02 and np.abs(want[1]).max() > 0.02
        assert np.all(Aa >= np.abs(u) - 1e-18) and np.all(G >= Aa - 1e-18) and np.all(E >= BR.GAIN_ULPS * Aa - 1e-18)
    # without air a band is the broadband room with the band's coefficients; 0^0 = 1 keeps the direct sound of the band with a zero wall
    u = BR.rir_bands(rm, BETA2, None, 8000, 700)[0]
    for k in range(2):
        assert np.abs(u[k] - R.rir(R.room(L0, S0, R0, BETA2[k]), 8000, 700)[0]).max() <= 1e-16
    d = math.dist(S0, R0)
    assert abs(BR.naive_bands(rm, BETA2, AIR2, 8000, 400, 0)[1].max() / BR.naive_bands(rm, BETA2, None, 8000, 400, 0)[1].max() - math.exp(-0.02 * d)) < 1e-15


def test_combination_is_a_causal_convolution():
    rs = np.random.RandomState(0)
    u, bank = rs.standard_normal((3, 50)), rs.standard_normal((3, 7))
    h, S = BR.combine(u, bank)
    want = np.zeros(50)
    for n in range(50):
        for k in range(3):
            for j in range(7):
                if n - j >= 0:
                    want[n] += bank[k, j] * u[k, n - j]
    assert np.abs(h - want).max() <= 1e-13 and np.all(S >= np.abs(h) - 1e-13)


def _taper_sums(Nh, G):
    """S (the largest sum over the design grid of |W(f - f_g)| / G over four offsets of f inside a grid step) with W the transform of the Hann taper
    of octave_bank, and the part of it further than 2 / Nh cycles per sample from f: derived from Nh and the taper alone"""
    P = (Nh - 1) // 2
    n = np.arange(-P, P + 1, dtype=np.float64)
    w = 0.5 * (1.0 + np.cos(np.pi * n / (P + 1)))
    total = side = 0.0
    for off in (0.0, 0.25, 0.5, 0.75):
        nu = (np.arange(G) - G // 2 + off) / G                            # f_g - f in cycles per sample
        W = np.abs(np.cos(2.0 * np.pi * nu[:, None] * n[None, :]) @ w) / G
        total, side = max(total, float(W.sum())), max(side, float(W[np.abs(nu) > 2.0 / Nh].sum()))
    return total, side


@pytest.mark.parametrize("fs,centres,Nh", [(16000, rooms.BAND_CENTRES, rooms.BANK_TAPS), (8000, (250, 500, 1000, 2000), 255), (16000, (1000,), 31)])
def test_octave_bank(fs, centres, Nh):
    """The tapered response is the ideal magnitude D, sampled on the design grid, under the discrete convolution with the taper's transform W, whose
    grid sum is the taper's centre tap, 1, at every frequency.  So |H(f)| <= S = sum |W| / G =: 1 + eps for every row (the last row, delta minus the
    others, included: the others' ideal magnitudes sum to a value in [0, 1]), and at a centre f_k, where D_k = 1,
    |H_k(f_k) - 1| <= sum |W| |D_k(f_g) - 1| <= S sin^2(pi / 2 |log2(1 - delta / f_k)|) + S_side, delta = 2 fs / Nh the split between the main lobe,
    where D_k departs from 1 by at most the cross-fade's value at f_k - delta, and the rest, where it departs by at most 1."""
    bank = rooms.octave_bank(fs, centres, Nh)
    nb, P = len(centres), (Nh - 1) // 2
    assert bank.shape == (nb, Nh) and bank.dtype == np.float64
    delta = np.zeros(Nh)
    delta[P] = 1.0
    assert np.abs(bank.sum(axis=0) - delta).max() <= 1e-15
    assert np.abs(bank - bank[:, ::-1]).max() <= 1e-15                                   # zero phase around tap P
    G = 8
    while G < 4 * Nh:
        G *= 2
    S, S_side = _taper_sums(Nh, G)
    n = np.arange(-P, P + 1, dtype=np.float64)
    f = np.linspace(0.0, 0.5 * fs, 4001)
    H = np.cos(2.0 * np.pi * f[:, None] / fs * n[None, :]) @ bank.T                      # (F, nb): real, the rows are even
    print(f"octave_bank fs {fs} Nh {Nh}: 1 + eps = {S:.4f}, largest |H| {np.abs(H).max():.6f}")
    assert np.abs(H).max() <= S
    if nb == 1:
        assert np.array_equal(bank[0], delta)
        return
    for k, fc in enumerate(centres):
        Hc = float(np.cos(2.0 * np.pi * fc / fs * n) @ bank[k])
        d = 2.0 * fs / Nh
        assert d < 0.5 * fc or k == 0, "the main lobe must fit below the centre"
        tol = S * math.sin(0.5 * math.pi * min(1.0, abs(math.log2(max(1.0 - d / fc, 0.5))))) ** 2 + S_side
        print(f"octave_bank fs {fs} Nh {Nh} centre {fc}: |H - 1| = {abs(Hc - 1.0):.2e}, tolerance {tol:.3f}")
        assert abs(Hc - 1.0) <= tol
    # far from the cross-fades a row is 1 or 0: half an octave below the lowest centre, row 0 passes and the last row stops
    lo = np.cos(2.0 * np.pi * 0.5 * centres[0] / fs * n) @ bank.T
    assert abs(lo[0] - 1.0) <= S_side and abs(lo[-1]) <= S_side


def test_octave_bank_refusals():
    for bad in ((125, 250, 501), (250, 125), (1000, 2000, 4000, 8000), (), (0.0,)):
        with pytest.raises(ValueError):
            rooms.octave_bank(16000, bad, 63)
    for Nh in (0, 64, 65539):
        with pytest.raises(ValueError):
            rooms.octave_bank(16000, (500, 1000), Nh)
    assert np.array_equal(rooms.octave_bank(16000, (500, 1000), 1).sum(axis=0), [1.0])


def test_eyring_beta_bands_round_trip():
    dims, t60s = (5.0, 4.0, 3.0), (0.9, 0.6, 0.45, 0.3, 0.2, 0.12)
    b = rooms.eyring_beta_bands(dims, t60s)
    assert b.shape == (6, 6) and b.dtype == np.float64 and np.all(b == b[:, :1]) and np.all(np.diff(b[:, 0]) < 0)
    for k, t in enumerate(t60s):
        assert b[k, 0] == rooms.eyring_beta(dims, t) and abs(rooms.eyring_t60(dims, b[k]) / t - 1.0) < 1e-12
    assert np.array_equal(rooms.eyring_beta_bands(dims, t60s, c=340.0)[:, 0], [rooms.eyring_beta(dims, t, 340.0) for t in t60s])


def test_draw_band_rooms_extends_draw_rooms():
    names = [f"p{u // 3:03d}/u{u:02d}" for u in range(12)]
    plain = rooms.draw_rooms(names, 5)
    rows, beta, t60s = rooms.draw_band_rooms(names, 5)
    cs = rooms.BAND_CENTRES
    assert rows.shape == (12, 16) and beta.shape == (12, 6, 6) and t60s.shape == (12, 6)
    keep = [i for i in range(16) if not 9 <= i < 15]
    assert np.array_equal(rows[:, keep], plain[:, keep])                                  # geometry, positions, c: exactly draw_rooms'
    k1 = rooms.nearest_band(cs)
    assert cs[k1] == 1000 and np.array_equal(rows[:, 9:15], plain[:, 9:15]) and np.array_equal(beta[:, k1], plain[:, 9:15])     # the nominal T60 sits at 1 kHz
    perm = [7, 2, 11, 0]
    sub = rooms.draw_band_rooms([names[i] for i in perm], 5)
    assert all(np.array_equal(x, y[perm]) for x, y in zip(sub, (rows, beta, t60s)))        # not a function of the list or its order
    slopes = []
    for b in range(12):
        T = rooms.eyring_t60(plain[b, 0:3], plain[b, 9:15])
        s = -np.log2(t60s[b] / t60s[b, k1]) / np.log2(np.array(cs) / 1000.0, where=np.arange(6) != k1, out=np.ones(6))
        s = np.delete(s, k1)
        assert abs(t60s[b, k1] / T - 1.0) < 1e-12 and np.abs(s - s[0]).max() < 1e-9 and -1e-9 <= s[0] <= 0.3 + 1e-9
        slopes.append(s[0])
        for k in range(6):
            assert np.all(beta[b, k] == rooms.eyring_beta(rows[b, 0:3], t60s[b, k]))
    assert len({round(v, 9) for v in slopes}) == 12
    # the slope comes from its own purpose number: the rooms' draws are untouched, and a fixed slope and the clip do what they say
    assert rooms.ROOM_BANDS == 5 and rooms.ROOM_BANDS != rooms.ROOMS
    flat = rooms.draw_band_rooms(names[:2], 5, slope=(0.0, 0.0))[2]
    assert np.abs(flat / flat[:, :1] - 1.0).max() < 1e-12
    clipped = rooms.draw_band_rooms(names[:2], 5, slope=(2.0, 2.0), t60_clip=(0.1, 1.5))[2]
    assert clipped.min() == 0.1 and clipped.max() == 1.5
    with pytest.raises(ValueError):
        rooms.draw_band_rooms(names[:1], 5, slope=(0.3, 0.1))
    with pytest.raises(ValueError):
        rooms.draw_band_rooms(names[:1], 5, centres=())


def test_rooms_csv_band_columns(tmp_path):
    nan = float("nan")
    cs = (500, 1000, 2000)
    rm = np.stack([R.room(L0, S0, R0, 0.9), R.room((5.0, 4.0, 3.0), (1, 1, 1), (4, 3, 2), 0.8, c=340.0)])
    beta = np.stack([rooms.eyring_beta_bands(L0, (0.5, 0.4, 0.3)), np.array([[0.9] * 6, [0.8, 0.7, 0.8, 0.8, 0.6, 0.8], [0.5] * 6])])
    vals = torch.zeros(2, 4, 6, dtype=torch.float64)
    vals[:, :, 1] = torch.tensor([[0.4, 0.5, 0.41, 0.3], [0.3, 0.35, nan, 0.2]], dtype=torch.float64)
    vals[:, :, 2] = vals[:, :, 1] + 0.01
    ac = A.RirAcoustics((0.0, 500.0, 1000.0, 2000.0), vals, torch.tensor([[511, 501, 502, 503], [511, 7, 8, 9]], dtype=torch.int32), torch.tensor([7, 9], dtype=torch.int32))
    rows = rooms.room_rows(["p1/a", "all/c"], rm, 16000, [4800, 7200], ac, torch.tensor([1, 1], dtype=torch.int32), bands=(cs, beta))
    assert rm[0, 9] == 0.9                                                               # the caller's rows are not written to
    p = str(tmp_path / "rooms.csv")
    rooms.write_rooms(p, rows)
    head = open(p).read().splitlines()[0]
    plain = ("file,Lx,Ly,Lz,sx,sy,sz,rx,ry,rz,beta_x0,beta_x1,beta_y0,beta_y1,beta_z0,beta_z1,c,eyring_T60,distance,fs,n,flag,"
             "EDT,T20,T30,C50,DRR,acoustics_flags")
    assert head == plain + "".join(f",beta_{f},eyring_T60_{f},T20_{f},T30_{f},acoustics_flags_{f}" for f in cs)
    back = AR.read_csv(p)
    assert [back[0][c] for c in rooms.COLUMNS[9:15]] == beta[0, 1].tolist() and [back[1][c] for c in rooms.COLUMNS[9:15]] == [0.8, 0.7, 0.8, 0.8, 0.6, 0.8]
    assert back[0]["beta_500"] == beta[0, 0, 0] and abs(back[0]["eyring_T60_500"] / 0.5 - 1.0) < 1e-12 and back[0]["eyring_T60"] == back[0]["eyring_T60_1000"]
    assert back[0]["T20_500"] == 0.5 and back[0]["T30_2000"] == 0.3 + 0.01 and back[0]["acoustics_flags_1000"] == 502 and math.isnan(back[1]["T20_1000"])
    assert back[1]["eyring_T60_1000"] == rooms.eyring_t60((5.0, 4.0, 3.0), beta[1, 1], 340.0)
    assert abs(rooms.eyring_t60((5.0, 4.0, 3.0), back[1]["beta_1000"], 340.0) / back[1]["eyring_T60_1000"] - 1.0) < 1e-12     # the equivalent uniform wall
    assert rooms.room_rows(["p1/a", "all/c"], rm, 16000, [4800, 7200], ac)[0].keys() == dict.fromkeys(plain.split(",")).keys()   # no block: today's columns
    with pytest.raises(ValueError, match="analysed"):
        rooms.room_rows(["p1/a", "all/c"], rm, 16000, 4800, ac, bands=((250, 500, 1000), beta))
    with pytest.raises(ValueError, match="shape"):
        rooms.room_rows(["p1/a", "all/c"], rm, 16000, 4800, ac, bands=(cs, beta[:, :2]))


def test_python_argument_checks():
    rm = np.stack([R.room(L0, S0, R0, 0.5)] * 2)
    beta = np.stack([np.array(BETA2)] * 2)
    bank = rooms.octave_bank(8000, (500, 1000), 31)
    ok = dict(rooms=rm, beta=beta, fs=8000, n=256, bank=bank)
    bad = [dict(rooms=rm.astype(np.float32)), dict(rooms=rm[:, :15]), dict(beta=beta.astype(np.float32)), dict(beta=beta[:1]), dict(beta=beta[:, :, :5]),
           dict(beta=np.zeros((2, 9, 6))), dict(beta=np.zeros((2, 0, 6))), dict(bank=bank[:1]), dict(bank=bank[:, :30]), dict(bank=bank.astype(np.float32)),
           dict(bank=np.zeros((2, 65539))), dict(air=np.zeros(3)), dict(air=np.zeros((2, 2), dtype=np.float32)), dict(air=np.zeros((1, 2)))]
    for change in bad:
        with pytest.raises(ValueError):
            rooms.shoebox_rir_bands(**{**ok, **change})
    with pytest.raises(ValueError, match="row 0 "):
        rooms.shoebox_rir_bands(**{**ok, "n": 32000, "max_images": 1e3})
    with pytest.raises(_lib.BuddyHipError):
        rooms.shoebox_rir_bands(**{**ok, "rooms": torch.from_numpy(rm)})


def test_c_argument_checks_need_no_gpu():
    """every BUDDY_ERR_ARG case of the two entries, with nothing launched: 0x1000 stands in for the device pointers"""
    lib = _lib.load()
    X = 0x1000
    assert lib.buddy_ism_max_bands() == 8 and lib.buddy_ism_band_list() >= 64 and lib.buddy_band_combine_tile() >= 64
    good = [X, X, None, 2, 3, 16000, 100, -1, X, 100, X]       # rooms, beta, air, B, nb, fs, N, max_order, u, ldu, flags
    cases = [(0, None, "null rooms"), (1, None, "null beta"), (8, None, "null u"), (10, None, "null flags"), (3, 0, "B < 1"), (3, 65536, "B above 65535"),
             (4, 0, "nb < 1"), (4, 9, "nb above 8"), (5, 999, "fs below 1000"), (5, 1000001, "fs above 10^6"), (6, 0, "N < 1"), (6, (1 << 20) + 1, "N above 2^20"),
             (9, 99, "ldu below N"), (7, -2, "max_order below -1")]
    for i, v, why in cases:
        args = list(good)
        args[i] = v
        if why == "N above 2^20":
            args[9] = 1 << 21
        assert lib.buddy_shoebox_bands(*args, None) == 2, why
        assert lib.buddy_last_error().decode().startswith("buddy_shoebox_bands: "), why
    good = [X, 2, 3, 100, 100, X, 31, X, 100]                   # u, B, nb, ldu, N, bank, Nh, h, ldh
    cases = [(0, None, "null u"), (5, None, "null bank"), (7, None, "null h"), (1, 0, "B < 1"), (1, 65536, "B above 65535"), (2, 0, "nb < 1"), (2, 9, "nb above 8"),
             (4, 0, "N < 1"), (3, 99, "ldu below N"), (8, 99, "ldh below N"), (6, 0, "Nh < 1"), (6, 30, "Nh even"), (6, 65539, "Nh above 65537")]
    for i, v, why in cases:
        args = list(good)
        args[i] = v
        assert lib.buddy_band_combine(*args, None) == 2, why
        assert lib.buddy_last_error().decode().startswith("buddy_band_combine: "), why
    for name in ("buddy_ism_max_bands", "buddy_ism_band_list", "buddy_band_combine_tile", "buddy_shoebox_bands", "buddy_band_combine"):
        assert name in _lib.EXPORTED


def test_high_band_decays_faster_on_the_restatement():
    """the coefficients of the GPU suite's physical check, chosen here first: on the restatement at a quarter of its length the 4 kHz band's response
    has lost more of its energy after the first 60 ms than the 500 Hz band's"""
    dims = (5.0, 4.0, 3.0)
    beta = rooms.eyring_beta_bands(dims, (0.35, 0.15))
    u = BR.rir_bands(R.room(dims, (1.2, 1.1, 1.4), (3.9, 2.8, 1.7), 0.5), beta, None, 16000, 2000)[0]
    late = (u[:, 1000:] ** 2).sum(axis=1) / (u ** 2).sum(axis=1)
    print(f"late energy after 60 ms: 500 Hz {late[0]:.3e}, 4 kHz {late[1]:.3e}")
    assert late[1] < 0.2 * late[0]
