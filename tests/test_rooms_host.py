"""CPU tests of the room simulator's host side: the float64 restatement (tests/_ism_ref.py) on closed forms and symmetries, the Eyring conversions,
the room draws, rooms.csv, and every argument check of the C entry (no GPU needed: nothing is launched and no data pointer is dereferenced)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acoustics_ref as AR  # noqa: E402
import _ism_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import acoustics as A  # noqa: E402
from buddy_amd.utils import rooms  # noqa: E402

L0, S0, R0 = (4.1, 3.3, 2.7), (1.1, 0.9, 1.3), (2.9, 2.2, 1.6)
BETA = (0.9, -0.7, 0.8, 0.85, -0.6, 0.75)                    # unequal, two of them negative


def test_vectorised_restatement_equals_the_triple_loop():
    rm = R.room(L0, S0, R0, BETA)
    want, count = R.naive(rm, 8000, 700, 2)
    h, M, Aa, G = R.rir(rm, 8000, 700, 2)
    assert count == 25 and len(R.images(rm, 8000, 700, 2)[0]) == 25          # every image of order <= 2 arrives before sample 700
    assert np.abs(h - want).max() <= 1e-15 and np.abs(want).max() > 0.02
    assert M.max() >= 2 and np.all(Aa >= np.abs(h) - 1e-18) and np.all(G >= Aa - 1e-18)


def test_free_field_is_one_kernel():
    rm = R.room(L0, S0, R0, 0.0)
    h, M, _, _ = R.rir(rm, 8000, 400)
    d = math.dist(S0, R0)
    tau = d * 8000 / 343.0
    n = np.arange(400)
    x = n - R.HW - tau
    want = np.where(np.abs(x) < R.HW, np.sinc(x) * 0.5 * (1.0 + np.cos(np.pi * x / R.HW)), 0.0) / (4.0 * np.pi * d)
    assert np.abs(h - want).max() <= 1e-17
    assert abs(int(np.argmax(np.abs(h))) - (tau + R.HW)) <= 0.5 and abs(h.max() * 4.0 * np.pi * d - 1.0) < 0.3
    assert M.max() > 1                                      # the images are counted whatever their gain


@pytest.mark.parametrize("order,count", [(0, 1), (1, 7), (2, 25)])
def test_image_counts_per_order(order, count):
    assert len(R.images(R.room(L0, S0, R0, BETA), 8000, 2048, order)[0]) == count
    assert rooms.images_within_order(order) == count


def test_reciprocity_and_mirroring():
    """measured here: 6.6e-16 and 2.6e-16 at a peak of 0.032.  The mirror with beta_x0 != beta_x1 catches walls assigned to the wrong exponent."""
    h0 = R.rir(R.room(L0, S0, R0, BETA), 8000, 2048)[0]
    assert np.abs(h0).max() > 0.03
    swapped = R.rir(R.room(L0, R0, S0, BETA), 8000, 2048)[0]
    assert np.abs(h0 - swapped).max() <= 1e-13
    b = BETA
    mirrored = R.rir(R.room(L0, (L0[0] - S0[0],) + S0[1:], (L0[0] - R0[0],) + R0[1:], (b[1], b[0]) + b[2:]), 8000, 2048)[0]
    assert np.abs(h0 - mirrored).max() <= 1e-13
    wrong = R.rir(R.room(L0, (L0[0] - S0[0],) + S0[1:], (L0[0] - R0[0],) + R0[1:], b), 8000, 2048)[0]       # walls not swapped: another room
    assert np.abs(h0 - wrong).max() > 1e-4


def test_eyring_round_trip():
    for dims, t in (((5.0, 4.0, 3.0), 0.3), ((8.0, 3.0, 2.4), 1.0), ((3.0, 3.0, 3.5), 0.2)):
        b = rooms.eyring_beta(dims, t)
        assert 0.0 < b < 1.0 and abs(rooms.eyring_t60(dims, b) / t - 1.0) < 1e-12 and abs(rooms.eyring_t60(dims, [b] * 6, 343.0) / t - 1.0) < 1e-12
    S, V = 2 * (20 + 12 + 15), 60.0
    assert abs(rooms.eyring_beta((5.0, 4.0, 3.0), 0.3) ** 2 - math.exp(-24 * math.log(10) * V / (343.0 * S * 0.3))) < 1e-15
    assert rooms.eyring_t60((5, 4, 3), 1.0) == math.inf and rooms.eyring_t60((5, 4, 3), 0.0) == 0.0
    assert rooms.eyring_t60((5, 4, 3), (0.9, 0.9, 0.9, 0.9, 0.5, 0.9)) < rooms.eyring_t60((5, 4, 3), 0.9)


def test_draw_rooms_is_a_function_of_seed_and_name():
    names = [f"p{u // 3:03d}/u{u:02d}" for u in range(12)]
    a = rooms.draw_rooms(names, 5)
    assert a.shape == (12, 16) and a.dtype == np.float64 and np.array_equal(a, rooms.draw_rooms(names, 5))
    assert not np.array_equal(a, rooms.draw_rooms(names, 6))
    perm = [7, 2, 11, 0]
    assert np.array_equal(rooms.draw_rooms([names[i] for i in perm], 5), a[perm])                  # reordering and subsetting
    for rm in a:
        L, s, r, beta, c = rm[0:3], rm[3:6], rm[6:9], rm[9:15], rm[15]
        assert 3 <= L[0] <= 8 and 3 <= L[1] <= 8 and 2.4 <= L[2] <= 3.5 and c == 343.0
        assert np.all(s >= 0.5) and np.all(s <= L - 0.5) and np.all(r >= 0.5) and np.all(r <= L - 0.5) and np.linalg.norm(s - r) >= 0.5
        assert np.all(beta == beta[0]) and 0.2 <= rooms.eyring_t60(L, beta, c) * (1 + 1e-12) and rooms.eyring_t60(L, beta, c) <= 1.0 * (1 + 1e-12)
    assert len({tuple(rm) for rm in a}) == 12
    with pytest.raises(RuntimeError, match="tries"):
        rooms.draw_rooms(["x"], 0, dims=((1.2, 1.2), (1.2, 1.2), (1.2, 1.2)), wall_margin=0.5, min_dist=0.5)    # the free box is 0.2 m wide
    with pytest.raises(ValueError):
        rooms.draw_rooms(["x"], 0, dims=((1.0, 2.0), (3, 8), (2.4, 3.5)))


def test_rooms_csv_round_trip(tmp_path):
    nan = float("nan")
    rm = np.stack([R.room(L0, S0, R0, BETA), R.room((5.0, 4.0, 3.0), (1, 1, 1), (4, 3, 2), 0.8, c=340.0)])
    ac = A.RirAcoustics((0.0,), torch.tensor([[[0.5, 0.25, nan, 3.0, -11.5, 0.036]], [[0.4, 0.2, 0.3, 2.0, -10.0, 0.03]]], dtype=torch.float64),
                        torch.tensor([[0b011111011], [511]], dtype=torch.int32), torch.tensor([7, 9], dtype=torch.int32))
    rows = rooms.room_rows(["p1/a b", "all/c"], rm, 16000, [4800, 7200], ac, torch.tensor([1, 0], dtype=torch.int32))
    p = str(tmp_path / "rooms.csv")
    rooms.write_rooms(p, rows)
    text = open(p).read().splitlines()
    assert text[0] == ("file,Lx,Ly,Lz,sx,sy,sz,rx,ry,rz,beta_x0,beta_x1,beta_y0,beta_y1,beta_z0,beta_z1,c,eyring_T60,distance,fs,n,flag,"
                       "EDT,T20,T30,C50,DRR,acoustics_flags")
    back = AR.read_csv(p)
    assert len(back) == 2 and [r["file"] for r in back] == ["p1/a b", "all/c"]
    for r, b in zip(rows, back):
        for k, v in r.items():
            if isinstance(v, float):
                assert (math.isnan(v) and math.isnan(b[k])) or v == b[k], (k, v, b[k])            # repr() of a double reads back bit for bit
            else:
                assert v == b[k], k
    assert back[0]["beta_x1"] == -0.7 and back[0]["n"] == 4800 and back[1]["flag"] == 0 and math.isnan(back[0]["T30"]) and back[0]["acoustics_flags"] == 0b011111011
    assert back[1]["eyring_T60"] == rooms.eyring_t60((5.0, 4.0, 3.0), 0.8, 340.0) and abs(back[1]["distance"] - math.sqrt(14.0)) < 1e-15


def test_cpu_tensor_is_refused():
    with pytest.raises(_lib.BuddyHipError):
        rooms.shoebox_rir(torch.from_numpy(R.room(L0, S0, R0, BETA)[None]), 8000, 256)


def test_max_images_refusal_names_the_row():
    rm = np.stack([R.room(L0, S0, R0, BETA), R.room((2.0, 2.0, 2.0), (0.5, 0.5, 0.5), (1.5, 1.5, 1.5), 0.9)])
    est = rooms.estimated_images(rm, 16000, 32000)
    assert abs(est[1] / (4.0 / 3.0 * math.pi * 686.0 ** 3 / 8.0) - 1.0) < 1e-12 and est[0] < est[1]
    with pytest.raises(ValueError, match="row 1 "):
        rooms.shoebox_rir(rm, 16000, 32000, max_images=0.5 * (est[0] + est[1]))
    with pytest.raises(ValueError, match="row 0 "):
        rooms.shoebox_rir(rm, 16000, 32000, max_images=1e3)
    assert rooms.estimated_images(rm, 16000, 32000, max_order=2).tolist() == [25.0, 25.0]            # an order cap bounds the count
    with pytest.raises(ValueError, match="float64"):
        rooms.shoebox_rir(rm.astype(np.float32), 16000, 256)


def test_argument_checks_need_no_gpu():
    """every BUDDY_ERR_ARG case of buddy_shoebox_rir, with nothing launched: 0x1000 stands in for the device pointers"""
    lib = _lib.load()
    X = 0x1000
    cases = [        # (rooms, B, fs, N, max_order, h, ldh, flags)
        ((None, 2, 16000, 100, -1, X, 100, X), "null rooms"), ((X, 2, 16000, 100, -1, None, 100, X), "null h"),
        ((X, 2, 16000, 100, -1, X, 100, None), "null flags"), ((X, 0, 16000, 100, -1, X, 100, X), "B < 1"),
        ((X, 65536, 16000, 100, -1, X, 100, X), "B above 65535"), ((X, 2, 999, 100, -1, X, 100, X), "fs below 1000"),
        ((X, 2, 1000001, 100, -1, X, 100, X), "fs above 10^6"), ((X, 2, 16000, 0, -1, X, 100, X), "N < 1"),
        ((X, 2, 16000, (1 << 20) + 1, -1, X, 1 << 21, X), "N above 2^20"), ((X, 2, 16000, 100, -1, X, 99, X), "ldh below N"),
        ((X, 2, 16000, 100, -2, X, 100, X), "max_order below -1"),
    ]
    for args, why in cases:
        assert lib.buddy_shoebox_rir(*args, None) == 2, why
        assert lib.buddy_last_error().decode().startswith("buddy_shoebox_rir: "), why
    assert lib.buddy_ism_half_width() == 40 == R.HW
    assert lib.buddy_ism_tile() >= 64 and lib.buddy_ism_tile() % 64 == 0 and lib.buddy_ism_list() >= 64


def test_new_names_are_exported():
    for name in ("buddy_ism_half_width", "buddy_ism_tile", "buddy_shoebox_rir"):
        assert name in _lib.EXPORTED
