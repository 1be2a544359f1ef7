"""CPU tests of the diffuse late tail's host side: the new symbols, ``rooms.tail_window`` on hand-computed cases with half-up
ties, every argument check of the two C entries (nothing is launched; the windows, decays and nu, which the entries read to check them, are real host
arrays) and of the Python layer and the tool, the float64 restatement (tests/_tail_ref.py) on closed forms, and the decay claim on the two small rooms
of the issue's table: with the tail the measured T30 misses the nominal T60 by less than half of what the pure image-source response misses it by."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _acoustics_ref as AR  # noqa: E402
import _ism_ref as IR  # noqa: E402
import _tail_ref as TR  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import noise as NZ  # noqa: E402
from buddy_amd.utils import rng, rooms  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000
# the two small rooms of the table: size, source, receiver, nominal T60
SMALL = (((5.0, 4.0, 3.0), (1.0, 1.1, 1.2), (3.5, 2.9, 1.6), 0.25), ((3.2, 3.5, 2.5), (1.0, 1.2, 1.3), (2.2, 2.6, 1.5), 0.30))


def table_room(L, s, r, t60):
    return rooms.room_row(L, s, r, rooms.eyring_beta(L, t60))


# ---- symbols, windows, refusals -----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("buddy_tail_fit", "buddy_tail_mix", "buddy_tail_tile"):
        assert name in _lib.EXPORTED and getattr(lib, name) is not None       # header = signatures = exports: tests/test_abi_host.py
    assert lib.buddy_tail_tile() == 1024 and rooms.TAIL == 10 == NZ.NOISE_SENSOR + 1 and TR.HW == lib.buddy_ism_half_width()
    assert (rooms.TAIL_PURE, rooms.TAIL_ZERO) == (TR.PURE, TR.ZERO) == (2, 4)
    assert os.path.isfile(os.path.join(ROOT, "buddy_amd", "csrc", "tail.hip"))             # build.sh compiles and links every csrc/*.hip


def test_tail_window_by_hand():
    """|s - r| = 3.43 m at c = 343 m/s, fs = 16 kHz: 160 samples exactly; Hw = 40.  80 ms = 1280 samples, half of it 640"""
    rm = rooms.room_row((6, 5, 3), (1.0, 2.0, 1.5), (4.43, 2.0, 1.5), 0.5)
    assert rooms.tail_window(rm[None], FS, 80.0, 256).tolist() == [[200, 840, 1480, 1736]]
    # ties round up: a lag of 112.5 samples (2.25 m at c = 320, fs = 16000) gives 113; 0.5 x 12.53125 ms = 100.25 -> 100, 12.53125 ms = 200.5 -> 201
    rm = rooms.room_row((6, 5, 3), (1.0, 2.0, 1.5), (3.25, 2.0, 1.5), 0.5, c=320.0)
    assert 2.25 * 16000 / 320.0 == 112.5 and 12.53125 * 1e-3 * 16000 == 200.5 and 0.03125 * 1e-3 * 16000 == 0.5
    assert rooms.tail_window(rm[None], FS, 12.53125, 1).tolist() == [[153, 253, 354, 355]]
    # 0.03125 ms = half a sample: n_f = n_d + half_up(0.25) = n_d, n_x = n_d + half_up(0.5) = n_d + 1
    assert rooms.tail_window(rm[None], FS, 0.03125, 7).tolist() == [[153, 153, 154, 161]]
    # a group takes the NEAREST microphone; groups are consecutive rows
    near = rooms.room_row((6, 5, 3), (1.0, 2.0, 1.5), (2.715, 2.0, 1.5), 0.5)                      # 1.715 m: 80 samples
    rm0 = rooms.room_row((6, 5, 3), (1.0, 2.0, 1.5), (4.43, 2.0, 1.5), 0.5)
    got = rooms.tail_window(np.stack([rm0, near, rm0, rm0]), FS, 80.0, 256, mics=2)
    assert got.tolist() == [[120, 760, 1400, 1656], [200, 840, 1480, 1736]] and got.dtype == np.int64
    assert np.array_equal(got, TR.window(np.stack([rm0, near, rm0, rm0]), FS, 80.0, 256, 2))
    # the restatement agrees on drawn rooms
    drawn = rooms.draw_rooms([f"r{i}" for i in range(16)], 0)
    assert np.array_equal(rooms.tail_window(drawn, FS, 80.0, 256), TR.window(drawn, FS, 80.0, 256))


def test_python_refusals():
    rm = table_room(*SMALL[0])[None]
    key = np.array([rng.stream_key(0, "a")], dtype=np.uint32)
    for bad in (dict(tail_ms=0.0), dict(tail_ms=float("nan")), dict(ramp=0), dict(mics=0), dict(mics=9), dict(mics=2), dict(tail_ms=0.03, ramp=4)):
        a = dict(dict(tail_ms=80.0, ramp=256, mics=1), **bad)
        with pytest.raises(ValueError, match="tail_window"):
            rooms.tail_window(rm, FS, a["tail_ms"], a["ramp"], a["mics"])
    with pytest.raises(ValueError, match="float64"):
        rooms.tail_window(rm.astype(np.float32), FS, 80.0, 256)
    same = rm.copy()
    same[0, 6:9] = same[0, 3:6]
    with pytest.raises(ValueError, match="distance"):
        rooms.tail_window(same, FS, 80.0, 256)
    with pytest.raises(ValueError, match="t60"):
        rooms.shoebox_rir_hybrid(rm, FS, 4000, -1.0, key)
    with pytest.raises(ValueError, match="t60"):
        rooms.shoebox_rir_hybrid(rm, FS, 4000, np.array([0.2, 0.3]), key)
    with pytest.raises(ValueError, match="keys"):
        rooms.shoebox_rir_hybrid(rm, FS, 4000, 0.25, np.zeros((2, 2), dtype=np.uint32))
    with pytest.raises(ValueError, match="n >= 1"):
        rooms.shoebox_rir_hybrid(rm, FS, 0, 0.25, key)
    with pytest.raises(ValueError, match="tail_window"):
        rooms.shoebox_rir_hybrid(rm, FS, 4000, 0.25, key, ramp=0)
    arr = rooms.array_rows(rm[0], 4)
    with pytest.raises(ValueError, match="waves"):
        rooms.shoebox_rir_hybrid(arr, FS, 4000, 0.25, key, mics=4, waves=0)
    with pytest.raises(ValueError, match="spherical"):
        rooms.shoebox_rir_hybrid(arr, FS, 4000, 0.25, key, mics=4, field="planar")
    with pytest.raises(ValueError, match="max_images"):                      # judged at n_e, not at n: n_e = 1592 samples here
        rooms.shoebox_rir_hybrid(rm, FS, 4000, 0.25, key, max_images=1e3)
    with pytest.raises(_lib.BuddyHipError):                                  # CPU tensors
        rooms.shoebox_rir_hybrid(torch.from_numpy(rm), FS, 4000, 0.25, key)
    # banded rooms
    beta = rooms.eyring_beta_bands(rm[0, 0:3], (0.3, 0.2))[None]
    bank = rooms.octave_bank(FS, (1000, 2000), 63)
    t60s = np.array([[0.3, 0.2]])
    with pytest.raises(ValueError, match="needs t60s"):
        rooms.shoebox_rir_bands(rm, beta, FS, 4000, bank, tail_ms=80.0)
    with pytest.raises(ValueError, match="t60s"):
        rooms.shoebox_rir_bands(rm, beta, FS, 4000, bank, tail_ms=80.0, t60s=t60s[:, :1], keys=key)
    with pytest.raises(ValueError, match="keys"):
        rooms.shoebox_rir_bands(rm, beta, FS, 4000, bank, tail_ms=80.0, t60s=t60s, keys=np.zeros((1, 3), dtype=np.uint32))
    with pytest.raises(ValueError, match="tail_window"):
        rooms.shoebox_rir_bands(rm, beta, FS, 4000, bank, tail_ms=-1.0, t60s=t60s, keys=key)
    with pytest.raises(_lib.BuddyHipError):
        rooms.shoebox_rir_bands(torch.from_numpy(rm), beta, FS, 4000, bank, tail_ms=80.0, t60s=t60s, keys=key)


def test_argument_checks_need_no_gpu():
    """every BUDDY_ERR_ARG case of the two entries, with nothing launched: 0x1000 stands in for the data pointers"""
    lib = _lib.load()
    X, inf, nan = 0x1000, float("inf"), float("nan")
    ints = lambda *v: C.cast((C.c_int * len(v))(*v), C.c_void_p)
    dbls = lambda *v: C.cast((C.c_double * len(v))(*v), C.c_void_p)
    win, delta, nu = ints(100, 200, 120, 220), dbls(*([20.0] * 4)), dbls(*([1.0] * 4))
    good = dict(u=X, f64=0, B=4, nb=2, D=2, ldr=1000, ldk=500, len=480, win=win, R=256, delta=delta, nu=nu, amp=X, flags=X, z=None, ldz=0, keys=X, purpose=10,
                fs=16000, n=4000, out=X, ldor=8000, ldok=4000)
    both = [(dict(u=None), "null u"), (dict(win=None), "null win"), (dict(delta=None), "null delta"), (dict(amp=None), "null amp"),
            (dict(B=0), "B < 1"), (dict(B=65536, D=1), "B above 65535"), (dict(nb=0), "nb < 1"), (dict(nb=lib.buddy_ism_max_bands() + 1), "nb above the bands"),
            (dict(D=0), "D < 1"), (dict(D=9, B=9), "D above 8"), (dict(D=3), "B % D"), (dict(fs=999), "fs"), (dict(len=0), "len < 1"),
            (dict(len=2 ** 20 + 1, ldr=2 ** 21, ldk=2 ** 20 + 1), "len above 2^20"), (dict(ldr=479), "ldr < len"), (dict(ldk=479), "ldk < len"),
            (dict(win=ints(100, 100, 120, 220)), "n_f = n_x"), (dict(win=ints(100, 200, 230, 220)), "n_f > n_x"), (dict(win=ints(-1, 200, 120, 220)), "n_f < 0"),
            (dict(delta=dbls(20.0, nan, 20.0, 20.0)), "NaN delta"), (dict(delta=dbls(20.0, 20.0, 20.0, inf)), "infinite delta")]
    fit_only = [(dict(flags=None), "null flags"), (dict(win=ints(100, 200, 120, 481)), "n_x beyond u"), (dict(nu=dbls(1.0, 0.0, 1.0, 1.0)), "nu = 0"),
                (dict(nu=dbls(1.0, 1.0, nan, 1.0)), "NaN nu")]
    mix_only = [(dict(out=None), "null out"), (dict(keys=None), "neither z nor keys"), (dict(R=0), "R < 1"), (dict(R=261), "n_x + R beyond u"),
                (dict(n=0), "n < 1"), (dict(n=2 ** 30 + 1, ldor=2 ** 32, ldok=2 ** 31), "n above 2^30"), (dict(z=X, ldz=3999), "ldz < n"),
                (dict(ldok=3999), "ldok < n"), (dict(ldor=7999), "ldor below (nb - 1) ldok + n")]

    def fit(a):
        return lib.buddy_tail_fit(a["u"], a["f64"], a["B"], a["nb"], a["D"], a["ldr"], a["ldk"], a["len"], a["win"], a["delta"], a["nu"], a["fs"], a["amp"],
                                  a["flags"], None)

    def mix(a):
        return lib.buddy_tail_mix(a["u"], a["f64"], a["B"], a["nb"], a["D"], a["ldr"], a["ldk"], a["len"], a["win"], a["R"], a["delta"], a["amp"], a["z"],
                                  a["ldz"], a["keys"], a["purpose"], a["fs"], a["n"], a["out"], a["ldor"], a["ldok"], None)
    for call, who, cases in ((fit, "buddy_tail_fit: ", both + fit_only), (mix, "buddy_tail_mix: ", both + mix_only)):
        for change, why in cases:
            assert call(dict(good, **change)) == 2, (who, why)
            assert lib.buddy_last_error().decode().startswith(who), (who, why)


def test_tool_flag_refusals(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_paired_set as T
    base = ["--clean", str(tmp_path), "--out", str(tmp_path / "out")]
    for extra, why in ((["--diffuse-tail", "0"], "--diffuse-tail"), (["--diffuse-tail", "--tail-ramp", "0"], "--tail-ramp"),
                       (["--diffuse-tail", "--mics", "4", "--tail-waves", "0"], "--tail-waves"), (["--diffuse-tail", "--mics", "9"], "--mics"),
                       (["--diffuse-tail", "--mics", "4", "--bands"], "--bands")):
        with pytest.raises(SystemExit) as e:
            T.main(base + extra)
        assert why in str(e.value), (extra, str(e.value))


# ---- the restatement on closed forms ------------------------------------------------------------------------------------------------------------
def test_fit_recovers_an_exponential_envelope():
    """u = A exp(-delta t) w[n] with w = +-1 has E = A^2 S exactly in real arithmetic: the fit returns A to the rounding of the two sums"""
    rs = np.random.RandomState(0)
    n_f, n_x = 700, 1340
    for D, A, delta in ((1, 0.37, 27.6), (3, 2.5e-3, 6.9), (8, 11.0, 0.0)):
        w = np.where(rs.rand(D, 1, n_x) < 0.5, -1.0, 1.0)
        u = A * np.exp(-delta * TR.times(0, n_x, FS)) * w
        got, flags, E, S = TR.fit(u, [n_f], [n_x], np.array([[delta]]), FS, D)
        rel = abs(got[0, 0] / A - 1.0)
        print(f"tail restatement fit: D {D} A {A} delta {delta}: relative error {rel:.2e}")
        assert rel <= 2.0 * TR.fit_bound(n_x - n_f, D, delta, n_x, FS) and flags.tolist() == [0]
    got, flags, _, _ = TR.fit(np.zeros((2, 1, n_x)), [n_f], [n_x], np.array([[5.0]]), FS, 2)
    assert got.tolist() == [[0.0]] and flags.tolist() == [TR.ZERO]


def test_mix_switches_at_the_crossover_and_keeps_u_below_it():
    rs = np.random.RandomState(1)
    n, n_x, delta, A = 900, 333, np.array([[31.0]]), np.array([[0.2]])
    u, z = rs.standard_normal((1, 1, 600)), rs.standard_normal((1, n))
    env = A[0, 0] * np.exp(-delta[0, 0] * TR.times(0, n, FS)) * z[0]
    # R = 1: th(n_x) = pi / 4, and from n_x + 1 on the tail alone (u is zero from n_e = n_x + 1)
    out, bound = TR.mix(u, n, [n_x], 1, delta, A, z, FS)
    assert np.array_equal(out[0, 0, :n_x], u[0, 0, :n_x]) and np.all(bound[0, 0, :n_x] == 0.0)
    assert abs(out[0, 0, n_x] - math.sqrt(0.5) * (u[0, 0, n_x] + env[n_x])) < 1e-15
    assert np.abs(out[0, 0, n_x + 1:] - env[n_x + 1:]).max() < 1e-16
    # a long ramp: power-complementary weights, u bit for bit wherever th = 0, and the pure rule
    R = 200
    out, _ = TR.mix(u, n, [n_x], R, delta, A, z, FS)
    idx = np.arange(n_x, n_x + R)
    th = 0.5 * np.pi * (idx - n_x + 0.5) / R
    assert np.array_equal(out[0, 0, :n_x], u[0, 0, :n_x])
    assert np.abs(out[0, 0, idx] - (np.cos(th) * u[0, 0, idx] + np.sin(th) * env[idx])).max() < 1e-15
    assert np.abs(out[0, 0, n_x + R:] - env[n_x + R:]).max() < 1e-16
    win = np.array([[100, 200, n_x, n_x + R]])
    for m in (n_x + R - 1, n_x + R):                                         # n <= n_e: the pure response, flag 2
        o, _, flags, _ = TR.hybrid(u, m, win, R, delta, z[:, :m], FS)
        assert np.array_equal(o[0, 0], u[0, 0, :m]) and flags.tolist() == [TR.PURE]
    o, _, flags, _ = TR.hybrid(u, n_x + R + 1, win, R, delta, z[:, :n_x + R + 1], FS)
    assert flags.tolist() == [0] and o[0, 0, -1] != 0.0 and np.array_equal(o[0, 0, :n_x], u[0, 0, :n_x])
    # nu divides the tail of its own row only
    o2, _ = TR.mix(np.repeat(u, 2, axis=0), n, [n_x], R, delta, A, np.repeat(z, 2, axis=0), FS, D=2, nu=np.array([1.0, 4.0]))
    assert np.array_equal(o2[0], out[0]) and np.abs(o2[1, 0, n_x + R:] - 0.25 * env[n_x + R:]).max() < 1e-16


def test_field_nu_is_the_taps_energy():
    dirs = NZ.sphere_directions(64)
    phi = 2.0 * np.pi * np.arange(4) / 4
    pos = np.stack([0.1 * np.cos(phi), 0.1 * np.sin(phi), np.zeros(4)], axis=1)
    rm = rooms.array_rows(table_room(*SMALL[0]), 4, 0.1, 0.0)
    p, nu = rooms.tail_field(rm, 4, FS, 64)
    assert np.abs(p[0] - pos).max() < 1e-15 and nu.shape == (4,)
    want = TR.field_nu(NZ.delay_taps(p[0], dirs, FS)[0])
    assert np.abs(nu / want - 1.0).max() < 1e-15 and np.all(np.abs(nu - 1.0) < 0.05)       # a fractional delay loses a little power above its band edge


# ---- the decay claim ----------------------------------------------------------------------------------------------------------------------------
def test_tail_brings_t30_to_the_nominal_t60():
    """the two small rooms of the table, response 1.5 x T60, the noise the file's own normals: |T30 / T60 - 1| with the tail is below half of the pure
    image-source response's (measured here: pure 0.44 to 0.73, tailed at most 0.063)"""
    for i, (L, s, r, t60) in enumerate(SMALL):
        rm = table_room(L, s, r, t60)
        n = int(round(1.5 * t60 * FS))
        pure = IR.rir(rm, FS, n)[0]
        win = TR.window(rm, FS, 80.0, 256)
        z = rng.normals(rng.stream_key(0, f"room{i}"), rooms.TAIL, 0, n).astype(np.float64)
        delta = np.array([[3.0 * math.log(10.0) / t60]])
        out, A, flags, _ = TR.hybrid(pure[None, None, :int(win[0, 3])], n, win, 256, delta, z[None], FS)
        assert flags.tolist() == [0] and A[0, 0] > 0.0
        t30 = [AR.metrics(h, AR.argmax_abs(h), FS)[0][AR.T30] for h in (pure, out[0, 0])]
        off = [abs(v / t60 - 1.0) for v in t30]
        print(f"tail decay (host): room {L} nominal T60 {t60:.2f} s: T30 pure {t30[0]:.3f} s (off by {off[0]:.3f}), with the tail {t30[1]:.3f} s (off by {off[1]:.3f})")
        assert off[1] < 0.5 * off[0]
