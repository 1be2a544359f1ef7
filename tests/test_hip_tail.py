"""GPU tests of the diffuse late tail (csrc/tail.hip) against the float64 restatement tests/_tail_ref.py.

Bounds, all derived (EPS = 2^-53) and doubled where the restatement evaluates the same expression in double, because it carries the same roundings:

  fit   one evaluation of A = sqrt(E / S) is within ``TR.fit_bound`` relative: a sum of m non-negative terms carries at most (m + c) EPS whatever its
        order -- E has W D terms and one rounding per square, S has W terms whose exp carries its argument's two roundings (2 |2 delta t| EPS) and
        two ulp -- the square root halves what the sums carry, quotient and root add two, and the division by nu one more.
  mix   per sample ``TR.mix``'s bound: EPS (8 |u| + (14 + 2 |delta t|) |env|), env = amp exp(-delta t) z (6 absolute on cos and sin from the angle's
        two roundings and two ulp; 2 |delta t| + 2 relative on exp; the products and the sum); the fp32 form adds its one output rounding,
        2^-24 |out|.  Below n_x the output holds the bits of u.

The noise is the kernel's own: z is what ``buddy_philox_fill`` stores for the same (key, purpose, draw), as tests/test_hip_noise.py takes its sources.
Every case prints its largest deviation over the bound (profiles/tail_accuracy.txt holds a run's lines)."""
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
import _ism_ref as IR  # noqa: E402
import _tail_ref as TR  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import acoustics, noise, rng, rooms  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000
SENTINEL = 12345.0
EPS = 2.0 ** -53
# the four rooms of the issue's table: size, source, receiver, nominal T60
TABLE = (((5.0, 4.0, 3.0), (1.0, 1.1, 1.2), (3.5, 2.9, 1.6), 0.25), ((3.2, 3.5, 2.5), (1.0, 1.2, 1.3), (2.2, 2.6, 1.5), 0.30),
         ((6.0, 4.5, 2.8), (1.5, 1.2, 1.4), (4.2, 3.1, 1.6), 0.50), ((7.5, 3.2, 3.3), (1.0, 1.6, 1.2), (6.2, 2.0, 1.7), 0.80))


def table_room(i, t60=None):
    L, s, r, t = TABLE[i]
    return rooms.room_row(L, s, r, rooms.eyring_beta(L, t if t60 is None else t60))


def keys_of(*names):
    return np.array([rng.stream_key(5, n) for n in names], dtype=np.uint32)


@pytest.fixture(scope="module")
def lib():
    return _lib.require_gpu()


def stream():
    return torch.cuda.current_stream().cuda_stream


def on(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_normals(keys, n, purpose=rooms.TAIL, draw=0):
    """(B, n) float32: what buddy_philox_fill stores for draw ``draw`` of ``purpose`` of each key"""
    B = len(keys)
    out = torch.empty(1, B, n, dtype=torch.float32, device="cuda")
    kt = on(keys.view(np.int32))
    _lib.check(_lib.require_gpu().buddy_philox_fill(out.data_ptr(), 1, B, n, kt.data_ptr(), purpose, draw, rng.NORMAL, stream()))
    return out[0].cpu().numpy()


def over(err, bound):
    """the largest err / bound; where the bound is zero the error must be"""
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


def padded(a, ld_row, ld_band, fill=SENTINEL):
    """(B, nb, len) -> a flat device array with row stride ``ld_row`` and band stride ``ld_band``, the gaps holding the sentinel; and its host copy"""
    B, nb, ln = a.shape
    flat = np.full(B * ld_row, fill, dtype=a.dtype)
    for b in range(B):
        for k in range(nb):
            flat[b * ld_row + k * ld_band:b * ld_row + k * ld_band + ln] = a[b, k]
    return on(flat), flat


# ---- fit ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 2, 8])
@pytest.mark.parametrize("D", [1, 3, 8])
def test_fit_against_the_restatement(lib, D, nb):
    """window lengths around the reduction's widths (a wave is 64 lanes, a workgroup 256 threads), fp32 and fp64 input in strides larger than the
    rows, two groups of which the second has an all-zero window in band 0 (amplitude 0, flag 4); the bound is the module's, doubled"""
    rs = np.random.RandomState(100 * D + nb)
    G, B = 2, 2 * D
    for W in (1, 63, 64, 65, 257, 1000):
        n_f = np.array([37, 5]) + 3 * W
        n_x = n_f + W
        ln = int(n_x.max()) + 9
        delta = rs.uniform(2.0, 40.0, (G, nb))
        nu = rs.uniform(0.8, 1.2, B)
        for dt in (np.float32, np.float64):
            u = rs.standard_normal((B, nb, ln)).astype(dt) * np.exp(-10.0 * np.arange(ln) / FS).astype(dt)
            u[D:, 0, n_f[1]:n_x[1]] = 0.0
            ldk = ln + 5
            ldr = nb * ldk + 7
            ut, _ = padded(u, ldr, ldk)
            amp = torch.full((B, nb), SENTINEL, dtype=torch.float64, device="cuda")
            flags = torch.full((G,), -1, dtype=torch.int32, device="cuda")
            win, dl, nt = on(np.stack([n_f, n_x], axis=1).astype(np.int32)), on(delta), on(nu)
            _lib.check(lib.buddy_tail_fit(ut.data_ptr(), int(dt == np.float64), B, nb, D, ldr, ldk, ln, win.data_ptr(), dl.data_ptr(), nt.data_ptr(), FS,
                                          amp.data_ptr(), flags.data_ptr(), stream()))
            A, fl, _, _ = TR.fit(u, n_f, n_x, delta, FS, D)
            want = np.repeat(A, D, axis=0) / nu[:, None]
            got = amp.cpu().numpy()
            bound = np.array([[2.0 * TR.fit_bound(W, D, delta[b // D, k], n_x[b // D], FS) + 2.0 * EPS for k in range(nb)] for b in range(B)]) * want
            ratio = over(np.abs(got - want), bound)
            print(f"tail fit: W {W} D {D} nb {nb} {np.dtype(dt).name}: max err/bound {ratio:.3f}")
            assert ratio <= 1.0 and flags.cpu().tolist() == fl.tolist() == [0, TR.ZERO] and np.all(got[D:, 0] == 0.0) and np.all(got[:D] > 0.0)
            # without nu: the amplitude itself, one value per group
            _lib.check(lib.buddy_tail_fit(ut.data_ptr(), int(dt == np.float64), B, nb, D, ldr, ldk, ln, win.data_ptr(), dl.data_ptr(), None, FS,
                                          amp.data_ptr(), flags.data_ptr(), stream()))
            got = amp.cpu().numpy()
            assert over(np.abs(got - np.repeat(A, D, axis=0)), bound * nu[:, None]) <= 1.0 and all(np.all(got[g * D:(g + 1) * D] == got[g * D]) for g in range(G))


# ---- mix ----------------------------------------------------------------------------------------------------------------------------------------
def run_mix(lib, u, n, n_x, R, delta, amp, keys, aligned, z=None):
    """one launch on padded arrays; returns the (B, nb, n) result after checking that every gap still holds the sentinel"""
    B, nb, ln = u.shape
    f64 = u.dtype == np.float64
    pad = (4 - ln % 4) % 4 + (0 if aligned else 1)
    ldk, ldok = ln + pad + 4, n + (4 - n % 4) % 4 + (4 if aligned else 5)
    ldr, ldor = nb * ldk + (4 if aligned else 3), nb * ldok + (8 if aligned else 6)
    ut, _ = padded(u, ldr, ldk)
    ot, _ = padded(np.zeros((B, nb, 0), dtype=u.dtype), ldor, ldok)
    win = on(np.stack([np.asarray(n_x) - 1, np.asarray(n_x)], axis=1).astype(np.int32))
    zt = None if z is None else on(z)
    dl, at, kt = on(delta), on(amp), on(keys.view(np.int32))
    _lib.check(lib.buddy_tail_mix(ut.data_ptr(), int(f64), B, nb, 1, ldr, ldk, ln, win.data_ptr(), R, dl.data_ptr(), at.data_ptr(),
                                  None if zt is None else zt.data_ptr(), 0 if zt is None else z.shape[1], kt.data_ptr(), rooms.TAIL, FS, n,
                                  ot.data_ptr(), ldor, ldok, stream()))
    flat = ot.cpu().numpy()
    out = np.empty((B, nb, n), dtype=u.dtype)
    keep = np.ones(len(flat), dtype=bool)
    for b in range(B):
        for k in range(nb):
            o = b * ldor + k * ldok
            out[b, k] = flat[o:o + n]
            keep[o:o + n] = False
    assert np.all(flat[keep] == SENTINEL), "something was written outside the rows"
    return out


@pytest.mark.parametrize("nb", [1, 8])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_mix_against_the_restatement(lib, nb, dt):
    """four rows whose crossovers take every residue mod 4, ramps 1, 2, 255, 256, 1000, lengths just behind n_e (+1, +3, +4, +5), around the tile of
    buddy_tail_tile() samples and 4097; 16-byte aligned strides (the vector path of the fp32 form) and odd ones; the bound is the module's, doubled;
    the gaps behind every row keep their sentinel"""
    T = lib.buddy_tail_tile()
    rs = np.random.RandomState(7 * nb + (dt == np.float64))
    keys = keys_of("a", "b", "c", "d")
    n_x = np.array([100, 101, 102, 103])
    B = 4
    z = gpu_normals(keys, 4200)
    for R in (1, 2, 255, 256, 1000):
        worst = 0.0
        ne = int(n_x[0]) + R
        ln = int(n_x.max()) + R
        u = (rs.standard_normal((B, nb, ln)) * 0.05).astype(dt)
        delta = rs.uniform(5.0, 35.0, (B, nb))
        amp = rs.uniform(0.01, 0.1, (B, nb))
        for n in sorted({ne + 1, ne + 3, ne + 4, ne + 5, T - 1, T, T + 1, 2 * T + 2, 4097}):
            want, bound = TR.mix(u, n, n_x, R, delta, amp, z[:, :n], FS)
            tol = 2.0 * bound + (2.0 ** -24 * np.abs(want) if dt == np.float32 else 0.0)
            for aligned in (True, False):
                got = run_mix(lib, u, n, n_x, R, delta, amp, keys, aligned)
                for b in range(B):
                    m = min(n, int(n_x[b]))
                    assert np.array_equal(got[b, :, :m], u[b, :, :m]), "below the crossover the output holds the bits of u"
                ratio = over(np.abs(got.astype(np.float64) - want), tol)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (R, n, aligned, ratio)
        print(f"tail mix: R {R} nb {nb} {np.dtype(dt).name}: max err/bound {worst:.3f}")
    # a given z (the array form) with the stored normals gives the bits of the generated form
    n = 2 * T + 4
    a = run_mix(lib, u, n, n_x, 1000, delta, amp, keys, True)
    for aligned in (True, False):
        zz = np.ascontiguousarray(z[:, :n + (0 if aligned else 1)])
        assert np.array_equal(run_mix(lib, u, n, n_x, 1000, delta, amp, keys, aligned, z=zz), a)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------------
def hybrid_against_restatement(tag, rm, n, t60, keys, D=1, z=None, **kw):
    """the whole chain on the GPU's own image-source part and noise: windows, amplitude (fit bound), result (mix bound on the GPU's amplitude)"""
    h, flags, info = rooms.shoebox_rir_hybrid(rm, FS, n, t60, keys, mics=D, **kw)
    R = info["ramp"]
    win = TR.window(rm, FS, info["tail_ms"], R, D)
    assert np.array_equal(info["windows"], win) and h.shape == (len(rm), n) and h.dtype == torch.float32
    ln = min(n, int(win[:, 3].max()))
    assert info["ism_samples"] == ln
    u = rooms.shoebox_rir(rm, FS, ln)[0].cpu().numpy()
    delta = (3.0 * math.log(10.0) / np.broadcast_to(np.asarray(t60, dtype=np.float64), (len(rm) // D,))).reshape(-1, 1)
    assert np.array_equal(info["delta"], delta)
    if z is None:
        z = gpu_normals(keys, n)
    nu = info["nu"]
    want, A, fl, _ = TR.hybrid(u[:, None, :], n, win, R, delta, z, FS, D, nu)
    got = h.cpu().numpy().astype(np.float64)
    assert flags.tolist() == [1 | int(v) for v in fl]
    ra = 0.0
    for g in range(len(win)):
        if A[g, 0] > 0.0 and n > int(win[g, 3]):
            fb = 2.0 * TR.fit_bound(int(win[g, 2] - win[g, 1]), D, delta[g, 0], win[g, 2], FS) + 2.0 * EPS
            ra = max(ra, abs(info["amp"][g, 0] / A[g, 0] - 1.0) / fb)
    want, bound = TR.mix(u[:, None, :], n, win[:, 2], R, delta, info["amp"], z, FS, D, nu)
    for b in range(len(rm)):
        if fl[b] & TR.PURE:
            want[b, 0], bound[b, 0] = u[b, :n], 0.0
    rh = over(np.abs(got - want[:, 0]), 3.0 * bound[:, 0] + 2.0 ** -24 * np.abs(want[:, 0]))
    print(f"tail hybrid {tag}: B {len(rm)} D {D} n {n} n_e {win[:, 3].tolist()}: amplitude err/bound {ra:.3f}, h err/bound {rh:.3f}")
    assert ra <= 1.0 and rh <= 1.0
    return h, flags, info, u, z


def test_broadband_hybrid_and_the_pure_rule(lib):
    rm = np.stack([table_room(0), table_room(1)])
    keys = keys_of("r0", "r1")
    win = rooms.tail_window(rm, FS, 80.0, 256)
    n = int(win[:, 3].max()) + 1501
    h, flags, info, u, _ = hybrid_against_restatement("two rooms", rm, n, np.array([0.25, 0.30]), keys)
    assert flags.tolist() == [1, 1] and np.all(info["amp"] > 0)
    for b in range(2):                                                       # below n_x: shoebox_rir at n_e, bit for bit
        pure = rooms.shoebox_rir(rm[b:b + 1], FS, int(win[b, 3]))[0][0].cpu().numpy()
        assert np.array_equal(h[b, :win[b, 2]].cpu().numpy(), pure[:win[b, 2]])
    assert float(h[:, -500:].abs().max()) > 0.0
    # n <= n_e: the pure response with flag bit 1; one sample more and the tail is there; a batch may hold both kinds (room 1 is the nearer pair)
    ne = int(win[1, 3])
    assert win[1, 3] < win[0, 3]
    for m, want in ((ne, [3, 3]), (ne - 5, [3, 3]), (ne + 1, [3, 1])):
        hm, fm, im = rooms.shoebox_rir_hybrid(rm, FS, m, np.array([0.25, 0.30]), keys)
        pure = rooms.shoebox_rir(rm, FS, m)[0]
        assert fm.tolist() == want and torch.equal(hm[0], pure[0]) and (torch.equal(hm[1], pure[1]) == (want[1] == 3))
        assert (im["amp"][:, 0] > 0).tolist() == [w == 1 for w in want]
    hybrid_against_restatement("mixed batch", rm, ne + 1, np.array([0.25, 0.30]), keys)
    # other crossovers and ramps, an odd length
    hybrid_against_restatement("20 ms, ramp 1", rm, 2001, 0.3, keys, tail_ms=20.0, ramp=1)
    hybrid_against_restatement("33.3 ms, ramp 1000", rm, 3002, 0.3, keys, tail_ms=33.3, ramp=1000)


def _bands_setup(nb=2, Nh=63):
    centres = (1000, 2000) if nb == 2 else rooms.BAND_CENTRES
    return centres, rooms.octave_bank(FS, centres, Nh)


def test_rows_are_independent_of_the_batch(lib):
    """a row in a batch of five equals its B = 1 run bit for bit: broadband, banded, and groups of four microphones"""
    rm = np.stack([table_room(0), table_room(1), table_room(2), table_room(3), table_room(1, 0.4)])
    names = [f"f{i}" for i in range(5)]
    keys = keys_of(*names)
    t60 = np.array([0.25, 0.30, 0.50, 0.80, 0.40])
    n = int(rooms.tail_window(rm, FS, 80.0, 256)[:, 3].max()) + 777
    h5, f5, _ = rooms.shoebox_rir_hybrid(rm, FS, n, t60, keys)
    for b in (0, 3):
        h1, f1, _ = rooms.shoebox_rir_hybrid(rm[b:b + 1], FS, n, t60[b:b + 1], keys[b:b + 1])
        assert torch.equal(h5[b], h1[0]) and f5[b] == f1[0] == 1
    centres, bank = _bands_setup()
    beta = np.stack([rooms.eyring_beta_bands(r[0:3], (t, 0.7 * t)) for r, t in zip(rm, t60)])
    t60s = np.stack([t60, 0.7 * t60], axis=1)
    air = np.array([0.0, 0.003])
    h5, f5, i5, u5 = rooms.shoebox_rir_bands(rm, beta, FS, n, bank, air=air, t60s=t60s, keys=keys, tail_ms=80.0, return_bands=True)
    assert np.allclose(i5["delta"], 3.0 * math.log(10.0) / t60s + 343.0 * air[None, :], rtol=1e-14, atol=0.0) and f5.tolist() == [1] * 5
    for b in (1, 4):
        h1, f1, i1, u1 = rooms.shoebox_rir_bands(rm[b:b + 1], beta[b:b + 1], FS, n, bank, air=air, t60s=t60s[b:b + 1], keys=keys[b:b + 1], tail_ms=80.0, return_bands=True)
        assert torch.equal(h5[b], h1[0]) and torch.equal(u5[b], u1[0]) and np.array_equal(i5["amp"][b], i1["amp"][0])
    arr = np.concatenate([rooms.array_rows(r, 4, 0.1, 0.2 * i) for i, r in enumerate(rm)])
    h5, f5, i5 = rooms.shoebox_rir_hybrid(arr, FS, n, t60, keys, mics=4, waves=32)
    assert h5.shape == (20, n) and f5.tolist() == [1] * 20 and i5["amp"].shape == (5, 1)
    for g in (0, 2):
        h1, _, i1 = rooms.shoebox_rir_hybrid(arr[4 * g:4 * g + 4], FS, n, t60[g:g + 1], keys[g:g + 1], mics=4, waves=32)
        assert torch.equal(h5[4 * g:4 * g + 4], h1) and i5["amp"][g, 0] == i1["amp"][0, 0]


def test_banded_hybrid_against_the_restatement_and_equal_bands(lib):
    """the band-domain mix on the GPU's own band responses, then: equal bands and no air give the broadband hybrid delayed by the bank's P, within the
    combine bound of tests/test_hip_rooms_bands.py (the fp32 rounding of the result plus the double sum's) plus what the broadband side carries -- its
    own fp32 rounding of u and of the result, 2^-24 each on the parts, and 2^-23 on the tail for the amplitude fitted to rounded samples -- and the
    two simulators' own bounds on the image-source part"""
    rm = table_room(1)[None]
    keys = keys_of("bands")
    centres, bank = _bands_setup(6, 127)
    nb, P = len(centres), 63
    t60s = np.array([[0.45, 0.40, 0.35, 0.30, 0.25, 0.2]])
    beta = rooms.eyring_beta_bands(rm[0, 0:3], t60s[0])[None]
    air = np.array([0.0, 0.0, 0.001, 0.002, 0.004, 0.008])
    win = rooms.tail_window(rm, FS, 80.0, 256)
    ne, nx = int(win[0, 3]), int(win[0, 2])
    n = ne + 1203
    h, flags, info, uo = rooms.shoebox_rir_bands(rm, beta, FS, n, bank, air=air, t60s=t60s, keys=keys, tail_ms=80.0, return_bands=True)
    ub = rooms.shoebox_rir_bands(rm, beta, FS, ne, bank, air=air, return_bands=True)[2].cpu().numpy()
    z = gpu_normals(keys, n)
    delta = 3.0 * math.log(10.0) / t60s + 343.0 * air[None, :]
    want, A, fl, _ = TR.hybrid(ub, n, win, 256, delta, z, FS)
    ra = max(abs(info["amp"][0, k] / A[0, k] - 1.0) / (2.0 * TR.fit_bound(nx - int(win[0, 1]), 1, delta[0, k], nx, FS)) for k in range(nb))
    want, bound = TR.mix(ub, n, win[:, 2], 256, delta, info["amp"], z, FS)
    got = uo.cpu().numpy()
    ru = over(np.abs(got - want), 3.0 * bound)
    assert np.array_equal(got[:, :, :nx], ub[:, :, :nx]) and flags.tolist() == [1]
    hw, S = BR.combine(want[0], bank)
    rh = over(np.abs(h[0].cpu().numpy().astype(np.float64) - hw), 2.0 ** -23 * np.abs(hw) + (bank.size + 8) * 2.0 ** -53 * S
              + np.array([np.convolve(np.abs(bank[k]), 3.0 * bound[0, k])[:n] for k in range(nb)]).sum(axis=0))
    print(f"tail banded hybrid: nb {nb} n {n} n_e {ne}: amplitude err/bound {ra:.3f}, bands err/bound {ru:.3f}, h err/bound {rh:.3f}")
    assert ra <= 1.0 and ru <= 1.0 and rh <= 1.0
    # equal bands
    t60 = 0.3
    beta = rooms.eyring_beta_bands(rm[0, 0:3], [t60] * nb)[None]
    h, flags, info, uo = rooms.shoebox_rir_bands(rm, beta, FS, n, bank, t60s=np.full((1, nb), t60), keys=keys, tail_ms=80.0, return_bands=True)
    got = uo.cpu().numpy()
    assert all(np.array_equal(got[0, k], got[0, 0]) for k in range(nb)), "one noise sequence and one arithmetic for all bands"
    hb, fb, ib = rooms.shoebox_rir_hybrid(rm, FS, n - P, t60, keys)
    broad = hb[0].cpu().numpy().astype(np.float64)
    u32 = rooms.shoebox_rir(rm, FS, ne)[0].cpu().numpy().astype(np.float64)
    parts, _ = TR.mix(np.abs(u32)[None, None, :], n - P, win[:, 2], 256, np.full((1, 1), 3.0 * math.log(10.0) / t60), ib["amp"], np.abs(z[:, :n - P]), FS)
    ref = IR.rir(rm[0], FS, ne)
    _, M, Aa, G, E = BR.rir_bands(rm[0], beta[0, :1], None, FS, ne, -1)
    ism = np.zeros(n - P)
    ism[:ne] = IR.bound(*ref) + BR.band_bound(ne, M, Aa, G, E)[0]
    delayed, dparts, dism = (np.concatenate([np.zeros(P), v[:n - P]]) for v in (broad, parts[0, 0], ism))
    hw, S = BR.combine(got[0], bank)
    tol = 2.0 ** -23 * np.abs(hw) + (bank.size + 8) * 2.0 ** -53 * S + 2.0 ** -24 * np.abs(delayed) + 3.0 * 2.0 ** -24 * dparts + dism
    ratio = over(np.abs(h[0].cpu().numpy().astype(np.float64) - delayed), tol)
    print(f"tail equal bands against the delayed broadband hybrid: max err/bound {ratio:.3f}")
    assert ratio <= 1.0 and np.abs(delayed[-400:]).max() > 0.0


def test_array_tail_is_a_diffuse_field(lib):
    """D = 4: one amplitude for the group, the rows' nu applied, the chain held to the restatement on the GPU's own field; the measured coherence of
    the tail between microphones is printed next to sinc(2 f d / c) and not asserted"""
    room = table_room(2)
    arr = rooms.array_rows(room, 4, 0.1, 0.3)
    keys = keys_of("array")
    win = rooms.tail_window(arr, FS, 80.0, 256, mics=4)
    n = int(win[0, 3]) + 16384
    pos, nu = rooms.tail_field(arr, 4, FS, 512)
    taps = noise.delay_taps(pos[0], noise.sphere_directions(512), FS)[0]
    assert np.abs(nu / TR.field_nu(taps) - 1.0).max() < 1e-15
    z = noise.diffuse_noise(pos, keys, n, FS, waves=512, purpose=rooms.TAIL)[0].cpu().numpy()
    assert not np.array_equal(z, noise.diffuse_noise(pos, keys, n, FS, waves=512)[0].cpu().numpy()), "the tail's draws are its own purpose's"
    h, flags, info, u, _ = hybrid_against_restatement("array of four", arr, n, 0.5, keys, D=4, z=z)
    assert info["amp"].shape == (1, 1) and np.array_equal(info["nu"], nu) and flags.tolist() == [1] * 4
    assert np.abs(info["amp_rows"][:, 0] * nu / info["amp"][0, 0] - 1.0).max() < 4 * EPS
    assert np.abs(z.astype(np.float64).std(axis=1) / nu - 1.0).max() < 0.05       # the analytic deviation is the field's (16 000 samples: about 1 %)
    # coherence of the whitened tail between microphones 0 and 1 (d = r sqrt 2) and 0 and 2 (d = 2 r): Welch, 256-sample Hann segments, half overlap
    start = int(win[0, 3])
    t = (np.arange(start, n) - TR.HW) / FS
    x = h[:, start:].cpu().numpy().astype(np.float64) * np.exp(info["delta"][0, 0] * t)
    seg = np.stack([x[:, i:i + 256] * np.hanning(256) for i in range(0, x.shape[1] - 255, 128)], axis=1)
    X = np.fft.rfft(seg, axis=2)
    for q, d in ((1, 0.1 * math.sqrt(2.0)), (2, 0.2)):
        coh = np.real((X[0] * np.conj(X[q])).mean(axis=0)) / np.sqrt((np.abs(X[0]) ** 2).mean(axis=0) * (np.abs(X[q]) ** 2).mean(axis=0))
        line = ", ".join(f"{f} Hz {coh[f * 256 // FS]:+.2f} ({np.sinc(2.0 * f * d / 343.0):+.2f})" for f in (500, 1000, 2000, 4000))
        print(f"tail array coherence (sinc), microphones 0-{q}, d = {d:.3f} m, {seg.shape[1]} segments: {line}")


# ---- the decay claim ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_decays():
    """per table room (nominal T60, T30 of the pure response, T30 with the tail) through the real kernels and rir_acoustics, response 1.5 x T60"""
    out = []
    for i, (L, s, r, t60) in enumerate(TABLE):
        rm = table_room(i)[None]
        n = int(round(1.5 * t60 * FS))
        pure = rooms.shoebox_rir(rm, FS, n)[0]
        tail, flags, _ = rooms.shoebox_rir_hybrid(rm, FS, n, t60, keys_of(f"table{i}"))
        assert flags.tolist() == [1]
        ac = acoustics.rir_acoustics(torch.cat([pure, tail]), FS)
        assert int(ac.flags[0, 0]) & 0b100 and int(ac.flags[1, 0]) & 0b100
        out.append((t60, float(ac.values[0, 0, 2]), float(ac.values[1, 0, 2])))
    return tuple(out)


def test_tail_brings_t30_to_the_nominal_t60(lib):
    """all four rooms of the table: |T30 / T60 - 1| with the tail is below half of the pure image-source response's"""
    for (L, _, _, _), (t60, pure, tail) in zip(TABLE, table_decays()):
        a, b = abs(pure / t60 - 1.0), abs(tail / t60 - 1.0)
        print(f"tail decay: room {L} nominal T60 {t60:.2f} s: T30 pure {pure:.3f} s (off by {a:.3f}), with the tail {tail:.3f} s (off by {b:.3f})")
        assert b < 0.5 * a


def test_a_three_second_room_is_simulable(lib):
    """nominal T60 = 3 s, 4.5 s of response: above max_images for the image-source method alone, far below it at n_e.  The pure response is not
    computed, so the decay condition takes the table's place for it: |T30 / T60 - 1| below half of the largest |T30 / T60 - 1| the four pure table
    responses gave in this run (the value the tailed table rooms stayed under is printed next to it)"""
    t60, n = 3.0, int(round(4.5 * FS))
    rm = table_room(1, t60)[None]
    keys = keys_of("long")
    ne = int(rooms.tail_window(rm, FS, 80.0, 256)[0, 3])
    assert rooms.estimated_images(rm, FS, n)[0] > 2e8 > 1e6 > rooms.estimated_images(rm, FS, ne)[0]
    with pytest.raises(ValueError, match="max_images"):
        rooms.shoebox_rir(rm, FS, n)
    h, flags, info = rooms.shoebox_rir_hybrid(rm, FS, n, t60, keys)
    assert h.shape == (1, n) and flags.tolist() == [1] and info["ism_samples"] == ne
    ac = acoustics.rir_acoustics(h, FS)
    t30 = float(ac.values[0, 0, 2])
    off = abs(t30 / t60 - 1.0)
    limit = 0.5 * max(abs(p / t - 1.0) for t, p, _ in table_decays())
    tailed = max(abs(q / t - 1.0) for t, _, q in table_decays())
    print(f"tail decay: 3 s room, {n} samples, image-source part {ne}: T30 {t30:.3f} s (off by {off:.3f}; limit {limit:.3f}; the tailed table rooms stayed under {tailed:.3f})")
    assert int(ac.flags[0, 0]) & 0b100 and off < limit


# ---- the tool -----------------------------------------------------------------------------------------------------------------------------------
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


NEW_COLUMNS = ("tail_ms", "tail_direct", "tail_start", "tail_ramp", "ism_samples", "tail_amp", "tail_flags")


def test_tool_with_the_tail(tmp_path):
    tool = _tool()
    clean = _clean_folder(str(tmp_path / "speech"))
    base = ["--clean", clean, "--seed", "3", "--t60", "0.2", "0.25"]
    out, out2 = str(tmp_path / "set"), str(tmp_path / "set2")
    tool.main(base + ["--diffuse-tail", "--out", out])
    tool.main(base + ["--diffuse-tail", "--out", out2])
    a, b = _tree(out), _tree(out2)
    assert sorted(a) == sorted(b) and len(a) == 5 and all(a[f] == b[f] for f in a)
    rows = AR.read_csv(os.path.join(out, "rooms.csv"))
    names = ["p001/p001_000", "p001/p001_001"]
    drawn = rooms.draw_rooms(names, 3, t60=(0.2, 0.25))
    for u, r in enumerate(rows):
        assert all(c in r for c in NEW_COLUMNS)
        t60 = rooms.eyring_t60(drawn[u, 0:3], drawn[u, 9:15], drawn[u, 15])
        n = int(round(1.5 * t60 * 16000))
        win = rooms.tail_window(drawn[u:u + 1], 16000, 80.0, 256)[0]
        assert (r["tail_ms"], r["tail_direct"], r["tail_start"], r["tail_ramp"], r["ism_samples"], r["tail_flags"]) == (80.0, win[0], win[2], 256, win[3], 0)
        assert r["n"] == n and r["flag"] == 1 and r["tail_amp"] > 0.0
        h = rooms.shoebox_rir_hybrid(drawn[u:u + 1], 16000, n, t60, np.array([rng.stream_key(3, names[u])], dtype=np.uint32))[0][0].cpu().numpy()
        assert np.array_equal(wavfile.read(os.path.join(out, "rir", names[u] + ".wav"))[1], h)
        print(f"tail tool: {names[u]} nominal T60 {t60:.3f} s, measured T30 {r['T30']:.3f} s")
    tool.main(base + ["--diffuse-tail", "60", "--tail-ramp", "128", "--bands", "--out", str(tmp_path / "bands")])
    rows = AR.read_csv(os.path.join(str(tmp_path / "bands"), "rooms.csv"))
    assert all(r["tail_ms"] == 60.0 and r["tail_ramp"] == 128 and r["tail_flags"] == 0 and "tail_amp" not in r for r in rows)
    assert all(r[f"tail_amp_{f}"] > 0.0 for r in rows for f in rooms.BAND_CENTRES)
    tool.main(base + ["--diffuse-tail", "--mics", "4", "--reverberant", "--tail-waves", "64", "--out", str(tmp_path / "array")])
    rows = AR.read_csv(os.path.join(str(tmp_path / "array"), "rooms.csv"))
    assert all(r["mics"] == 4 and r["tail_amp"] > 0.0 and r["tail_flags"] == 0 for r in rows)
    fs, y = wavfile.read(os.path.join(str(tmp_path / "array"), "reverberant", names[0] + ".wav"))
    assert y.shape[1] == 4 and wavfile.read(os.path.join(str(tmp_path / "array"), "rir_array", names[0] + ".wav"))[1].shape[1] == 4


def test_tool_without_the_flag_is_unchanged(tmp_path, monkeypatch):
    """without --diffuse-tail the two new entries are never called and rooms.csv has no new column"""
    tool = _tool()
    lib = _lib.require_gpu()

    def refuse(*a, **k):
        raise AssertionError("a tail entry was called without --diffuse-tail")
    for name in ("buddy_tail_fit", "buddy_tail_mix"):
        monkeypatch.setattr(lib, name, refuse)
    monkeypatch.setattr(rooms, "shoebox_rir_hybrid", refuse)
    monkeypatch.setattr(rooms, "tail_window", refuse)
    clean = _clean_folder(str(tmp_path / "speech"))
    for extra in ([], ["--bands"], ["--mics", "2"]):
        out = str(tmp_path / ("set" + "".join(extra).replace("-", "")))
        tool.main(["--clean", clean, "--out", out, "--seed", "3", "--t60", "0.2", "0.25"] + extra)
        header = open(os.path.join(out, "rooms.csv")).readline()
        assert "tail" not in header and "ism_samples" not in header
