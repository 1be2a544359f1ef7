"""GPU: the diffuse-noise bank (csrc/noise.hip, buddy_amd/utils/noise.py) against the float64 restatement tests/_noise_ref.py.  The restatement is
fed the sources ``buddy_philox_fill`` itself returns for the same keys, purpose and draws, so the comparison holds the kernel's own generator to
the fill's bits as well: one differing normal is an error of the order of a tap, ten orders above the bound

    |out_gpu - out_ref| <= 2^-24 |out_ref| + gamma,    gamma = 2 (2 N W + N + W + 4) 2^-53 A,   A = scale sum_n sum_k |taps s|

(output rounding; the double accumulation of N W terms -- derived in ``_noise_ref.gamma_bound``).  Lengths sit around the tile
T = buddy_noise_tile(), wave counts around the LDS chunk of four.  Every case prints its largest deviation over the bound
(profiles/noise_accuracy.txt holds them)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _noise_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import noise as NZ  # noqa: E402
from buddy_amd.utils import rng  # noqa: E402

pytestmark = pytest.mark.gpu

FS, C = 16000, 343.0
P, W = NZ.PAD, NZ.TAPS


def ring(D, radius=0.1, angle=0.3, lift=0.0):
    phi = angle + 2.0 * np.pi * np.arange(D) / D
    return np.stack([radius * np.cos(phi), radius * np.sin(phi), lift * np.arange(D)], axis=1)


def key_of(name):
    return np.array(rng.stream_key(11, name), dtype=np.uint32)


def gpu_sources(key, purpose, draw0, N, n):
    """(N, n) float64 of the fp32 normals buddy_philox_fill stores: draws draw0 .. draw0 + N - 1"""
    out = torch.empty(N, 1, n, dtype=torch.float32, device="cuda")
    kt = torch.from_numpy(key.reshape(1, 2).view(np.int32).copy()).cuda()
    _lib.check(_lib.require_gpu().buddy_philox_fill(out.data_ptr(), N, 1, n, kt.data_ptr(), purpose, draw0, rng.NORMAL, torch.cuda.current_stream().cuda_stream))
    return out[:, 0].cpu().numpy().astype(np.float64)


def check(tag, taps, first, L, name="a", draw0=0, check_first=True):
    """one file against the restatement; returns (gpu (D, L), ref (D, L), the sources)"""
    N, D, Wt = taps.shape
    key = key_of(name)
    src = gpu_sources(key, NZ.NOISE_FIELD, draw0, N, L + 2 * P)
    want, A = R.noise_bank(taps, first, src, P, L, want_abs=True)
    got = NZ.noise_bank_hip(taps[None], first[None], key[None], L, draw0=draw0, check_first=check_first)
    assert got.shape == (1, D, L) and got.dtype == torch.float32
    got = got[0].cpu().numpy().astype(np.float64)
    bound = 2.0 ** -24 * np.abs(want) + R.gamma_bound(N, Wt, A)
    ratio = np.abs(got - want) / np.maximum(bound, 1e-300)
    print(f"{tag}: N = {N}, D = {D}, L = {L}: max |gpu - ref| = {np.abs(got - want).max():.3e}, worst over the bound {ratio.max():.3f}, max |ref| = {np.abs(want).max():.3f}")
    assert np.all(np.abs(got - want) <= bound), (tag, float(ratio.max()))
    return got, want, src


def geometry(D, N, radius=0.1, fs=FS, field="spherical"):
    pos = ring(D, radius, lift=0.013) if D > 1 else np.array([[0.05, 0.02, 0.01]])
    return NZ.delay_taps(pos, NZ.directions(field, N), fs, C)


@pytest.mark.parametrize("L", [1, 255, 256, 257, 700])
def test_lengths_around_the_tile(L):
    assert _lib.load().buddy_noise_tile() == 256
    got, want, _ = check("length", *geometry(3, 7), L)
    assert np.abs(want).max() > 0.05


@pytest.mark.parametrize("N,D,L", [(1, 3, 257), (7, 3, 257), (8, 3, 257), (9, 3, 257), (512, 2, 600)])
def test_wave_counts_around_the_chunk(N, D, L):
    got, _, _ = check("waves", *geometry(D, N), L)
    if N == 512:
        assert abs(got.var() - 1.0) < 0.15                                   # about unit power: 1200 samples


@pytest.mark.parametrize("D", [1, 3, 8])
def test_microphone_counts(D):
    check("microphones", *geometry(D, 9), 300)


def test_wide_array_and_cylindrical_field():
    taps, first = geometry(4, 9, radius=1.3)                                 # delays up to 60.6 samples
    assert np.abs(first + NZ.HW - 1).max() > 55
    check("wide", taps, first, 300)
    check("cylindrical", *geometry(3, 9, field="cylindrical"), 300)


def unit_geometry(offsets, dirs=((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0))):
    """microphones on the x axis at integer ``offsets`` with fs = c = 1: tau = +-offset exactly"""
    return NZ.delay_taps(np.array([[float(o), 0.0, 0.0] for o in offsets]), np.array(dirs), 1.0, 1.0)


def test_zero_delay_is_the_sum_of_the_sources():
    N, L = 9, 300
    taps, first = NZ.delay_taps(np.zeros((2, 3)), NZ.sphere_directions(N), FS, C)
    assert np.all(first == 1 - NZ.HW) and np.count_nonzero(taps) == N * 2 and np.all(taps[:, :, NZ.HW - 1] == 1.0)
    got, want, src = check("tau = 0", taps, first, L)
    direct = src[:, P:P + L].sum(axis=0) / np.sqrt(N)                        # N^(-1/2) sum_n s_n[i + P]
    assert np.abs(want - direct).max() <= 1e-15
    assert np.all(np.abs(got - direct) <= 2.0 ** -24 * np.abs(direct) + 2.0 * (N + 2) * R.U * np.abs(src[:, P:P + L]).sum(axis=0) / np.sqrt(N))
    assert np.array_equal(got[0], got[1])


def test_integer_and_extreme_delays():
    taps, first = unit_geometry((3, -17))
    assert np.count_nonzero(taps) == 4 and sorted((first + NZ.HW - 1).reshape(-1).tolist()) == [-17, -3, 3, 17]
    got, want, src = check("integer tau", taps, first, 300)
    assert np.abs(want[0] - (src[0, P - 3:P - 3 + 300] + src[1, P + 3:P + 3 + 300]) / np.sqrt(2.0)).max() <= 1e-15
    taps, first = unit_geometry((NZ.MAX_DELAY, -NZ.MAX_DELAY), dirs=((1.0, 0.0, 0.0),))
    assert first.reshape(-1).tolist() == [NZ.MAX_DELAY - NZ.HW + 1, -NZ.MAX_DELAY - NZ.HW + 1]
    # tau = +M: output i reads source i + P - M = i + Hw, and the zero-padded last tap reaches source sample 0 at i = 0;
    # tau = -M: output L - 1 reads source L - 1 + P + M = L + 2 P - 1 - Hw, and the first tap reaches sample L + 2 P - 2
    for L in (1, 257):
        got, want, src = check("tau = +-M", taps, first, L)
        assert np.abs(want[0] - src[0, NZ.HW:NZ.HW + L]).max() <= 1e-15 and np.abs(want[1] - src[0, 2 * P - NZ.HW:2 * P - NZ.HW + L]).max() <= 1e-15
    lowest = np.full_like(first, -P)                                         # the lowest first lag the range admits: tap 0 reads the LAST source sample
    check("first = -P", np.ones_like(taps), lowest, 257)
    check("first = P - W + 1", np.ones_like(taps), np.full_like(first, P - W + 1), 257)      # the highest: tap W - 1 reads source sample 0 at i = 0


def test_first_outside_the_source_range_reads_zeros():
    """the definition: a source index outside [0, L + 2 P) contributes zero -- whatever ``first`` says.  Rows within 128 lags of their wave's largest
    first lag go through the LDS window (zeros stored in it), rows further below it are generated sample by sample with the range test."""
    L, N, D = 300, 5, 2
    taps, first = geometry(D, N)
    taps = np.abs(taps) + 0.01                                               # every tap counts
    first = first.copy()
    first[0, 1] = -P - 5                                                     # five taps beyond the end; shares the window
    first[1, 0] = P + 50                                                     # reads below sample 0; the wave's other row is 193 lags below: per-sample path
    first[2, 0], first[2, 1] = 5000, -100000                                 # nothing of either row lies inside the range
    first[3, 1] = P - W + 40                                                 # partly below sample 0
    key = key_of("a")
    with pytest.raises(ValueError, match="first lag"):
        NZ.noise_bank_hip(taps[None], first[None], key[None], L)
    got, want, src = check("first outside", taps, first, L, check_first=False)
    only = np.zeros_like(taps)
    only[2] = taps[2]
    out = NZ.noise_bank_hip(only[None], first[None], key[None], L, check_first=False)
    assert torch.count_nonzero(out) == 0                                     # wave 2 alone: exact zeros
    assert np.abs(want).max() > 0.1


def test_draw_offset():
    taps, first = geometry(3, 7)
    a, _, _ = check("draw0 = 5", taps, first, 257, draw0=5)
    b, _, _ = check("draw0 = 0", taps, first, 257)
    assert not np.array_equal(a, b)
    tail, _, _ = check("draw0 = 5, waves 5 .. 6", taps[:2], first[:2], 257, draw0=5)
    assert not np.array_equal(tail, b)


def test_rows_are_independent_of_the_batch():
    L = 700
    ta, fa = geometry(3, 9)
    tb, fb = NZ.delay_taps(ring(3, 0.07, angle=1.1), NZ.sphere_directions(9), FS, C)
    ka, kb = key_of("a"), key_of("b")
    both = NZ.noise_bank_hip(np.stack([ta, tb]), np.stack([fa, fb]), np.stack([ka, kb]), L)
    one_a, one_b = NZ.noise_bank_hip(ta[None], fa[None], ka[None], L), NZ.noise_bank_hip(tb[None], fb[None], kb[None], L)
    assert torch.equal(both[0], one_a[0]) and torch.equal(both[1], one_b[0]) and not torch.equal(both[0], both[1])
    twice = NZ.noise_bank_hip(np.stack([ta, ta]), np.stack([fa, fa]), np.stack([ka, ka]), L)
    assert torch.equal(twice[0], twice[1]) and torch.equal(twice[0], one_a[0])
    assert torch.equal(NZ.noise_bank_hip(ta[None], fa[None], ka[None], L), one_a)         # and of the run


def test_diffuse_noise_with_tilt_against_the_float64_chain():
    """tilt -3, D = 3, L = 1000, N = 16: the restatement followed by a float64 FIR.  With x the bank's output (e_x its bound above), h the shaping
    filter and h32 its fp32 rounding, the GPU returns fir32(x_gpu, h32):
        |fir32(x_gpu, h32) - fir64(x_gpu, h32)| <= 1e-5 max |fir64(x_gpu, h32)|     buddy_fir's own bound: tests/test_hip_kernels.py::test_fir_and_adjoint
        |fir64(x_gpu - x_ref, h32)|             <= |h32| * e_x                      the bank's error through the filter
        |fir64(x_ref, h32 - h)|                 <= 2^-24 |h| * |x_ref|              the filter's rounding to fp32
    (* is the convolution), and the transient of M - 1 samples is cut on both sides."""
    D, L, N, tilt = 3, 1000, 16, -3.0
    pos, key = ring(D), key_of("tilt")
    h = NZ.shaping_fir(FS, tilt)
    M = len(h)
    Lg = L + M - 1
    src = gpu_sources(key, NZ.NOISE_FIELD, 0, N, Lg + 2 * P)
    taps, first = NZ.delay_taps(pos, NZ.sphere_directions(N), FS, C)
    x, A = R.noise_bank(taps, first, src, P, Lg, want_abs=True)
    want = R.fir(x, h)[:, M - 1:]
    assert np.abs(want - R.diffuse(pos, key, L, FS, N, tilt=tilt, src=src)).max() == 0.0
    e_x = 2.0 ** -24 * np.abs(x) + R.gamma_bound(N, W, A)
    h32 = h.astype(np.float32).astype(np.float64)
    bound = 1e-5 * np.abs(R.fir(x, h32)).max() + (R.fir(e_x, np.abs(h32)) + 2.0 ** -24 * R.fir(np.abs(x), np.abs(h)))[:, M - 1:]
    got = NZ.diffuse_noise(pos, key[None], L, FS, waves=N, tilt=tilt)
    assert got.shape == (1, D, L) and got.is_contiguous()
    got = got[0].cpu().numpy().astype(np.float64)
    ratio = np.abs(got - want) / bound
    print(f"tilt chain: max |gpu - ref| = {np.abs(got - want).max():.3e}, worst over the bound {ratio.max():.3f}, max |ref| = {np.abs(want).max():.3f}")
    assert np.all(np.abs(got - want) <= bound)
    white = NZ.diffuse_noise(pos, key[None], L, FS, waves=N)
    assert torch.equal(white, NZ.noise_bank_hip(taps[None], first[None], key[None], L))


def test_sensor_noise_is_the_fill():
    keys = np.stack([key_of("a"), key_of("b")])
    out = NZ.sensor_noise(keys, 3, 257)
    assert out.shape == (2, 3, 257) and out.is_contiguous()
    for b in range(2):
        assert np.array_equal(out[b].cpu().numpy().astype(np.float64), gpu_sources(keys[b], NZ.NOISE_SENSOR, 0, 3, 257))


def test_raw_entry_refuses_before_launching():
    """D = 9, W above the maximum and a NaN scale return BUDDY_ERR_ARG with nothing launched: the output keeps its bits"""
    lib = _lib.require_gpu()
    taps, first = geometry(3, 4)
    tt, ft = torch.from_numpy(taps).cuda(), torch.from_numpy(first).cuda()
    kt = torch.from_numpy(key_of("a").reshape(1, 2).view(np.int32).copy()).cuda()
    out = torch.full((1, 3, 100), 7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for D, Wt, scale in ((9, W, 0.5), (3, lib.buddy_noise_max_taps() + 1, 0.5), (3, W, float("nan"))):
        assert lib.buddy_noise_bank(tt.data_ptr(), ft.data_ptr(), kt.data_ptr(), 8, 0, out.data_ptr(), 1, D, 4, Wt, P, 100, scale, st) == 2
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)
