"""GPU: the Philox noise kernels (csrc/rng.hip: buddy_philox_fill, buddy_perturb_philox) against the host restatement of buddy_amd/utils/rng.py.
Words and uniforms bit for bit at lengths around the four-sample block and the 1024-sample workgroup, with and without 16-byte alignment, inside
guard-filled buffers; normals against the float64 Box-Muller of the same words; a stream's samples independent of the shape of the fill; the fused
perturbation equal to buddy_perturb of the filled noise bit for bit."""
import numpy as np
import pytest
import torch

from buddy_amd import _lib
from buddy_amd.utils import rng

pytestmark = pytest.mark.gpu

NAMES = ["u0.wav", "u1.wav", "p226_003.wav"]
GUARD = -1234.5
PAD = 64                      # floats of guard either side (256 bytes: the carved buffer keeps the allocation's alignment unless `shift` moves it)
N_ACC = 1 << 22
# max |z_gpu - z_float64| over the 2^22 samples of (0, "u0.wav"), purpose 0, draw 0, measured on the MI355X (profiles/rng_accuracy.txt)
MEASURED_MAX_ERR = 7.011e-07
# 4 x the measured maximum (a sample maximum of ulp-level errors understates the worst case), and in no case above 1e-5 = 5.9 x a handful of 2^-23:
# more would mean a fast intrinsic crept in
ERR_BOUND = min(4.0 * MEASURED_MAX_ERR, 1e-5)        # 2.80e-06


def _keys(names, seed=0):
    k = np.array([rng.stream_key(seed, n) for n in names], dtype=np.uint32)
    return k, torch.from_numpy(k.view(np.int32).copy()).cuda()


def _fill(names, R, n, purpose, draw0, kind, shift=0):
    """buddy_philox_fill into an (R, B, n) window of a guard-filled buffer that starts ``shift`` floats off the 16-byte grid -> (window, keys); the
    guards either side are checked here"""
    k, kd = _keys(names)
    B, total = len(names), R * len(names) * n
    buf = torch.full((PAD + shift + total + PAD,), GUARD, dtype=torch.float32, device="cuda")
    out = buf[PAD + shift:PAD + shift + total]
    assert (out.data_ptr() % 16 == 0) == (shift % 4 == 0)
    _lib.check(_lib.require_gpu().buddy_philox_fill(out.data_ptr(), R, B, n, kd.data_ptr(), purpose, draw0, kind, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((buf[:PAD + shift] == GUARD).all()) and bool((buf[PAD + shift + total:] == GUARD).all()), "wrote outside out[0 .. R * B * n)"
    return out.reshape(R, B, n).clone(), k


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, 4099])
def test_raw_words_equal_host_bit_for_bit(n, shift):
    for purpose, draw0 in ((0, 0), (3, 7)):
        out, k = _fill(NAMES, 2, n, purpose, draw0, rng.RAW, shift)
        got = _bits(out)
        for r in range(2):
            for b in range(3):
                assert np.array_equal(got[r, b], rng.words(k[b], purpose, draw0 + r, n)), (n, shift, purpose, r, b)


@pytest.mark.parametrize("n,shift", [(5, 0), (1024, 0), (1024, 2), (4099, 0)])
def test_uniforms_equal_host_bit_for_bit(n, shift):
    out, k = _fill(NAMES, 2, n, 1, 0, rng.UNIFORM, shift)
    got = out.cpu().numpy()
    assert got.min() >= 0.0 and got.max() < 1.0
    for r in range(2):
        for b in range(3):
            assert np.array_equal(got[r, b], rng.uniforms(k[b], 1, r, n).astype(np.float32)), (n, shift, r, b)


@pytest.fixture(scope="module")
def acc():
    """the 2^22 normals of (0, "u0.wav"), purpose 0, draw 0: (GPU values, float64 Box-Muller of the same words, the words)"""
    out, k = _fill(["u0.wav"], 1, N_ACC, 0, 0, rng.NORMAL)
    return out.reshape(-1).cpu().numpy(), rng.normals(k[0], 0, 0, N_ACC), rng.words(k[0], 0, 0, N_ACC)


def test_normals_against_float64_box_muller(acc):
    """no NaN / inf, |z| <= 5.887, and within ERR_BOUND of the float64 Box-Muller of the same words"""
    z, ref, _ = acc
    assert np.isfinite(z).all()
    err = float(np.abs(z.astype(np.float64) - ref).max())
    print(f"normals: max |z| {np.abs(z).max():.4f}, max |gpu - float64| over 2^22 samples {err:.3e} (bound {ERR_BOUND:.3e})")
    assert np.abs(z).max() <= 5.887
    assert err <= ERR_BOUND, err
    # the per-element store path (odd length, misaligned rows) gives the same values
    odd, k3 = _fill(NAMES, 2, 4099, 2, 1, rng.NORMAL, shift=3)
    for r in range(2):
        for b in range(3):
            assert np.abs(odd[r, b].cpu().numpy().astype(np.float64) - rng.normals(k3[b], 2, 1 + r, 4099)).max() <= ERR_BOUND


def test_normals_where_u1_is_close_to_one(acc):
    """u1 = (k + 0.5) 2^-24 is not an fp32 number for k >= 2^23; rounded to fp32 it would put the radius off by up to 2.4e-4 where u1 -> 1.  The
    kernel takes the logarithm from 1 - u1 there, which is exact: the samples with u1 > 1 - 2^-12 (radius below 0.0221) meet the same bound."""
    z, ref, w = acc
    near_one = np.repeat((w[0::2] >> 8) >= (1 << 24) - 4096, 2)
    assert near_one.sum() >= 256
    err = float(np.abs(z.astype(np.float64) - ref)[near_one].max())
    print(f"normals with u1 > 1 - 2^-12: {int(near_one.sum())} samples, max |gpu - float64| {err:.3e}")
    assert err <= ERR_BOUND and np.abs(ref[near_one]).max() < 0.0222


def test_samples_do_not_depend_on_the_shape_of_the_fill():
    names = [f"v{i}.wav" for i in range(5)] + ["u0.wav", "v6.wav", "v7.wav"]
    big = rng.PhiloxStreams(names, 0, "cuda")
    a = big.randn(rng.SAMPLER, (64000,))
    one = rng.PhiloxStreams(["u0.wav"], 0, "cuda").randn(rng.SAMPLER, (1000,))
    assert a.shape == (8, 64000) and one.shape == (1, 1000)
    assert torch.equal(one[0], a[5, :1000])
    # a slice draws what the parent's rows draw, from the parent's counters, through the same device keys
    part = big[4:7]
    p = part.randn(rng.SAMPLER, (1001,))
    full = big.randn(rng.SAMPLER, (1001,))
    assert big.counters[0] == 2 and part.counters[0] == 2 and torch.equal(p, full[4:7]) and not torch.equal(full[5, :1000], a[5, :1000])
    # several draws in one launch = the draws one at a time
    s1, s2 = rng.PhiloxStreams(names[:3], 3, "cuda"), rng.PhiloxStreams(names[:3], 3, "cuda")
    three = s1.randn(rng.RIR_REG, (13825,), count=3)
    for r in range(3):
        assert torch.equal(three[r], s2.randn(rng.RIR_REG, (13825,)))
    u = s1.rand(rng.PHASES, (513, 100))
    assert u.shape == (3, 513, 100) and float(u.min()) >= 0.0 and float(u.max()) < 1.0


@pytest.mark.parametrize("L", [1025, 8192])
def test_fused_perturb_equals_perturb_of_the_fill_bit_for_bit(L):
    from buddy_amd.testing import _hipops
    B, scale = 3, 0.37
    x = torch.from_numpy(np.random.RandomState(L).standard_normal((B, L)).astype(np.float32)).cuda()
    a, b = rng.PhiloxStreams(NAMES, 0, "cuda"), rng.PhiloxStreams(NAMES, 0, "cuda")
    for s in (a, b):
        s.randn(rng.SAMPLER, (L,))                      # draw 0 = initialize_x: the steps start at draw 1
    for step in range(2):
        fused = a.perturb(x, scale)
        eps = b.randn(rng.SAMPLER, (L,))
        want = _hipops.perturb(x, eps, scale)
        assert torch.equal(fused, want), (L, step, float((fused - want).abs().max()))
        assert np.abs(eps[0].cpu().numpy().astype(np.float64) - rng.normals(a.keys[0], 0, 1 + step, L)).max() <= ERR_BOUND
    assert a.counters == b.counters == [3, 0, 0, 0]
    # bounds: the C entry on a window of a guard-filled buffer, aligned and not
    k, kd = _keys(NAMES)
    for shift in (0, 1):
        buf = torch.full((PAD + shift + B * L + PAD,), GUARD, dtype=torch.float32, device="cuda")
        out = buf[PAD + shift:PAD + shift + B * L]
        _lib.check(_lib.require_gpu().buddy_perturb_philox(_lib.ptr(x), kd.data_ptr(), 2, scale, out.data_ptr(), B, L, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((buf[:PAD + shift] == GUARD).all()) and bool((buf[PAD + shift + B * L:] == GUARD).all())
        assert torch.equal(out.reshape(B, L), fused)


def test_bad_arguments_are_refused():
    _, kd = _keys(NAMES)
    out = torch.empty(3 * 8, device="cuda")
    lib = _lib.require_gpu()
    for args in ((out.data_ptr(), 1, 3, 8, kd.data_ptr(), 0, 0, 3), (out.data_ptr(), 0, 3, 8, kd.data_ptr(), 0, 0, 0), (out.data_ptr(), 1, 3, 0, kd.data_ptr(), 0, 0, 0),
                 (None, 1, 3, 8, kd.data_ptr(), 0, 0, 0), (out.data_ptr(), 1, 3, 8, None, 0, 0, 0)):
        with pytest.raises(_lib.BuddyHipError):
            _lib.check(lib.buddy_philox_fill(*args, _lib.stream_ptr()))
    with pytest.raises(_lib.BuddyHipError):
        _lib.check(lib.buddy_perturb_philox(None, kd.data_ptr(), 0, 1.0, out.data_ptr(), 3, 8, _lib.stream_ptr()))
