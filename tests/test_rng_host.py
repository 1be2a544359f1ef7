"""CPU: the host side of seeded sampling (buddy_amd/utils/rng.py): the numpy restatement of Philox4x32-10 against the Random123 known answers and the
pinned keys / words of the stream layout, PhiloxStreams bookkeeping (slices, per-purpose counters) on the CPU device, the config defaults, and the
moments of the float64 normals at 5 sigma of their sampling error."""
import numpy as np
import pytest
import torch

from buddy_amd.config import compose
from buddy_amd.utils import rng

N = 1 << 22
KEY0 = (129767252, 798795333)           # stream_key(0, "u0.wav")


def _hex(w):
    return " ".join(f"{int(v):08x}" for v in np.asarray(w).reshape(-1))


def test_philox_known_answers_keys_and_first_words():
    assert _hex(rng.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(rng.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    assert rng.stream_key(0, "u0.wav") == KEY0
    assert rng.stream_key(0, "p226_003.wav") == (725741547, 1453957188)
    assert rng.stream_key(1, "u0.wav") != KEY0
    assert _hex(rng.words(KEY0, 0, 0, 8)) == "8513bde7 cce883e8 eae9e125 6c64a7c6 4d91ef03 7ab7e1f2 b1fe9b75 50d7e6ed"
    # sample i is word i & 3 of block i >> 2: a shorter draw is a prefix of a longer one, and a length that is no multiple of four ends inside a block
    w = rng.words(KEY0, 0, 0, 4099)
    assert w.shape == (4099,) and np.array_equal(w[:8], rng.words(KEY0, 0, 0, 8)) and np.array_equal(w[:1023], rng.words(KEY0, 0, 0, 1023))
    assert np.array_equal(rng.philox4x32_10((1024, 0, 0, 0), KEY0).reshape(-1)[:3], w[4096:])
    # draw and purpose are counter words of their own
    assert not np.array_equal(rng.words(KEY0, 0, 1, 8), w[:8]) and not np.array_equal(rng.words(KEY0, 1, 0, 8), w[:8])


def test_uniform_and_normal_maps():
    w = np.array([0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFF, 0x40000000, 0x80000000, 0xC0000000], dtype=np.uint32)
    u = rng.uniforms_from_words(w)
    assert u[0] == 0.0 and u[2] == 1.0 - 2.0 ** -24 and u[4] == 0.0 and u[5] == 0.25
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)              # exact in fp32
    z = rng.normals_from_words(w)
    assert np.isfinite(z).all()
    assert abs(z[0] - np.sqrt(50 * np.log(2.0))) < 1e-12 and z[1] == 0.0           # u1 = 2^-25, angle 0: the truncated tail, |z| <= 5.887
    assert abs(z[0]) <= rng.Z_MAX * (1 + 1e-15) and abs(rng.Z_MAX - 5.887) < 1e-4 and abs(z[2]) < 4e-4                              # u1 = 1 - 2^-25: radius sqrt(2^-24)
    r = np.sqrt(-2.0 * np.log((0xFF >> 8) * 2.0 ** -24 + 2.0 ** -25))
    assert abs(z[4]) < 1e-12 * r and abs(z[5] - r) < 1e-12 * r                      # a quarter turn: (cos, sin) = (0, 1)
    assert np.array_equal(rng.normals(KEY0, 0, 0, 5), rng.normals(KEY0, 0, 0, 8)[:5])


def test_streams_slices_and_counters():
    names = [f"u{i}.wav" for i in range(5)]
    s = rng.PhiloxStreams(names, 0, "cpu")
    assert len(s) == 5 and np.array_equal(s.keys[0], np.array(KEY0, dtype=np.uint32))
    a0 = s.randn(rng.SAMPLER, (7,))                      # purpose 0, draw 0
    assert a0.shape == (5, 7) and a0.dtype == torch.float32
    assert np.array_equal(a0[0].numpy(), rng.normals(KEY0, 0, 0, 7).astype(np.float32))
    assert np.array_equal(a0[3].numpy(), rng.normals(rng.stream_key(0, "u3.wav"), 0, 0, 7).astype(np.float32))
    u0 = s.rand(rng.PHASES, (2, 3))                      # purpose 1 has a counter of its own: still draw 0
    assert u0.shape == (5, 2, 3) and np.array_equal(u0[0].reshape(-1).numpy(), rng.uniforms(KEY0, 1, 0, 6).astype(np.float32))
    assert s.counters == [1, 1, 0, 0]
    part = s[1:4]                                        # independent object, parent's counters
    assert len(part) == 3 and part.names == names[1:4] and part.counters == [1, 1, 0, 0]
    p1 = part.randn(rng.SAMPLER, (7,))
    assert part.counters == [2, 1, 0, 0] and s.counters == [1, 1, 0, 0]
    a1 = s.randn(rng.SAMPLER, (7,))                      # the parent's own next draw: its rows 1..3 are what the slice drew
    assert torch.equal(a1[1:4], p1) and not torch.equal(a1, a0)
    r = s.randn(rng.RIR_REG, (9,), count=3)             # three draws in one fill
    assert r.shape == (3, 5, 9) and s.counters == [2, 1, 0, 3]
    assert np.array_equal(r[2, 4].numpy(), rng.normals(rng.stream_key(0, "u4.wav"), 3, 2, 9).astype(np.float32))
    assert torch.equal(s.randn(rng.RIR_REG, (9,))[1], torch.from_numpy(rng.normals(rng.stream_key(0, "u1.wav"), 3, 3, 9).astype(np.float32)))
    h = s.randn(rng.UPDATE_H, (4,))
    assert np.array_equal(h[0].numpy(), rng.normals(KEY0, 2, 0, 4).astype(np.float32)) and s.counters == [2, 1, 1, 4]
    # a row's draws do not depend on the rows beside it, and another seed is another stream
    alone = rng.PhiloxStreams(["u3.wav"], 0, "cpu")
    assert torch.equal(alone.randn(rng.SAMPLER, (7,))[0], a0[3])
    assert not torch.equal(rng.PhiloxStreams(["u3.wav"], 1, "cpu").randn(rng.SAMPLER, (7,))[0], a0[3])
    with pytest.raises(TypeError):
        s[0]


class _Net(torch.nn.Module):
    def forward(self, x, c):
        return 0.5 * x


def _tester(overrides=(), tester="blind_dereverberation_BUDDy"):
    from buddy_amd.instantiate import instantiate
    from buddy_amd.testing.tester import Tester
    args = compose(tester=tester, overrides=list(overrides))
    return Tester(args, _Net(), instantiate(args.diff_params), test_set=None, device="cpu", in_training=True)


def test_config_defaults_leave_noise_factory_unset():
    for name in ("blind_dereverberation_BUDDy", "informed_dereverberation_DPS", "only_unconditional", "real_dereverberation_BUDDy"):
        args = compose(tester=name)
        assert args.tester.noise.generator == "torch" and args.tester.noise.seed == 0
        t = _tester(tester=name)
        assert getattr(t, "noise_factory", None) is None and t.sampler.noise is None
    args = compose()
    del args.tester["noise"]                           # a config written before the block existed
    assert rng.factory_from_config(args.tester, "cpu") is None
    t = _tester(["tester.noise.generator=philox", "tester.noise.seed=7"])
    s = t.noise_factory(["u0.wav", "a_c1.wav"])
    assert isinstance(s, rng.PhiloxStreams) and s.seed == 7 and s.names == ["u0.wav", "a_c1.wav"] and len(s) == 2
    assert _tester(["tester.noise.generator=philox"]).noise_factory(["u0.wav"]).seed == 0        # seed read with its default
    outside = lambda names: "outside"
    t.noise_factory = outside                          # a factory set from outside still wins
    assert t.noise_factory(["x"]) == "outside"
    with pytest.raises(ValueError):
        _tester(["tester.noise.generator=mt19937"])


def test_unconditional_sampler_draws_through_the_streams_on_cpu():
    """the plain Euler-Heun sampler on the CPU device with Philox streams: initialize_x is draw 0 of purpose 0, every step takes one more draw whether
    or not gamma is 0, the result does not depend on the rows beside it and repeats for the same seed"""
    ov = ["tester.sampling_params.T=4", "tester.unconditional.num_samples=2", "tester.unconditional.audio_len=33", "tester.noise.generator=philox"]
    t = _tester(ov, tester="only_unconditional")
    a = t.sample_unconditional("unconditional")
    assert a.shape == (2, 33) and torch.isfinite(a).all()
    assert t.sampler.noise.names == ["unconditional_0", "unconditional_1"] and t.sampler.noise.counters == [1 + 4, 0, 0, 0]
    assert torch.equal(_tester(ov, tester="only_unconditional").sample_unconditional("unconditional"), a)
    one = _tester(ov[:1] + ["tester.unconditional.num_samples=1"] + ov[2:], tester="only_unconditional").sample_unconditional("unconditional")
    assert torch.equal(one[0], a[0])
    other = _tester(ov + ["tester.noise.seed=1"], tester="only_unconditional").sample_unconditional("unconditional")
    assert not torch.equal(other, a)


@pytest.fixture(scope="module")
def z():
    return rng.normals(KEY0, 0, 0, N)


def test_normal_moments_at_five_sigma(z):
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.887
    m, v = z.mean(), z.var()
    k = ((z - m) ** 4).mean() / v ** 2
    print(f"mean {m:.3e} (bound {5 / np.sqrt(N):.3e}), var - 1 {v - 1:.3e} ({5 * np.sqrt(2 / N):.3e}), kurtosis - 3 {k - 3:.3e} ({5 * np.sqrt(24 / N):.3e})")
    assert abs(m) <= 5 / np.sqrt(N)
    assert abs(v - 1) <= 5 * np.sqrt(2 / N)
    assert abs(k - 3) <= 5 * np.sqrt(24 / N)
    for lag in (1, 2, 4):
        c = (z[:-lag] * z[lag:]).mean()
        print(f"lag {lag}: {c:.3e}")
        assert abs(c) <= 5 / np.sqrt(N), lag


def test_normal_streams_are_uncorrelated(z):
    for what, other in (("draw 1", rng.normals(KEY0, 0, 1, N)), ("u1.wav", rng.normals(rng.stream_key(0, "u1.wav"), 0, 0, N))):
        c = ((z - z.mean()) * (other - other.mean())).mean() / (z.std() * other.std())
        print(f"correlation with {what}: {c:.3e} (bound {5 / np.sqrt(N):.3e})")
        assert abs(c) <= 5 / np.sqrt(N), what
