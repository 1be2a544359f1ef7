"""GPU: real recordings end to end (tester mode `real_blind_dereverberation`): wavs of several rates, channel counts and lengths -> the command
line -> resampler, pooled chunk batches, blind sampler, cross-fade, resampler -> a wav tree at the input's rate and length.  Small network,
3 steps.  Plus: pooling chunks of several files into one batch changes no file's result, and with the sampler replaced by the identity the
plumbing around it (scaling, chunking, cross-fade, both resamplers) returns the input."""
import math
import os
import zlib

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

OVERRIDES = ["tester.sampling_params.T=3", "tester.posterior_sampling.blind_hp.op_updates_per_step=2",
             "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "tester.real_recordings.chunk_seconds=1.024",
             "tester.real_recordings.overlap_seconds=0.128", "network.nf=32"]
#        name  rate   seconds  channels  dtype
FILES = [("A", 48000, 2.5, 1, np.float32), ("B", 44100, 1.9, 2, np.int16), ("C", 16000, 0.7, 1, np.float32), ("D", 16000, 0.05, 1, np.float32)]


def oracle(x, up, down, h):
    """float64 scipy with the same taps (scipy multiplies a given window by `up` itself)"""
    return signal.resample_poly(np.asarray(x, np.float64), up, down, axis=-1, window=np.asarray(h, np.float64) / up, padtype="constant")


def bound(h, up, xmax):
    """the resampler's elementwise fp32 bound, derived in tests/test_hip_resample.py"""
    T = math.ceil(len(h) / up)
    S = max(np.abs(h[p::up]).sum() for p in range(up))
    return (T + 3) * 2.0 ** -23 * S * xmax


def _reverberant(u, n):
    from buddy_amd.synth import synth_clean, synth_rir
    y = signal.fftconvolve(synth_clean(u, n).astype(np.float64), synth_rir(u, 2000).astype(np.float64))[:n]
    return 0.3 * y / np.abs(y).max()


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    """the four input files -> (folder, {name: (rate, samples)})"""
    root = tmp_path_factory.mktemp("recordings")
    info = {}
    for u, (name, fs, sec, ch, dt) in enumerate(FILES):
        n = int(round(sec * fs))
        y = _reverberant(u, n)
        if ch == 2:
            y = np.stack([y, 0.5 * np.roll(y, 7)], axis=1)
        wavfile.write(root / f"{name}.wav", fs, (y * 32767).astype(np.int16) if dt == np.int16 else y.astype(np.float32))
        info[name] = (fs, n)
    return str(root), info


def _cli(tmp_path, data, extra=()):
    import test as cli
    out = str(tmp_path / "exp")
    tester = cli.main(["--config-name=conf_VCTK.yaml", "tester=real_dereverberation_BUDDy", *OVERRIDES, f"model_dir={out}", "+gpu=0",
                       f"dset.test.path={data}", "+batch_size=4", "tester.overriden_name=run", "+allow_random_init=true", *extra])
    return tester, os.path.join(out, "run", "real_blind_dereverberation", "VCTK_16k_4s_time")


def _read(path):
    sr, a = wavfile.read(path)
    assert a.dtype == np.float32 and a.ndim == 1
    return sr, a


def test_cli_end_to_end(tmp_path, recordings):
    data, info = recordings
    tester, base = _cli(tmp_path, data)
    assert tester.skipped == ["D.wav"]
    assert sorted(os.listdir(base)) == [".argv", "degraded", "estimated_rir", "reconstructed"]
    assert sorted(os.listdir(os.path.join(base, "reconstructed"))) == ["A.wav", "B.wav", "C.wav"]
    assert sorted(os.listdir(os.path.join(base, "degraded"))) == ["A.wav", "B.wav", "C.wav"]
    assert sorted(os.listdir(os.path.join(base, "estimated_rir"))) == ["A_c0.wav", "A_c1.wav", "A_c2.wav", "B_c0.wav", "B_c1.wav", "C_c0.wav"]
    for name in "ABC":
        fs, n = info[name]
        sr, a = _read(os.path.join(base, "reconstructed", name + ".wav"))
        assert sr == fs and len(a) == n                                    # the input's rate and exactly its sample count
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        sr, d = _read(os.path.join(base, "degraded", name + ".wav"))
        assert sr == 16000 and len(d) == math.ceil(n * 16000 / fs)
        assert abs(d.std() - 0.05) < 1e-3 * 0.05                            # gain * scaling_factor * y / std(y)
    for f in os.listdir(os.path.join(base, "estimated_rir")):
        sr, r = _read(os.path.join(base, "estimated_rir", f))
        assert sr == 16000 and np.isfinite(r).all() and np.abs(r).max() > 0


def test_cli_output_rate_model(tmp_path, recordings):
    data, info = recordings
    tester, base = _cli(tmp_path, data, ["tester.real_recordings.output_rate=model", "dset.test.num_examples=2"])
    assert tester.skipped == [] and sorted(os.listdir(os.path.join(base, "reconstructed"))) == ["A.wav", "B.wav"]
    for name in "AB":
        fs, n = info[name]
        sr, a = _read(os.path.join(base, "reconstructed", name + ".wav"))
        up, down = 16000 // math.gcd(fs, 16000), fs // math.gcd(fs, 16000)
        assert sr == 16000 and len(a) == math.ceil(n * up / down)
        assert np.isfinite(a).all() and np.abs(a).max() > 0


def _tester(data, extra=(), batch_size=4):
    from buddy_amd.config import compose
    from buddy_amd.datasets.recordings import AudioFolder
    from buddy_amd.instantiate import instantiate
    from buddy_amd.synth import synth_state_dict
    from buddy_amd.testing.tester import Tester
    args = compose(tester="real_dereverberation_BUDDy", overrides=OVERRIDES + list(extra))
    net = instantiate(args.network)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(3, 32).items()})
    net = net.cuda().eval()
    return Tester(args, net, instantiate(args.diff_params), test_set=AudioFolder(path=data), device="cuda", in_training=True, batch_size=batch_size)


def test_pooling_changes_nothing(recordings):
    """chunks of A, B (one pool: batches of 4 and 1) and C, each with a noise stream seeded from its own name: every file's result equals the run that
    samples one chunk at a time, within the bound tests/test_hip_cli.py::test_harness_ragged_utterance_lengths holds a batched run to
    (guidance normalisation amplifies round-off)"""
    from oracle.sampler_ref import NoiseStream
    data, _ = recordings
    names = []

    def run(batch_size):
        t = _tester(data, batch_size=batch_size)
        t.noise_factory = lambda ns: [names.append(n) or NoiseStream(zlib.crc32(n.encode()) % 100000) for n in ns]
        t.test_real_recordings("real_blind_dereverberation")
        return dict(t.results)

    pooled = run(4)
    assert names == ["A_c0.wav", "A_c1.wav", "A_c2.wav", "B_c0.wav", "B_c1.wav", "C_c0.wav"]      # file-then-chunk order, one name per chunk
    single = run(1)
    assert sorted(pooled) == sorted(single) == ["A", "B", "C"]
    for k in "ABC":
        a, b = pooled[k].double(), single[k].double()
        rel = float((a - b).abs().max() / b.abs().max())
        print(f"pooled vs one chunk at a time, {k}: {rel:.3e}")
        assert a.shape == b.shape and torch.isfinite(a).all()
        assert rel < 1e-3


def test_plumbing_is_the_identity(recordings):
    """sampler := identity, no level match: what is left is scaling, chunking, the cross-fade (a partition of unity), the scaling undone and the
    two resamplers"""
    from buddy_amd.utils.resample import design_filter
    data, info = recordings
    t = _tester(data, ["tester.posterior_sampling.constraint_speech_magnitude.use=false", "tester.sub_batches=1"])

    def identity(y, operator, shape=None, blind=False, **kw):
        t.sampler.operator = operator
        return y.clone()

    t.sampler.predict_conditional = identity
    t.test_real_recordings("real_blind_dereverberation")
    res = dict(t.results)
    _, c = wavfile.read(os.path.join(data, "C.wav"))
    assert res["C"].shape == c.shape
    assert np.abs(res["C"].numpy().astype(np.float64) - c).max() <= 1e-6 * np.abs(c).max()
    _, a = wavfile.read(os.path.join(data, "A.wav"))
    hd, hu = design_filter(1, 3), design_filter(3, 1)
    r1 = oracle(a, 1, 3, hd)
    r2 = oracle(r1, 3, 1, hu)[:len(a)]
    tol = bound(hd, 1, np.abs(a).max()) + bound(hu, 3, np.abs(r1).max())
    err = np.abs(res["A"].numpy().astype(np.float64) - r2).max()
    print(f"A 48 kHz down-then-up: max|err| {err:.3e}  bound {tol:.3e}")
    assert res["A"].shape == a.shape and err <= tol
