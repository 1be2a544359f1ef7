"""GPU: the multichannel WPE front end of the real-recordings mode (``tester.real_recordings.channels``), and simulated microphone arrays
(``tools/make_paired_set.py --mics``).  The pattern of tests/test_hip_real_recordings.py: nf = 32, T = 3, short chunks; where the plumbing is
the subject the sampler is replaced by the identity, so a file's result is what the sampler observed."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wpe_mc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

OVERRIDES = ["tester.sampling_params.T=3", "tester.posterior_sampling.blind_hp.op_updates_per_step=2",
             "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "tester.real_recordings.chunk_seconds=1.024",
             "tester.real_recordings.overlap_seconds=0.128", "network.nf=32"]
#        name  rate   seconds  channels
FILES = [("A", 16000, 1.5, 3), ("B", 44100, 1.2, 2), ("C", 16000, 1.1, 1)]


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    """the three input files -> (folder, {name: (rate, samples, (C, n) float32 as written)})"""
    root = tmp_path_factory.mktemp("array_recordings")
    info = {}
    for u, (name, fs, sec, ch) in enumerate(FILES):
        n = int(round(sec * fs))
        y = ref.mc_input(u, n, ch)
        y = (0.3 * y / np.abs(y).max()).astype(np.float32)
        wavfile.write(root / f"{name}.wav", fs, y[0] if ch == 1 else np.ascontiguousarray(y.T))
        info[name] = (fs, n, y)
    return str(root), info


def _identity_run(data, extra):
    from buddy_amd.config import compose
    from buddy_amd.datasets.recordings import AudioFolder
    from buddy_amd.instantiate import instantiate
    from buddy_amd.synth import synth_state_dict
    from buddy_amd.testing.tester import Tester
    args = compose(tester="real_dereverberation_BUDDy", overrides=OVERRIDES + ["tester.posterior_sampling.constraint_speech_magnitude.use=false",
                                                                               "tester.sub_batches=1"] + list(extra))
    net = instantiate(args.network)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(3, 32).items()})
    t = Tester(args, net.cuda().eval(), instantiate(args.diff_params), test_set=AudioFolder(path=data), device="cuda", in_training=True, batch_size=4)

    def identity(y, operator, shape=None, blind=False, **kw):
        t.sampler.operator = operator
        return y.clone()

    t.sampler.predict_conditional = identity
    return t


def test_front_end_through_the_tester(recordings):
    from oracle import wpe_ref
    data, info = recordings
    # channels = wpe: the reference channel of MC-WPE on all channels is what the sampler observes
    t = _identity_run(data, ["tester.real_recordings.channels=wpe"])
    t.test_real_recordings("real_blind_dereverberation")
    res = dict(t.results)
    assert t.skipped == [] and sorted(res) == ["A", "B", "C"]
    fs, n, y = info["A"]
    want = ref.signal(wpe_ref.wpe(ref.spectrum(y), taps=10, delay=3, iterations=3), n)[0]
    e = ref.rel(res["A"].numpy(), want)
    print(f"channels=wpe, A (3 channels, 16 kHz): result vs oracle's reference channel {e:.2e}")
    assert res["A"].shape == (n,) and e < 1e-4
    for k in "BC":
        assert res[k].shape == (info[k][1],) and torch.isfinite(res[k]).all() and float(res[k].abs().max()) > 0
    # another reference channel of the WPE result
    t = _identity_run(data, ["tester.real_recordings.channels=wpe", "tester.real_recordings.reference_channel=2", "tester.real_recordings.wpe.taps=4"])
    t.test_real_recordings("real_blind_dereverberation")
    assert sorted(t.skipped) == ["B.wav", "C.wav"]                                            # fewer than three channels
    want = ref.signal(wpe_ref.wpe(ref.spectrum(y), taps=4, delay=3, iterations=3), n)[2]
    assert ref.rel(dict(t.results)["A"].numpy(), want) < 1e-4
    # channels = reference
    t = _identity_run(data, ["tester.real_recordings.channels=reference", "tester.real_recordings.reference_channel=1"])
    t.test_real_recordings("real_blind_dereverberation")
    res = dict(t.results)
    assert t.skipped == ["C.wav"] and sorted(res) == ["A", "B"]                               # the mono file has no channel 1
    assert np.abs(res["A"].numpy().astype(np.float64) - y[1]).max() <= 1e-6 * np.abs(y[1]).max()
    assert res["B"].shape == (info["B"][1],) and torch.isfinite(res["B"]).all()
    # channels = mean: the path of before, and not one unmixed read
    t = _identity_run(data, ["tester.real_recordings.channels=mean"])
    t.test_set.channels = None
    t.test_real_recordings("real_blind_dereverberation")
    res = dict(t.results)
    mean = np.mean(y.astype(np.float64).T, axis=1)
    assert t.skipped == [] and np.abs(res["A"].numpy().astype(np.float64) - mean).max() <= 1e-6 * np.abs(mean).max()


def test_too_short_and_too_wide_files(tmp_path):
    """a file with fewer frames than channels x taps + delay is processed as its reference channel; one the kernel cannot take is skipped"""
    rs = np.random.RandomState(5)
    a = (0.1 * rs.standard_normal((2, 12000))).astype(np.float32)                             # 97 frames < 2 * 48 + 3
    wavfile.write(tmp_path / "short.wav", 16000, np.ascontiguousarray(a.T))
    wavfile.write(tmp_path / "wide.wav", 16000, (0.1 * rs.standard_normal((12000, 9))).astype(np.float32))
    t = _identity_run(str(tmp_path), ["tester.real_recordings.channels=wpe", "tester.real_recordings.wpe.taps=48"])
    t.test_real_recordings("real_blind_dereverberation")
    assert t.skipped == ["wide.wav"]
    assert np.abs(dict(t.results)["short"].numpy() - a[0]).max() <= 1e-6 * np.abs(a[0]).max()


def _cli(tmp_path, data, extra=()):
    import test as cli
    out = str(tmp_path / "exp")
    tester = cli.main(["--config-name=conf_VCTK.yaml", "tester=real_dereverberation_BUDDy", *OVERRIDES, f"model_dir={out}", "+gpu=0",
                       f"dset.test.path={data}", "+batch_size=4", "tester.overriden_name=run", "+allow_random_init=true", *extra])
    return tester, os.path.join(out, "run", "real_blind_dereverberation", "VCTK_16k_4s_time")


def test_cli_with_the_front_end(tmp_path, recordings):
    data, info = recordings
    tester, base = _cli(tmp_path / "wpe", data, ["tester.real_recordings.channels=wpe"])
    assert tester.skipped == []
    assert sorted(os.listdir(base)) == [".argv", "degraded", "estimated_rir", "reconstructed", "wpe"]
    for sub in ("degraded", "wpe", "reconstructed"):
        assert sorted(os.listdir(os.path.join(base, sub))) == ["A.wav", "B.wav", "C.wav"]
    rirs = sorted(os.listdir(os.path.join(base, "estimated_rir")))
    assert sorted({f.split("_c")[0] for f in rirs}) == ["A", "B", "C"] and all(f.endswith(".wav") and "_c" in f for f in rirs)
    for name in "ABC":
        fs, n, y = info[name]
        sr, a = wavfile.read(os.path.join(base, "reconstructed", name + ".wav"))
        assert sr == fs and a.shape == (n,) and a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0
        sr, d = wavfile.read(os.path.join(base, "degraded", name + ".wav"))
        sr2, w = wavfile.read(os.path.join(base, "wpe", name + ".wav"))
        assert sr == sr2 == 16000 and d.shape == w.shape == (math.ceil(n * 16000 / fs),) and np.isfinite(w).all()
        assert abs(w.std() - 0.05) < 1e-3 * 0.05                                              # the observed signal carries the scaling rule
        assert not np.array_equal(d, w)
    _, d = wavfile.read(os.path.join(base, "degraded", "A.wav"))                               # the reference channel as recorded, with the file's gain
    y0 = info["A"][2][0].astype(np.float64)
    g = float(np.dot(d, y0) / np.dot(y0, y0))
    assert np.abs(d - g * y0).max() <= 1e-5 * np.abs(d).max()
    # a default run has no wpe/
    tester, base = _cli(tmp_path / "default", data, ["dset.test.num_examples=1"])
    assert sorted(os.listdir(base)) == [".argv", "degraded", "estimated_rir", "reconstructed"]


def test_simulated_arrays(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_paired_set
    from buddy_amd.synth import synth_clean
    clean = tmp_path / "clean" / "p1"
    os.makedirs(clean)
    for u in range(2):
        wavfile.write(clean / f"u{u}.wav", 16000, synth_clean(u, 8000))
    common = ["--clean", str(tmp_path / "clean"), "--rir-seconds", "0.2", "--max-order", "3", "--reverberant", "--seed", "4"]
    rows = make_paired_set.main(common + ["--out", str(tmp_path / "arr"), "--mics", "3"])
    assert [r["mics"] for r in rows] == [3, 3] and all(r["array_radius"] == 0.1 and 0.0 <= r["array_angle"] < 2 * math.pi for r in rows)
    assert rows[0]["array_angle"] != rows[1]["array_angle"]
    for u in range(2):
        fs, h = wavfile.read(tmp_path / "arr" / "rir_array" / "p1" / f"u{u}.wav")
        fs1, h0 = wavfile.read(tmp_path / "arr" / "rir" / "p1" / f"u{u}.wav")
        assert fs == fs1 == 16000 and h.shape == (3200, 3) and h0.shape == (3200,) and h.dtype == h0.dtype == np.float32
        assert np.array_equal(h[:, 0], h0) and not np.array_equal(h[:, 1], h0) and np.abs(h).max(axis=0).min() > 0
        fs, y = wavfile.read(tmp_path / "arr" / "reverberant" / "p1" / f"u{u}.wav")
        assert fs == 16000 and y.shape == (8000, 3) and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max(axis=0).min() > 0
    # --mics 1 is the run without the flag, byte for byte
    make_paired_set.main(common + ["--out", str(tmp_path / "one"), "--mics", "1"])
    make_paired_set.main(common + ["--out", str(tmp_path / "none")])
    listing = lambda d: sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs_ in os.walk(d) for f in fs_)
    assert listing(tmp_path / "one") == listing(tmp_path / "none") and "rooms.csv" in listing(tmp_path / "one")
    assert not any(f.startswith("rir_array") for f in listing(tmp_path / "one"))
    for f in listing(tmp_path / "one"):
        assert open(tmp_path / "one" / f, "rb").read() == open(tmp_path / "none" / f, "rb").read(), f
    with pytest.raises(SystemExit):
        make_paired_set.main(common + ["--out", str(tmp_path / "bad"), "--mics", "3", "--bands"])
