"""GPU: the wMPDR beamformer behind the multichannel WPE front end of the real-recordings mode (``tester.real_recordings.beamformer``) and of
``tools/wpe.py --beamformer wmpdr``.  The pattern of tests/test_hip_wpe_mc_recordings.py: nf = 32, T = 3, short chunks; where the plumbing is
the subject the sampler is replaced by the identity, so a file's result is what the sampler observed."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mpdr_ref as bf  # noqa: E402
import _wpe_mc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

OVERRIDES = ["tester.sampling_params.T=3", "tester.posterior_sampling.blind_hp.op_updates_per_step=2",
             "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "tester.real_recordings.chunk_seconds=1.024",
             "tester.real_recordings.overlap_seconds=0.128", "network.nf=32"]
#        name  rate   seconds  channels
FILES = [("A", 16000, 1.5, 3), ("C", 16000, 1.1, 1)]
BF = ["tester.real_recordings.channels=wpe", "tester.real_recordings.beamformer.use=true"]


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    """the input files -> (folder, {name: (rate, samples, (C, n) float32 as written)})"""
    root = tmp_path_factory.mktemp("array_recordings_bf")
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


def test_beamformer_through_the_tester(recordings):
    from oracle import wpe_ref
    data, info = recordings
    t = _identity_run(data, BF)
    t.test_real_recordings("real_blind_dereverberation")
    res = dict(t.results)
    assert t.skipped == [] and sorted(res) == ["A", "C"]
    fs, n, y = info["A"]
    want = bf.signal(bf.mpdr(wpe_ref.wpe(ref.spectrum(y), taps=10, delay=3, iterations=3)), n)
    e = ref.rel(res["A"].numpy(), want)
    print(f"channels=wpe beamformer.use=true, A (3 channels): result vs the restatement's chain {e:.2e}")
    assert res["A"].shape == (n,) and e < 1e-4
    # the mono file: D = 1 is a copy of the WPE result
    plain = _identity_run(data, ["tester.real_recordings.channels=wpe"])
    plain.test_real_recordings("real_blind_dereverberation")
    other = dict(plain.results)
    assert torch.equal(res["C"], other["C"]) and not torch.equal(res["A"], other["A"])
    # the beamformer needs the WPE output of all channels
    t = _identity_run(data, ["tester.real_recordings.channels=mean", "tester.real_recordings.beamformer.use=true"])
    with pytest.raises(AssertionError, match="channels: wpe"):
        t.test_real_recordings("real_blind_dereverberation")
    assert t.results == []


def _cli(tmp_path, data, extra=()):
    import test as cli
    out = str(tmp_path / "exp")
    tester = cli.main(["--config-name=conf_VCTK.yaml", "tester=real_dereverberation_BUDDy", *OVERRIDES, f"model_dir={out}", "+gpu=0",
                       f"dset.test.path={data}", "+batch_size=4", "tester.overriden_name=run", "+allow_random_init=true", *extra])
    return tester, os.path.join(out, "run", "real_blind_dereverberation", "VCTK_16k_4s_time")


def test_cli_with_the_beamformer(tmp_path, recordings):
    data, info = recordings
    tester, base = _cli(tmp_path / "bf", data, BF)
    assert tester.skipped == []
    assert sorted(os.listdir(base)) == [".argv", "degraded", "estimated_rir", "reconstructed", "wpe"]
    tester, base0 = _cli(tmp_path / "wpe", data, ["tester.real_recordings.channels=wpe"])
    for sub in ("degraded", "wpe", "reconstructed"):
        assert sorted(os.listdir(os.path.join(base, sub))) == sorted(os.listdir(os.path.join(base0, sub))) == ["A.wav", "C.wav"]
    sr, w = wavfile.read(os.path.join(base, "wpe", "A.wav"))
    sr0, w0 = wavfile.read(os.path.join(base0, "wpe", "A.wav"))
    assert sr == sr0 == 16000 and w.shape == w0.shape == (info["A"][1],) and np.isfinite(w).all() and not np.array_equal(w, w0)
    assert abs(w.std() - 0.05) < 1e-3 * 0.05                                                  # the observed signal carries the scaling rule
    _, d = wavfile.read(os.path.join(base, "degraded", "A.wav"))                               # the reference channel as recorded, with the file's gain
    y0 = info["A"][2][0].astype(np.float64)
    g = float(np.dot(d, y0) / np.dot(y0, y0))
    assert np.abs(d - g * y0).max() <= 1e-5 * np.abs(d).max()
    # a default run lists the folders of before
    tester, base = _cli(tmp_path / "default", data, ["dset.test.num_examples=1"])
    assert sorted(os.listdir(base)) == [".argv", "degraded", "estimated_rir", "reconstructed"]


def test_tool_with_the_beamformer(tmp_path, monkeypatch):
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    import importlib.util
    import make_paired_set
    spec = importlib.util.spec_from_file_location("wpe_tool", os.path.join(tools, "wpe.py"))      # not ``import wpe``: the name is taken in the package
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from buddy_amd.synth import synth_clean
    from buddy_amd.utils import wpe as W
    clean = tmp_path / "clean" / "p1"
    os.makedirs(clean)
    for u in range(2):
        wavfile.write(clean / f"u{u}.wav", 16000, synth_clean(u, 8000))
    make_paired_set.main(["--clean", str(tmp_path / "clean"), "--rir-seconds", "0.2", "--max-order", "3", "--reverberant", "--seed", "4", "--out",
                          str(tmp_path / "arr"), "--mics", "3"])
    src = str(tmp_path / "arr" / "reverberant")
    written = tool.main([src, "--out", str(tmp_path / "bf"), "--taps", "4", "--beamformer", "wmpdr", "--channel", "1"])
    assert [os.path.relpath(p, tmp_path / "bf") for p in written] == [os.path.join("p1", "u0.wav"), os.path.join("p1", "u1.wav")]
    fs, y = wavfile.read(os.path.join(src, "p1", "u0.wav"))
    fs1, z = wavfile.read(written[0])
    assert fs1 == fs == 16000 and z.shape == (8000,) and z.dtype == np.float32 and np.isfinite(z).all() and np.abs(z).max() > 0
    want = W.wpe_mc_mpdr_dereverb(torch.from_numpy(np.ascontiguousarray(y.T))[None].cuda(), taps=4, reference=1)[0].cpu().numpy()
    assert np.array_equal(z, want)
    z_all = wavfile.read(tool.main([src, "--out", str(tmp_path / "bf0"), "--taps", "4", "--beamformer", "wmpdr"])[0])[1]      # all: reference 0
    assert z_all.shape == (8000,) and not np.array_equal(z_all, z)
    # without the flag: the library calls and the bytes of before
    calls = []
    real = W.wpe_mc_dereverb
    monkeypatch.setattr(W, "wpe_mc_dereverb", lambda *a, **k: calls.append("wpe_mc_dereverb") or real(*a, **k))
    monkeypatch.setattr(W, "wpe_mc_mpdr_dereverb", lambda *a, **k: calls.append("wpe_mc_mpdr_dereverb"))
    for extra, shape in ([], (8000, 3)), (["--channel", "1"], (8000,)):
        out = tool.main([src, "--out", str(tmp_path / ("plain" + "".join(extra))), "--taps", "4", *extra])
        fs2, x = wavfile.read(out[0])
        x0 = real(torch.from_numpy(np.ascontiguousarray(y.T))[None].cuda(), taps=4)[0].cpu().numpy()
        assert fs2 == 16000 and x.shape == shape and x.dtype == np.float32
        assert np.array_equal(x, x0.T if not extra else x0[1])
    assert calls == ["wpe_mc_dereverb"] * 4
