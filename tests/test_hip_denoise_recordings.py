"""GPU: the spectral post-filter as the last stage of the real-recordings front end (``tester.real_recordings.denoise``) and the stand-alone tool
(``tools/denoise.py``).  The pattern of tests/test_hip_wpe_mc_recordings.py: nf = 32, T = 3, short chunks, two files of 1.1 s at 16 kHz, one of
them with two channels; seeded Philox noise, so that two runs of one configuration write the same bytes."""
import csv
import importlib.util
import os
import sys

import numpy as np
import pytest
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _denoise_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERRIDES = ["tester.sampling_params.T=3", "tester.posterior_sampling.blind_hp.op_updates_per_step=2",
             "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "tester.real_recordings.chunk_seconds=1.024",
             "tester.real_recordings.overlap_seconds=0.128", "network.nf=32", "tester.noise.generator=philox",
             "tester.real_recordings.channels=reference", "tester.real_recordings.reference_channel=0"]
COLUMNS = ["file", "samples", "frames", "snr_est_db", "noise_db", "att_db", "flags", "gain", "floor_db"]
N = 17600


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    root = tmp_path_factory.mktemp("noisy_recordings")
    a = 0.1 * R.noisy_bursts(10.0, L=N, seed=5, start=0.1)[0]
    b = np.stack([0.1 * R.noisy_bursts(5.0, L=N, seed=6 + c, start=0.1)[0] for c in range(2)], axis=1)
    wavfile.write(root / "A.wav", 16000, a.astype(np.float32))
    wavfile.write(root / "B.wav", 16000, np.ascontiguousarray(b, dtype=np.float32))
    return str(root)


def _cli(out, data, extra=()):
    import test as cli
    import torch
    torch.manual_seed(0)                             # the operator's start is drawn from the global generators: every run from the same state
    tester = cli.main(["--config-name=conf_VCTK.yaml", "tester=real_dereverberation_BUDDy", *OVERRIDES, f"model_dir={out}", "+gpu=0",
                       f"dset.test.path={data}", "+batch_size=4", "tester.overriden_name=run", "+allow_random_init=true", *extra])
    return tester, os.path.join(str(out), "run", "real_blind_dereverberation", "VCTK_16k_4s_time")


def _listing(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


def _tool():
    spec = importlib.util.spec_from_file_location("denoise_tool", os.path.join(ROOT, "tools", "denoise.py"))      # not ``import denoise``: the package has one
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_post_filter_through_the_tester_and_the_tool(tmp_path, recordings, monkeypatch, capsys):
    from buddy_amd.utils import denoise as D
    tester, on = _cli(tmp_path / "on", recordings, ["tester.real_recordings.denoise.use=true"])
    assert tester.skipped == []
    assert sorted(os.listdir(on)) == [".argv", "degraded", "denoise.csv", "denoised", "estimated_rir", "reconstructed"]
    rows = list(csv.DictReader(open(os.path.join(on, "denoise.csv"))))
    assert list(rows[0].keys()) == COLUMNS and [r["file"] for r in rows] == ["A", "B"]
    for r in rows:
        assert int(r["samples"]) == N and int(r["frames"]) == R.frames(N) and r["flags"] == "" and r["gain"] == "lsa" and float(r["floor_db"]) == -15.0
        assert 0.0 < float(r["snr_est_db"]) < 20.0 and 0.0 < float(r["att_db"]) < 15.0
    assert float(rows[0]["snr_est_db"]) > float(rows[1]["snr_est_db"])                     # 10 dB against 5 dB
    for name in ("A", "B"):
        fs, d = wavfile.read(os.path.join(on, "degraded", name + ".wav"))
        fs1, z = wavfile.read(os.path.join(on, "denoised", name + ".wav"))
        assert fs == fs1 == 16000 and d.shape == z.shape == (N,) and np.isfinite(z).all() and not np.array_equal(d, z)
        assert abs(z.std() - 0.05) < 1e-3 * 0.05                                          # what the sampler observed carries the scaling rule
    # the block off, and the block absent: nothing of the post-filter runs, and both write the same folders and bytes
    monkeypatch.setattr(D, "denoise", lambda *a, **k: pytest.fail("the post-filter ran with denoise.use off"))
    _, off = _cli(tmp_path / "off", recordings)
    _, absent = _cli(tmp_path / "absent", recordings, ["tester.real_recordings.denoise=null"])
    monkeypatch.undo()
    wavs = [f for f in _listing(off) if f.endswith(".wav")]
    assert [f for f in _listing(off) if f != ".argv"] == wavs == [f for f in _listing(absent) if f != ".argv"]
    assert sorted({os.path.dirname(f) for f in wavs}) == ["degraded", "estimated_rir", "reconstructed"]
    for f in wavs:
        assert open(os.path.join(off, f), "rb").read() == open(os.path.join(absent, f), "rb").read(), f
    for name in ("A", "B"):                                                                # degraded/ does not know about the post-filter
        f = os.path.join("degraded", name + ".wav")
        assert open(os.path.join(on, f), "rb").read() == open(os.path.join(off, f), "rb").read(), f
    # the tool on the same files: wavs of the input's rate, length and channels, and the tester's statistics
    capsys.readouterr()
    written, trows = _tool().main([recordings, "--out", str(tmp_path / "tool")])
    printed = capsys.readouterr().out
    assert [os.path.relpath(p, tmp_path / "tool") for p in written] == ["A.wav", "B.wav"]
    for p, shape in zip(written, ((N,), (N, 2))):
        fs, x = wavfile.read(p)
        assert fs == 16000 and x.shape == shape and x.dtype == np.float32 and np.isfinite(x).all()
    assert [r["file"] for r in trows] == ["A", "B:0", "B:1"]
    assert list(csv.DictReader(open(tmp_path / "tool" / "denoise.csv")))[0].keys() == rows[0].keys()
    for mine, theirs in ((trows[0], rows[0]), (trows[1], rows[1])):
        for key in ("snr_est_db", "noise_db", "att_db"):
            assert abs(mine[key] - float(theirs[key])) <= 1e-6, (mine["file"], key)
            assert f"{mine[key]:.6f}" in printed
    _, z = wavfile.read(os.path.join(on, "denoised", "A.wav"))                              # the same signal up to the tester's gain
    _, x = wavfile.read(written[0])
    g = float(np.dot(z, x) / np.dot(x, x))
    assert np.abs(z - g * x).max() <= 1e-5 * np.abs(z).max()
    # another rule and floor
    written, wrows = _tool().main([os.path.join(recordings, "A.wav"), "--out", str(tmp_path / "wiener"), "--gain", "wiener", "--floor-db", "-20"])
    assert wrows[0]["gain"] == "wiener" and wrows[0]["floor_db"] == -20.0 and wrows[0]["att_db"] > trows[0]["att_db"]
