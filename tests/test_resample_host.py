"""CPU tests of the real-recording path's host side: rate ratio and filter design (response through the float64 scipy oracle), the pooled chunk
plan, the wav-folder dataset, the tester yaml and the absence of a CPU resampling path."""
import math
import os

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

from buddy_amd.utils.resample import design_filter, out_length, ratio, resample

RATIOS = [(1, 3), (160, 441), (1, 2), (3, 1), (441, 160), (2, 1)]


def oracle(x, up, down, h):
    """the float64 reference of every resampler test: scipy multiplies a given window by `up` itself, hence h / up"""
    return signal.resample_poly(np.asarray(x, np.float64), up, down, axis=-1, window=np.asarray(h, np.float64) / up, padtype="constant")


def test_ratio_and_length():
    assert ratio(44100, 16000) == (160, 441)
    assert ratio(16000, 44100) == (441, 160)
    assert ratio(48000, 16000) == (1, 3) and ratio(16000, 16000) == (1, 1)
    for up, down in RATIOS + [(3, 2)]:
        h = design_filter(up, down)
        for Lin in (1, 7, 1000):
            want = math.ceil(Lin * up / down)
            assert out_length(Lin, up, down) == want
            assert oracle(np.ones(Lin), up, down, h).shape[-1] == want


@pytest.mark.parametrize("up,down", RATIOS)
def test_design(up, down):
    h = design_filter(up, down)
    assert h.dtype == np.float64 and h.ndim == 1
    assert len(h) == 2 * 24 * max(up, down) + 1 and len(h) % 2 == 1
    assert np.array_equal(h, h[::-1])
    assert abs(h.sum() - up) < 1e-12 * up
    assert design_filter(up, down) is h
    assert len(design_filter(up, down, zeros=8)) == 2 * 8 * max(up, down) + 1


def _tone_gain_db(up, down, r, fit):
    """gain of a unit tone at fraction r of the lower of the two rates, over the middle half of the output"""
    h = design_filter(up, down)
    Lin = 6000 if up <= down else 3000
    f_in = r * min(1.0, up / down)                      # cycles per input sample
    x = np.sin(2 * np.pi * f_in * np.arange(Lin) + 0.3)
    y = oracle(x, up, down, h)
    n = np.arange(len(y))[len(y) // 4: 3 * len(y) // 4]
    mid = y[len(y) // 4: 3 * len(y) // 4]
    if fit:                                             # amplitude of the tone itself (least squares at its known frequency)
        f_out = f_in * down / up
        A = np.stack([np.cos(2 * np.pi * f_out * n), np.sin(2 * np.pi * f_out * n)], axis=1)
        amp = np.hypot(*np.linalg.lstsq(A, mid, rcond=None)[0])
    else:                                               # everything that is left (the tone aliases): rms as an amplitude
        amp = np.sqrt(2.0 * np.mean(mid ** 2))
    return 20 * np.log10(amp + 1e-300)


@pytest.mark.parametrize("up,down", RATIOS)
def test_response(up, down):
    lo, mid = _tone_gain_db(up, down, 0.0625, True), _tone_gain_db(up, down, 0.40, True)
    print(f"{up}/{down}: r=0.0625 {lo:+.4f} dB, r=0.40 {mid:+.4f} dB")
    assert abs(lo) <= 0.001
    assert mid >= -0.1
    if down > up:
        stop = _tone_gain_db(up, down, 0.55, False)
        print(f"{up}/{down}: r=0.55 {stop:.1f} dB")
        assert stop <= -100.0


def test_pool_plan():
    from buddy_amd.testing.longform import pool_plan
    lengths, chunk, overlap, bs = [40000, 30400, 11200], 16384, 2048, 4
    cuts, batches = pool_plan(lengths, chunk, overlap, bs)
    assert [len(s) for s, _ in cuts] == [3, 2, 1]
    assert [c for _, c in cuts] == [chunk, chunk, 11200]                    # equal chunks; a short file is one chunk of its own length
    for L, (starts, clen) in zip(lengths, cuts):
        covered = np.zeros(L, bool)
        for s in starts:
            assert 0 <= s and s + clen <= L                                  # never padded
            covered[s:s + clen] = True
        assert covered.all()
        for a, b in zip(starts, starts[1:]):
            assert a + clen - b >= overlap
    assert batches == [[(0, 0), (0, 1), (0, 2), (1, 0)], [(1, 1)], [(2, 0)]]   # file-then-chunk order, full except the last, short group apart
    # short files share a batch only at exactly equal length; a file of exactly one chunk is pooled
    cuts, batches = pool_plan([5000, 16384, 5000, 5001, 5000], chunk, overlap, 2)
    assert batches == [[(1, 0)], [(0, 0), (2, 0)], [(4, 0)], [(3, 0)]]
    assert cuts[1] == ([0], chunk)
    assert pool_plan([], chunk, overlap, 4) == ([], [])


def test_audio_folder(tmp_path):
    from buddy_amd.datasets.recordings import AudioFolder
    rs = np.random.RandomState(0)
    st = (rs.uniform(-1, 1, (4410, 2)) * 32767).astype(np.int16)
    mono = rs.uniform(-1, 1, 4800).astype(np.float32)
    os.makedirs(tmp_path / "sub")
    wavfile.write(tmp_path / "sub" / "b_stereo.wav", 44100, st)
    wavfile.write(tmp_path / "a_mono.wav", 48000, mono)
    wavfile.write(tmp_path / "c_mono.wav", 16000, mono[:100])
    (tmp_path / "notes.txt").write_text("not audio")
    ds = AudioFolder(path=str(tmp_path))
    assert len(ds) == 3
    assert [ds[i][2] for i in range(3)] == ["a_mono.wav", "c_mono.wav", "b_stereo.wav"]       # sorted by path
    a, fs, _ = ds[0]
    assert fs == 48000 and a.dtype == np.float64 and a.shape == (4800,) and np.array_equal(a, mono.astype(np.float64))
    b, fs, _ = ds[2]
    assert fs == 44100 and b.dtype == np.float64 and b.shape == (4410,)                           # own rate, no crop
    assert np.allclose(b, (st.astype(np.float64) / 32767).mean(axis=1), rtol=0, atol=1e-15)      # int scaling of vctk._read, mean downmix
    assert len(AudioFolder(path=str(tmp_path), num_examples=2)) == 2
    assert len(AudioFolder(path=str(tmp_path), num_examples=0)) == 3


def test_yaml_and_directories(tmp_path):
    from buddy_amd.config import compose
    args = compose(tester="real_dereverberation_BUDDy")
    assert args.tester.modes == ["real_blind_dereverberation"]
    rr = args.tester.real_recordings
    assert rr.gain == 1.0 and rr.chunk_seconds is None and rr.overlap_seconds == 0.5 and rr.output_rate == "input"
    blind = compose(tester="blind_dereverberation_BUDDy").tester
    for k in ("sampler", "sampling_params", "posterior_sampling", "informed_dereverberation", "blind_dereverberation"):
        assert args.tester[k] == blind[k]
    assert "real_recordings" not in blind
    from buddy_amd.testing.tester import Tester
    t = Tester.__new__(Tester)
    t.args = compose(tester="real_dereverberation_BUDDy", overrides=[f"model_dir={tmp_path}", "tester.overriden_name=run"])
    t.prepare_directories("real_blind_dereverberation")
    base = os.path.join(str(tmp_path), "run", "real_blind_dereverberation", "VCTK_16k_4s_time")
    assert sorted(os.listdir(base)) == ["degraded", "estimated_rir", "reconstructed"]


def test_no_cpu_path():
    from buddy_amd import _lib
    x = torch.zeros(2, 480)
    assert resample(x, 16000, 16000) is x
    with pytest.raises(_lib.BuddyHipError):
        resample(x, 48000, 16000)
    with pytest.raises(_lib.BuddyHipError):
        resample(x[0], 16000, 44100)


def test_entry_refuses_bad_arguments_before_any_launch():
    """the argument checks of buddy_resample need no GPU: every one returns BUDDY_ERR_ARG with a message (pointers are never dereferenced)"""
    from buddy_amd import _lib
    lib = _lib.load()
    p = 0x1000
    bad = {"null x": (None, 1, 10, p, 3, 1, 1, p, 10), "null h": (p, 1, 10, None, 3, 1, 1, p, 10), "null y": (p, 1, 10, p, 3, 1, 1, None, 10),
           "B": (p, 0, 10, p, 3, 1, 1, p, 10), "Lin": (p, 1, 0, p, 3, 1, 1, p, 0), "up": (p, 1, 10, p, 3, 0, 1, p, 0), "down": (p, 1, 10, p, 3, 1, 0, p, 0),
           "gcd": (p, 1, 10, p, 3, 2, 4, p, 5), "up > 1024": (p, 1, 10, p, 3, 1025, 1, p, 10250), "down > 1024": (p, 1, 10, p, 3, 1, 1025, p, 1),
           "Nh even": (p, 1, 10, p, 4, 1, 1, p, 10), "Nh > 65537": (p, 1, 10, p, 65539, 1, 1, p, 10), "Lout": (p, 1, 10, p, 3, 3, 2, p, 14)}
    for why, a in bad.items():
        assert lib.buddy_resample(*a, None) == 2, why
        assert lib.buddy_last_error().decode().startswith("buddy_resample: "), why
