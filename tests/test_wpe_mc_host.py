"""Host side of the multichannel WPE front end (no GPU): argument validation before the GPU is asked for, the shape limit and the frame count,
the unmixed read of ``AudioFolder``, the geometry of ``rooms.array_rows``, and the defaults of the new yaml keys."""
import math

import numpy as np
import pytest
import torch
from scipy.io import wavfile


def test_arguments_are_validated_without_a_gpu():
    from buddy_amd.utils.wpe import wpe_mc_dereverb, wpe_mc_hip
    y = torch.zeros(1, 2, 4000)
    for bad in (torch.zeros(2, 4000), torch.zeros(1, 9, 4000), torch.zeros(1, 2, 4000, dtype=torch.float64), torch.zeros(1, 2, 0)):
        with pytest.raises(ValueError):
            wpe_mc_dereverb(bad)
    for kw in (dict(taps=0), dict(taps=49), dict(delay=-1), dict(iterations=-1)):
        with pytest.raises(ValueError):
            wpe_mc_dereverb(y, **kw)
    with pytest.raises(ValueError):
        wpe_mc_dereverb(torch.zeros(1, 8, 4000), taps=13)                   # D * taps = 104
    Y = torch.zeros(4, 2, 30, dtype=torch.complex128)
    for bad in (torch.zeros(4, 2, 30, dtype=torch.complex64), torch.zeros(4, 30, dtype=torch.complex128), torch.zeros(4, 9, 30, dtype=torch.complex128)):
        with pytest.raises(ValueError):
            wpe_mc_hip(bad)
    with pytest.raises(ValueError):
        wpe_mc_hip(Y, taps=49)
    if not torch.cuda.is_available():                                       # a CPU tensor of a valid shape: the product has no CPU form
        from buddy_amd._lib import BuddyHipError
        with pytest.raises(BuddyHipError):
            wpe_mc_dereverb(y)
        with pytest.raises(BuddyHipError):
            wpe_mc_hip(Y)


def test_supported_and_frames():
    from buddy_amd.utils.wpe import frames, supported
    from oracle import wpe_ref
    assert supported(1, 96) and supported(8, 12) and supported(8, 1) and supported(3, 32)
    assert not supported(9, 1) and not supported(8, 13) and not supported(1, 97) and not supported(0, 10) and not supported(2, 0)
    for L in (1, 127, 128, 129, 383, 384, 385, 512, 700, 2000, 5000, 12345, 16000, 64000):
        assert frames(L) == wpe_ref.stft(np.zeros((1, L), np.float32)).shape[1], L


def test_audio_folder_channels(tmp_path):
    from buddy_amd.datasets.recordings import AudioFolder
    rs = np.random.RandomState(0)
    wavfile.write(tmp_path / "a.wav", 16000, (0.1 * rs.standard_normal((500, 3))).astype(np.float32))
    wavfile.write(tmp_path / "b.wav", 8000, (3000 * rs.standard_normal(300)).astype(np.int16))
    ds = AudioFolder(path=str(tmp_path))
    for i, (name, C, n, fs) in enumerate([("a.wav", 3, 500, 16000), ("b.wav", 1, 300, 8000)]):
        ch, f1, n1 = ds.channels(i)
        mono, f2, n2 = ds[i]
        assert ch.shape == (C, n) and ch.dtype == np.float64 and (f1, n1) == (f2, n2) == (fs, name)
        assert np.array_equal(np.mean(ch.T, axis=1), mono) if C > 1 else np.array_equal(ch[0], mono)


def test_array_rows_geometry():
    from buddy_amd.utils import rooms
    room = rooms.room_row((5.0, 4.0, 3.0), (1.0, 1.0, 1.5), (3.0, 2.0, 1.2), 0.8)
    for mics, radius, angle in [(8, 0.1, 0.3), (3, 0.25, -1.0), (1, 0.1, 0.0)]:
        rows = rooms.array_rows(room, mics, radius, angle)
        assert rows.shape == (mics, 16) and rows.dtype == np.float64
        keep = [k for k in range(16) if k not in (6, 7)]
        assert np.array_equal(rows[:, keep], np.tile(room[keep], (mics, 1)))                  # the shared room, source and height
        d = rows[:, 6:8] - room[6:8]
        assert np.allclose(np.hypot(d[:, 0], d[:, 1]), radius, rtol=0, atol=1e-12)
        want = angle + 2.0 * np.pi * np.arange(mics) / mics
        got = np.arctan2(d[:, 1], d[:, 0])
        assert np.allclose(np.angle(np.exp(1j * (got - want))), 0.0, atol=1e-9)
        if mics > 1:                                                                          # neighbours one chord apart
            assert np.allclose(np.linalg.norm(rows[0, 6:9] - rows[1, 6:9]), 2.0 * radius * math.sin(math.pi / mics), atol=1e-12)
    assert rooms.array_rows(room, 4, 1.9, 0.0).shape == (4, 16)
    for radius in (2.0, 2.5, 4.0):                                                            # the receiver is 2 m from the walls x = Lx, y = 0 and y = Ly
        with pytest.raises(ValueError):
            rooms.array_rows(room, 4, radius, 0.0)
    with pytest.raises(ValueError):
        rooms.array_rows(room, 0, 0.1, 0.0)
    assert rooms.ARRAY not in (rooms.ROOMS, rooms.ROOM_BANDS, 0, 1, 2, 3)
    a = rooms.draw_array_angle(3, "p1/x")
    assert 0.0 <= a < 2.0 * np.pi and a == rooms.draw_array_angle(3, "p1/x") and a != rooms.draw_array_angle(3, "p1/y")


def test_yaml_defaults():
    from buddy_amd.config import compose
    from buddy_amd.testing.tester import channel_options
    rr = compose(tester="real_dereverberation_BUDDy").tester.real_recordings
    assert rr.channels == "mean" and rr.reference_channel == 0 and dict(rr.wpe) == {"taps": 10, "delay": 3, "iterations": 3}
    assert channel_options(rr) == ("mean", 0, (10, 3, 3))
    assert channel_options({}) == ("mean", 0, (10, 3, 3))                                     # a yaml written before the keys existed
    rr = compose(tester="real_dereverberation_BUDDy", overrides=["tester.real_recordings.channels=wpe", "tester.real_recordings.wpe.taps=4"]).tester.real_recordings
    assert channel_options(rr) == ("wpe", 0, (4, 3, 3))
