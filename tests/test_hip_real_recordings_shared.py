"""GPU: real recordings with one RIR estimate per file (`tester.real_recordings.shared_rir=true`): the chunks of a file are tied rows of one blind
operator.  Same files, overrides and tester construction as tests/test_hip_real_recordings.py (A: three chunks, B: two, C: shorter than a chunk,
D: too short to run): small network, 3 steps, 2 operator updates, 1.024 s chunks."""
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
NAMES = ["A_c0.wav", "A_c1.wav", "A_c2.wav", "B_c0.wav", "B_c1.wav", "C_c0.wav"]
SHARED = "tester.real_recordings.shared_rir=true"


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


def _tester(data, extra=(), batch_size=4, model_dir=None):
    from buddy_amd.config import compose
    from buddy_amd.datasets.recordings import AudioFolder
    from buddy_amd.instantiate import instantiate
    from buddy_amd.synth import synth_state_dict
    from buddy_amd.testing.tester import Tester
    ov = OVERRIDES + list(extra) + ([] if model_dir is None else [f"model_dir={model_dir}", "tester.overriden_name=run"])
    args = compose(tester="real_dereverberation_BUDDy", overrides=ov)
    net = instantiate(args.network)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(3, 32).items()})
    net = net.cuda().eval()
    return Tester(args, net, instantiate(args.diff_params), test_set=AudioFolder(path=data), device="cuda", in_training=model_dir is None,
                  batch_size=batch_size)


def _run(data, extra=(), batch_size=4, model_dir=None):
    """one pass over the folder, every chunk with a noise stream seeded from its own name -> (tester, names handed to noise_factory,
    [(group map of a batch, the row ranges split_groups cut it into; None where there is no group map)])"""
    from buddy_amd.testing import concurrent
    from oracle.sampler_ref import NoiseStream
    t = _tester(data, extra, batch_size, model_dir)
    names, splits = [], []
    t.noise_factory = lambda ns: [names.append(n) or NoiseStream(zlib.crc32(n.encode()) % 100000) for n in ns]
    observed = t.sample_observed

    split_groups, parts = concurrent.split_groups, []

    def split_spy(groups, S):
        parts.append(split_groups(groups, S))
        return parts[-1]

    def spy(y, nm, groups=None):
        del parts[:]
        out = observed(y, nm, groups=groups)
        splits.append((groups, list(parts[-1]) if parts else None))
        return out

    t.sample_observed = spy
    concurrent.split_groups = split_spy
    try:
        if model_dir is not None:
            t.prepare_directories("real_blind_dereverberation")
        t.test_real_recordings("real_blind_dereverberation")
    finally:
        concurrent.split_groups = split_groups
    return t, names, splits


@pytest.fixture(scope="module")
def shared_run(recordings, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shared"))
    t, names, splits = _run(recordings[0], [SHARED], 4, model_dir=out)
    return t, names, splits, os.path.join(out, "run", "real_blind_dereverberation", "VCTK_16k_4s_time")


@pytest.fixture(scope="module")
def default_run(recordings, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("default"))
    t, names, splits = _run(recordings[0], ["tester.real_recordings.shared_rir=false"], 4, model_dir=out)
    return t, names, splits, os.path.join(out, "run", "real_blind_dereverberation", "VCTK_16k_4s_time")


def test_shared_run(recordings, shared_run):
    _, info = recordings
    t, names, splits, base = shared_run
    assert t.skipped == ["D.wav"] and names == NAMES
    assert [g for g, _ in splits] == [[0, 0, 0], [0, 0], [0]]                   # a batch never splits a file
    assert sorted(os.listdir(os.path.join(base, "estimated_rir"))) == ["A.wav", "B.wav", "C.wav"]
    assert [len(t.rirs[k]) for k in "ABC"] == [3, 2, 1]
    for k in "AB":
        for r in t.rirs[k][1:]:
            assert torch.equal(r, t.rirs[k][0])
    assert not torch.equal(t.rirs["A"][0], t.rirs["B"][0])
    for k in "ABC":
        sr, r = wavfile.read(os.path.join(base, "estimated_rir", k + ".wav"))
        assert sr == 16000 and np.array_equal(r, t.rirs[k][0].numpy()) and np.isfinite(r).all() and np.abs(r).max() > 0
        fs, n = info[k]
        sr, a = wavfile.read(os.path.join(base, "reconstructed", k + ".wav"))
        assert sr == fs and len(a) == n and a.dtype == np.float32               # the input's rate and exactly its sample count
        assert np.isfinite(a).all() and np.abs(a).max() > 0


def test_default_is_unchanged(default_run):
    t, names, splits, base = default_run
    assert names == NAMES
    assert all(g is None for g, _ in splits)
    assert sorted(os.listdir(os.path.join(base, "estimated_rir"))) == ["A_c0.wav", "A_c1.wav", "A_c2.wav", "B_c0.wav", "B_c1.wav", "C_c0.wav"]
    assert [len(t.rirs[k]) for k in "ABC"] == [3, 2, 1]
    assert not torch.equal(t.rirs["A"][0], t.rirs["A"][1])                        # one estimate per chunk


def test_one_chunk_file_is_a_group_of_one(shared_run, default_run):
    """C is shorter than a chunk: a batch of its own in both modes, a group of one in the shared one -- the untied path, same noise stream"""
    a, b = dict(shared_run[0].results)["C"].double(), dict(default_run[0].results)["C"].double()
    rel = float((a - b).abs().max() / b.abs().max())
    print(f"C, shared_rir true vs false: {rel:.3e}")
    assert a.shape == b.shape and torch.isfinite(a).all()
    assert rel < 1e-3
    ra, rb = shared_run[0].rirs["C"][0].double(), default_run[0].rirs["C"][0].double()
    assert float((ra - rb).abs().max() / rb.abs().max()) < 1e-3


def test_sub_batches_keep_groups_whole(recordings):
    t, names, splits = _run(recordings[0], [SHARED, "tester.sub_batches=2"], 8)
    assert names == NAMES
    assert splits[0][0] == [0, 0, 0, 1, 1] and splits[1][0] == [0]              # A and B share the batch of chunk-length rows; C's length is its own
    assert splits[0][1] == [(0, 3), (3, 5)]                                     # the sub-batch boundary falls between A and B
    for k in "AB":
        for r in t.rirs[k][1:]:
            assert torch.equal(r, t.rirs[k][0])
    for _, pred in t.results:
        assert torch.isfinite(pred).all()
