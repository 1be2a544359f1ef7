"""Host logic of the training loop (no GPU): the EMA factor, the new instantiate targets and the untouched sampler configuration, the training
dataset's rules, and the optimizer's documented state-dict layout against torch's own Adam."""
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "train_small.npz")


def test_ema_factor_formula_and_fixture():
    from buddy_amd.training.trainer import ema_factor
    d = np.load(GOLD)
    B, steps = int(d["meta"][4]), int(d["meta"][6])
    _, _, rate, rampup = (float(v) for v in d["hp"])
    got = [ema_factor(it, B, rampup, rate) for it in range(steps)]
    assert got == [float(v) for v in d["ema_s"]], (got, d["ema_s"])
    assert got[:3] == [0.0, 2 / 6, 4 / 6] and got[3:] == [0.9] * 3        # ramp branch, then the constant one
    # t = it * batch_size at 0, rampup - 1 and rampup (batch_size 1 makes t = it)
    assert ema_factor(0, 1, 10000, 0.9999) == 0.0
    assert ema_factor(9999, 1, 10000, 0.9999) == float(np.clip(9999 / 10000, 0.0, 0.9999)) == 0.9999
    assert ema_factor(9998, 1, 10000, 0.9999) == 0.9998
    assert ema_factor(10000, 1, 10000, 0.9999) == 0.9999
    assert ema_factor(5, 16, 10000, 0.9999) == 80 / 10000                # t counts examples, not iterations


def test_new_targets_resolve_and_sampler_config_is_unchanged():
    from buddy_amd.config import compose, compose_train
    from buddy_amd.instantiate import resolve
    assert resolve("training.trainer.Trainer").__name__ == "Trainer"
    assert resolve("datasets.vctk.VCTKTrain").__name__ == "VCTKTrain"
    args = compose()
    assert sorted(args.keys()) == ["diff_params", "exp", "model_dir", "network", "tester"]
    assert dict(args.exp) == {"exp_name": "VCTK_16k_4s_time", "sample_rate": 16000, "audio_len": 65536}
    tr = compose_train(tester="blind_dereverberation_BUDDy")
    for k in ("network", "diff_params", "tester", "model_dir"):        # the training tree holds the sampler's groups as they are
        assert tr[k] == args[k], k
    assert {k: tr.exp[k] for k in args.exp} == dict(args.exp)
    for k in ("optimizer", "batch_size", "seed", "resume", "resume_checkpoint", "ema_rate", "ema_rampup", "use_grad_clip", "max_grad_norm", "trainer"):
        assert k in tr.exp.keys(), k
    assert resolve(tr.exp.trainer["_target_"]).__name__ == "Trainer" and resolve(tr.dset.train["_target_"]).__name__ == "VCTKTrain"
    for k in ("log", "log_interval", "heavy_log_interval", "save_model", "save_interval", "num_sigma_bins"):
        assert k in tr.logging.keys(), k


def _wav(path, data, fs=16000):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, fs, data.astype(np.float32))


def test_vctk_train_rules(tmp_path):
    from buddy_amd.datasets.vctk import VCTKTrain
    rs = np.random.RandomState(0)
    long_ = rs.uniform(-0.5, 0.5, 5000)
    stereo = rs.uniform(-0.5, 0.5, (4000, 2))
    short = rs.uniform(-0.5, 0.5, 300)
    _wav(str(tmp_path / "p001" / "a.wav"), long_)
    _wav(str(tmp_path / "p002" / "b.wav"), stereo)
    _wav(str(tmp_path / "p003" / "c.wav"), short)
    _wav(str(tmp_path / "p280" / "d.wav"), np.full(5000, 0.25))       # discarded speaker
    _wav(str(tmp_path / "p351" / "e.wav"), np.full(5000, -0.25))      # test speaker: not in the training set either
    seg = 1024
    ds = VCTKTrain(fs=16000, segment_length=seg, path=str(tmp_path), speakers_discard=["p280"], speakers_test=["p351"], seed=3)
    assert sorted(os.path.basename(os.path.dirname(f)) for f in ds.train_samples) == ["p001", "p002", "p003"]
    it = iter(ds)
    first = [next(it) for _ in range(40)]
    assert all(s.shape == (seg,) for s in first)
    l32, m32, s32 = long_.astype(np.float32).astype(np.float64), stereo.astype(np.float32).astype(np.float64).mean(axis=1), short.astype(np.float32).astype(np.float64)

    def is_crop(s, full):
        return any(np.array_equal(s, full[i:i + seg]) for i in np.flatnonzero(full[:len(full) - seg + 1] == s[0]))

    kinds = set()
    for s in first:
        assert not np.all(s == 0.25) and not np.all(s == -0.25), "a discarded / test speaker was drawn"
        if is_crop(s, l32):
            kinds.add("crop")
        elif is_crop(s, m32):
            kinds.add("mono")                                           # the mean over the two channels
        else:
            # wrap padding of the short file: some offset idx with s == np.pad(short, (idx, seg - 300 - idx), 'wrap')
            assert any(np.array_equal(s, np.pad(s32, (i, seg - 300 - i), "wrap")) for i in range(seg - 300)), "not a wrap-padded short file"
            kinds.add("wrap")
    assert kinds == {"crop", "mono", "wrap"}
    again = iter(VCTKTrain(fs=16000, segment_length=seg, path=str(tmp_path), speakers_discard=["p280"], speakers_test=["p351"], seed=3))
    for s in first[:8]:
        assert np.array_equal(s, next(again)), "the same seed must give the same first segments"
    with pytest.raises(AssertionError):
        next(iter(VCTKTrain(fs=8000, segment_length=seg, path=str(tmp_path), speakers_discard=["p280"], speakers_test=["p351"])))


def test_state_dict_layout_matches_torch_adam():
    """the documented layout of FusedAdam.state_dict() (a function that needs no GPU) against torch.optim.Adam on CPU tensors of the network's
    shapes, before and after a step; W (requires_grad False) gets no state in either"""
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.training.fused import GROUP_DEFAULTS, STATE_KEYS, describe_state_dict, state_dict_layout
    net = instantiate(compose(overrides=["network.nf=32"]).network)
    shapes = [tuple(p.shape) for p in net.parameters()]
    rg = [kind != "fourier" for _, _, kind, _ in net._specs]
    assert rg.count(False) == 1
    params = [torch.nn.Parameter(torch.zeros(s), requires_grad=r) for s, r in zip(shapes, rg)]
    opt = torch.optim.Adam(params, lr=2e-4, betas=(0.8, 0.99), eps=1e-7)
    assert describe_state_dict(opt.state_dict()) == state_dict_layout(shapes, rg, lr=2e-4, betas=(0.8, 0.99), eps=1e-7, stepped=False)
    for p in params:
        if p.requires_grad:
            p.grad = torch.ones_like(p)
    opt.step()
    sd = opt.state_dict()
    want = state_dict_layout(shapes, rg, lr=2e-4, betas=(0.8, 0.99), eps=1e-7)
    assert describe_state_dict(sd) == want
    assert set(sd["param_groups"][0]) == set(GROUP_DEFAULTS) | {"params"}
    assert all(tuple(st) == STATE_KEYS for st in sd["state"].values())
    defaults = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0]
    assert {k: (tuple(v) if k == "betas" else v) for k, v in defaults.items() if k != "params"} == GROUP_DEFAULTS


def test_optimizer_has_no_cpu_path():
    from buddy_amd import _lib
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.training.fused import FusedAdam
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    net = instantiate(compose(overrides=["network.nf=32"]).network)
    with pytest.raises(_lib.BuddyHipError):
        FusedAdam(net.parameters(), lr=1e-4, network=net)
