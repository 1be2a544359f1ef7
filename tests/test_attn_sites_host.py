"""Host checks of the NCSN++ attention sites (``attn_resolutions``): constructor, state-dict names against the reference's (stored in the
fixtures recorded by tests/golden/make_golden_attn.py), parameter counts of the C-ABI, the refusal of configurations where the reference's
construction and forward would disagree, the config / checkpoint surface.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["net_attn_lo", "net_attn_hi", "net_full_attn"]


def _net(g, **kw):
    from buddy_amd.config import AttrDict, CONF_DIR, load_yaml
    from buddy_amd.networks.ncsnpp import NCSNppTime
    nf, n_fft, hop = (int(v) for v in g["meta"][:3])
    cfg = load_yaml(os.path.join(CONF_DIR, "network", "ncsnpp.yaml"))
    cfg.pop("_target_")
    cfg.update(nf=nf, ch_mult=[int(c) for c in g["ch_mult"]], num_res_blocks=int(g["num_res_blocks"]),
               attn_resolutions=[int(r) for r in g["attn_resolutions"]], image_size=int(g["image_size"]),
               stft=AttrDict(n_fft=n_fft, hop_length=hop, center=True), **kw)
    return NCSNppTime(**cfg)


@pytest.mark.parametrize("name", FIXTURES)
def test_constructor_accepts_and_names_match_reference(golden, name):
    from buddy_amd.synth import synth_state_dict
    g = golden(name)
    net = _net(g)
    assert list(net.state_dict().keys()) == [str(n) for n in g["names"]]
    nf, seed = int(g["meta"][0]), int(g["meta"][5])
    sd = synth_state_dict(seed, nf, tuple(int(c) for c in g["ch_mult"]), int(g["num_res_blocks"]), attn_mask=net.attn_mask)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    # the reference's AttnBlocks sit at these module indices (taps recorded from its forward hooks)
    attn_idx = sorted(int(n.split(".")[1]) for n, *_ in net._specs if n.endswith("NIN_0.W"))
    assert attn_idx == [int(i) for i in g["attn_taps"]]


def test_masks_of_the_fixture_configurations(golden):
    from buddy_amd.synth import attn_mask_of
    assert _net(golden("net_attn_lo")).attn_mask == 0b0100
    assert _net(golden("net_attn_hi")).attn_mask == 0b0011
    assert _net(golden("net_full_attn")).attn_mask == 0b1100
    assert attn_mask_of((0,), 256, 4) == 0 and attn_mask_of((16,), 256, 4) == 0 and attn_mask_of((256, 32), 256, 4) == 0b1001


@pytest.mark.parametrize("nf,ch_mult,nrb,mask", [(32, (1, 2, 2, 2), 2, 0b0100), (32, (1, 2, 2, 2), 2, 0b0011), (128, (1, 2, 2, 2), 1, 0b1100),
                                                 (32, (1, 2), 2, 0b11), (128, (1, 2, 2, 2), 1, 0)])
def test_param_count_attn_equals_blob(nf, ch_mult, nrb, mask):
    from buddy_amd import _lib
    from buddy_amd.synth import module_specs
    lib = _lib.load()
    cm = (ctypes.c_int * len(ch_mult))(*ch_mult)
    n, n0 = ctypes.c_longlong(), ctypes.c_longlong()
    assert lib.buddy_ncsnpp_param_count_attn(nf, cm, len(ch_mult), nrb, mask, ctypes.byref(n)) == 0
    assert n.value == sum(int(np.prod(s)) for _, s, *_ in module_specs(nf, ch_mult, nrb, attn_mask=mask))
    assert lib.buddy_ncsnpp_param_count(nf, cm, len(ch_mult), nrb, ctypes.byref(n0)) == 0
    assert lib.buddy_ncsnpp_param_count_attn(nf, cm, len(ch_mult), nrb, 0, ctypes.byref(n)) == 0 and n.value == n0.value
    # a mask bit beyond the last level is an argument error
    assert lib.buddy_ncsnpp_param_count_attn(nf, cm, len(ch_mult), nrb, 1 << len(ch_mult), ctypes.byref(n)) != 0


def test_default_specs_unchanged():
    from buddy_amd.synth import module_specs, synth_state_dict
    for args in [(128, (1, 2, 2, 2), 1), (32, (1, 2), 2), (32, (1, 1, 2, 2), 1)]:
        assert module_specs(*args) == module_specs(*args, attn_mask=0)
        a, b = synth_state_dict(3, *args), synth_state_dict(3, *args, attn_mask=0)
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("image_size,R", [(256, (16,)), (64, (64,)), (128, (32, 8))])
def test_image_size_bins_mismatch_refused(image_size, R):
    """n_fft = 510: 256 bins.  image_size 256 / attn (16,): built at level 4 -- there is none -- fine; at 64 / (64,): built at level 0, the reference
    runs it at level 2 (height 64): refused, naming both values."""
    from buddy_amd.config import AttrDict, CONF_DIR, load_yaml
    from buddy_amd.networks.ncsnpp import NCSNppTime
    cfg = load_yaml(os.path.join(CONF_DIR, "network", "ncsnpp.yaml"))
    cfg.pop("_target_")
    cfg.update(nf=32, attn_resolutions=list(R), image_size=image_size, stft=AttrDict(n_fft=510, hop_length=128, center=True))
    if image_size == 256:
        assert NCSNppTime(**cfg).attn_mask == 0
        return
    with pytest.raises(NotImplementedError, match=rf"image_size={image_size}.*256 frequency bins"):
        NCSNppTime(**cfg)


def test_instantiate_override_and_checkpoint_load():
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.synth import synth_state_dict
    from buddy_amd.utils.training_utils import load_state_dict
    args = compose(overrides=["network.nf=32", "network.attn_resolutions=[32]"])
    net = instantiate(args.network)
    assert net.attn_mask == 0b1000
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(4, 32, attn_mask=0b1000).items()}
    assert any(k.startswith("all_modules.") and k.endswith("NIN_0.W") for k in sd)
    assert load_state_dict({"network": sd, "ema": sd}, network=net, log=False)
    got = net.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items())


def test_header_and_exports_agree():
    from buddy_amd import _lib
    lib = _lib.load()
    for name in ("buddy_ncsnpp_param_count_attn", "buddy_ncsnpp_create_attn"):       # header = signatures = exports: tests/test_abi_host.py
        assert name in _lib.EXPORTED and hasattr(lib, name)
