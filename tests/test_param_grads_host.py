"""Host: the parameter-gradient entry points are declared and exported, the EDM training formulas (reference diff_params/edm.py:24-33,
shared.py:123-160, restated here in numpy) hold on fixed draws, and a default module stays inference-only (requires_grad=False)."""
import os
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("buddy_ncsnpp_vjp_params", "buddy_ncsnpp_update_params")


def test_new_symbols_declared_bound_and_exported():
    from buddy_amd import _lib
    lib = _lib.load()
    for s in NEW:                                 # header, signatures and exports agree for every name: tests/test_abi_host.py
        assert s in _lib.EXPORTED and hasattr(lib, s), s


def _edm():
    from buddy_amd.diff_params.edm import EDM
    return EDM("ve_karras", SimpleNamespace(sigma_data=0.05, sigma_min=1e-5, sigma_max=10.0, rho=10.0))


def test_sample_time_training_formula():
    e = _edm()
    torch.manual_seed(11)
    t = e.sample_time_training(6).double().numpy()
    torch.manual_seed(11)
    a = torch.rand(6).double().numpy()
    r = (10.0 ** 0.1 + a * ((1e-5) ** 0.1 - 10.0 ** 0.1)) ** 10.0
    assert np.allclose(t, r, rtol=1e-5)
    assert (t >= 1e-5 * (1 - 1e-4)).all() and (t <= 10.0 * (1 + 1e-4)).all()


def test_train_preconditioning_and_loss_formulas():
    e = _edm()
    rs = np.random.RandomState(5)
    x = rs.standard_normal((3, 64))
    n = rs.standard_normal((3, 64))
    t = np.array([0.01, 0.5, 3.0])
    sd = 0.05
    inp, target, cnoise = e.prepare_train_preconditioning(torch.from_numpy(x), torch.from_numpy(t), n=torch.from_numpy(n))
    s = t[:, None]
    xp = x + s * n
    cskip, cout, cin = sd ** 2 / (s ** 2 + sd ** 2), s * sd / np.sqrt(sd ** 2 + s ** 2), 1 / np.sqrt(sd ** 2 + s ** 2)
    assert np.allclose(inp.numpy(), cin * xp)
    assert np.allclose(target.numpy(), (x - cskip * xp) / cout)
    assert np.allclose(cnoise.numpy(), 0.25 * np.log(t))
    net = lambda a, c: 0.3 * a + c[:, None, None]
    err2, sig = e.loss_fn(net, torch.from_numpy(x), torch.from_numpy(n), t=torch.from_numpy(t))
    est = 0.3 * cin * xp + 0.25 * np.log(t)[:, None]
    assert np.allclose(err2.numpy(), (est - (x - cskip * xp) / cout) ** 2)
    assert np.allclose(sig.numpy(), t)


def test_default_module_is_inference_only():
    from buddy_amd.networks.ncsnpp import NCSNppTime
    net = NCSNppTime(stft={"n_fft": 126, "hop_length": 32, "center": True}, nf=32)
    assert all(not p.requires_grad for p in net.parameters())
    assert net._n_params == sum(p.numel() for p in net.parameters())
    assert net._train_params() == ()
