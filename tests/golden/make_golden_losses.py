"""Fixtures of the reconstruction-loss family (utils/losses.py of the reference): recorded from the REFERENCE on the CPU, through the stubs,
configuration composer, synthetic signals and end-to-end runner of make_golden.py (imported, not copied).

    python tests/golden/make_golden_losses.py [losses] [e2e_blind_losses]

losses.npz            U = 1, L = 8192, blind operator (BlindSubbandFiltering, random-coherent phases from NoiseStream(21)) on fixed y / x_hat:
                      value of get_loss(spec, op)(y, op.degradation(x_hat)) for every STFT name x {None, sqrt, exp, log, linear} and for l2_sum /
                      l2_mean; its gradient w.r.t. x_hat for every name without weighting and with one weighting per name (the weightings rotate
                      over the names, so each is covered; all of them would not fit the 1 MiB file limit).  The same for the informed RIROperator
                      for a handful of names.
e2e_blind_losses.npz  _e2e(blind=True, T=4, order=1) with non-default losses in all three blocks (the overrides are stored in the fixture).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (sets up the reference's import path and its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STFT_NAMES = ["l2_stft_sum", "l2_stft_mag_sum", "l2_stft_logmag_sum", "l2_log_stft_sum", "l2_comp_stft_sum", "l2_comp_stft_mean",
              "l2_comp_stft_summean"]
TIME_NAMES = ["l2_sum", "l2_mean"]
WEIGHTINGS = [None, "sqrt", "exp", "log", "linear"]
INFORMED = [("l2_stft_mag_sum", "sqrt"), ("l2_log_stft_sum", None), ("l2_comp_stft_sum", "log"), ("l2_sum", None)]
E2E_OVERRIDES = ["tester.posterior_sampling.rec_loss.name=l2_stft_mag_sum",
                 "+tester.posterior_sampling.rec_loss.freq_weighting=sqrt",
                 "tester.posterior_sampling.rec_loss_params.name=l2_log_stft_sum",
                 "tester.posterior_sampling.RIR_noise_regularization.loss.name=l2_sum",
                 "tester.posterior_sampling.blind_hp.op_updates_per_step=3",
                 "tester.posterior_sampling.warm_initialization.mode=reverb_scaled"]


def key(name, fw):
    return f"{name}.{fw or 'none'}"


def grad_weighting(i):
    return WEIGHTINGS[1 + i % 4]


def _case(get_loss, op, y, xh, name, fw, want_grad):
    la = MG.AttrDict(name=name, weight=1.0)
    if "comp" in name:
        la["compression_factor"] = 0.667
    if fw is not None:
        la["freq_weighting"] = fw
    x = xh.clone().requires_grad_(want_grad)
    v = get_loss(la, operator=op)(y, op.degradation(x))
    g = torch.autograd.grad(v, x)[0] if want_grad else None
    return v.detach(), g


def gen_losses():
    from utils.losses import get_loss
    from testing.operators.reverb import RIROperator
    from testing.operators.subband_filtering import BlindSubbandFiltering
    args = MG.compose()
    op_hp = args.tester.informed_dereverberation.op_hp
    L = 8192
    clean = torch.from_numpy(MG.synth_clean(3, L))[None]
    rir = torch.from_numpy(MG.synth_rir(3, taps=1500))
    iop = RIROperator(op_hp, time_kernel_size=rir.shape[-1], sample_rate=16000)
    iop.update_params(rir)
    with torch.no_grad():
        y = iop.degradation(clean)
    xh = 0.9 * clean + 0.02 * torch.from_numpy(MG.synth_clean(4, L))[None]
    ns = MG.NoiseStream(21)
    with MG.patched_noise(ns):
        bop = BlindSubbandFiltering(op_hp, 16000)
        bop.update_H(use_noise=True)
    out = dict(y=y, x_hat=xh, rir=rir, H_head=torch.view_as_real(bop.H.detach())[:, :8], meta=np.array([1, L, 21]))      # H: first 8 filter frames
    for i, name in enumerate(STFT_NAMES):
        for fw in WEIGHTINGS:
            v, g = _case(get_loss, bop, y, xh, name, fw, fw is None or fw == grad_weighting(i))
            out[f"blind.{key(name, fw)}.value"] = v
            if g is not None:
                out[f"blind.{key(name, fw)}.grad"] = g
    for name in TIME_NAMES:
        v, g = _case(get_loss, bop, y, xh, name, None, True)
        out[f"blind.{key(name, None)}.value"], out[f"blind.{key(name, None)}.grad"] = v, g
    for name, fw in INFORMED:
        v, g = _case(get_loss, iop, y, xh, name, fw, True)
        out[f"informed.{key(name, fw)}.value"], out[f"informed.{key(name, fw)}.grad"] = v, g
    MG.save("losses", **out)


def gen_e2e_blind_losses():
    MG._e2e("e2e_blind_losses", "blind_dereverberation_BUDDy", blind=True, T=4, order=1, overrides=E2E_OVERRIDES)
    path = os.path.join(HERE, "e2e_blind_losses.npz")
    d = dict(np.load(path))
    d["overrides"] = np.array(E2E_OVERRIDES)
    np.savez_compressed(path, **d)
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


GENS = {"losses": gen_losses, "e2e_blind_losses": gen_e2e_blind_losses}

if __name__ == "__main__":
    for k in (sys.argv[1:] or list(GENS)):
        GENS[k]()
