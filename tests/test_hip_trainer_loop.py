"""GPU: what tests/test_hip_trainer.py leaves open -- the order inside ``Trainer.training_loop`` (step, EMA, save, ``it += 1``, stop after
``max_iters``), a state dict WRITTEN by torch's Adam loading into ``FusedAdam`` (the other direction of "either loads the other"), and the
gradient of ``output_layer.bias`` on its own.

The bias bounds are derived, not measured.  The gradient is sum_k S[k] b_c[k] with S the column sums of the frame gradient and b_c the bin
sums of the inverse-DFT basis (csrc/wgrad.hip, launch_basis_bias), both in double.  For the real channel b_0[k] = w[k] delta[k] = 0 exactly
(periodic Hann), so component 0 is left with double rounding only: 1e-9 of component 1 is six orders above 2^-53 times any plausible
cancellation and four below what a sum of fp32-rounded spectrum gradients leaves (3.8e-4, profiles/param_grads_accuracy.txt).  Component 1
carries three fp32 roundings per term of the frame gradient (2 x 10^-7); 1e-5 allows a fifty-fold cancellation of the sum."""
import os

import numpy as np
import pytest
import torch

from test_hip_trainer import GOLD, Draws, build_net, make_trainer, _steps

pytestmark = pytest.mark.gpu


def test_output_layer_bias_gradient_vs_float64():
    from test_hip_param_grads import GEOMS, build, gpu_grads, inputs, ref_grads
    g = GEOMS["small"]
    for gemm in ("fp32", "f16x2"):
        net, sd = build(gemm=gemm, **g)
        x, cn, cot = inputs(2, 4096)
        got = gpu_grads(net, x, cn, cot)["output_layer.bias"]
        again = gpu_grads(net, x, cn, cot)["output_layer.bias"]
        ref = ref_grads(sd, x, cn, cot, 126, 32, g["ch_mult"], g["num_res_blocks"], g["fir"])["output_layer.bias"]
        print(f"[{gemm}] output_layer.bias gradient {got} vs float64 {ref}")
        assert got.tobytes() == again.tobytes(), "two runs differ"
        assert abs(ref[0]) <= 1e-9 * abs(ref[1]), "the float64 gradient of the real channel's bias is not ~0: the derivation does not hold"
        assert abs(got[0]) <= 1e-9 * abs(ref[1]), (got, ref)
        assert abs(got[1] - ref[1]) <= 1e-5 * abs(ref[1]), (got, ref)


def test_training_loop_order_and_stop(tmp_path):
    d = np.load(GOLD)
    tr = make_trainer(d, str(tmp_path), max_iters=2)
    tr.args.logging.save_model, tr.args.logging.save_interval = True, 1
    tr.args.logging.remove_old_checkpoints = False
    seen = []
    step, ema, save = tr.train_step, tr.update_ema, tr.save_checkpoint
    tr.train_step = lambda: (seen.append(("step", tr.it)), step())[1]
    tr.update_ema = lambda: (seen.append(("ema", tr.it)), ema())[1]
    tr.save_checkpoint = lambda: (seen.append(("save", tr.it)), save())[1]
    with Draws(d):
        tr.training_loop()
    # it = 0 saves nothing (the reference's `it > 0`), the EMA sees `it` before the increment, the loop stops once it > max_iters
    assert seen == [("step", 0), ("ema", 0), ("step", 1), ("ema", 1), ("save", 1), ("step", 2), ("ema", 2), ("save", 2)], seen
    assert tr.it == 3
    assert sorted(os.listdir(str(tmp_path))) == ["t-1.pt", "t-2.pt"]
    ck = torch.load(str(tmp_path / "t-2.pt"), map_location="cpu", weights_only=False)
    assert ck["it"] == 2 and all(float(s["step"]) == 3.0 for s in ck["optimizer"]["state"].values())


def test_state_written_by_torch_adam_loads_into_fused(tmp_path):
    """two steps of torch.optim.Adam on a second network, its state_dict() into FusedAdam: same moments, same step counts, and the next
    fused step starts from them (m moves by (1 - beta1) g from the loaded value, not from zero)"""
    d = np.load(GOLD)
    net = build_net(d)
    for (_, _, kind, _), p in zip(net._specs, net._params()):
        p.requires_grad_(kind != "fourier")
    from buddy_amd.diff_params.edm import EDM
    from types import SimpleNamespace
    edm = EDM("ve_karras", SimpleNamespace(sigma_data=0.05, sigma_min=1e-5, sigma_max=10, rho=10))
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    with Draws(d):
        for it in range(2):
            opt.zero_grad()
            err, _ = edm.loss_fn(net, torch.from_numpy(d["x"][it]).cuda(), n=None)
            err.mean().backward()
            opt.step()
    sd = opt.state_dict()
    tr = make_trainer(d, str(tmp_path))
    tr.optimizer.load_state_dict(sd)
    mine = tr.optimizer.state_dict()
    assert mine["param_groups"] == sd["param_groups"] and mine["state"].keys() == sd["state"].keys()
    for i, st in sd["state"].items():
        assert float(mine["state"][i]["step"]) == float(st["step"]) == 2.0
        assert torch.equal(mine["state"][i]["exp_avg"], st["exp_avg"]) and torch.equal(mine["state"][i]["exp_avg_sq"], st["exp_avg_sq"])
    flat_m = torch.cat([sd["state"][i]["exp_avg"].reshape(-1) if i in sd["state"] else torch.zeros(p.numel(), device="cuda")
                        for i, p in enumerate(net.parameters())])
    assert torch.equal(tr.optimizer._m, flat_m), "the loaded moments must live in the flat buffer the kernel reads"
    _steps(tr, d, 1, 2)
    assert all(float(s["step"]) == 3.0 for s in tr.optimizer.state_dict()["state"].values())
    assert not torch.equal(tr.optimizer._m, flat_m)
