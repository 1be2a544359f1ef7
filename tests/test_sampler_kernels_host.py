"""CPU: the float64 arbiter of the sampler-step kernels (tests/_sampler_ref.py) against the product's torch path, the arbiter's FIR pair against
each other, and the argument checks of the sampler entries of the C ABI, which need no GPU."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sampler_ref as R  # noqa: E402

B, L = 3, 257
ROW_GAIN = np.array([0.5, -3.0, 40.0])


class _Fixed:
    """a noise stream whose draw is a given tensor"""

    def __init__(self, t):
        self.t = t

    def randn(self, shape):
        assert tuple(shape) == tuple(self.t.shape)
        return self.t


def _sampler(order, rescale):
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.testing.EulerHeunSamplerDPS import EulerHeunSamplerDPS
    args = compose(overrides=[f"tester.sampling_params.order={order}", "tester.posterior_sampling.constraint_speech_magnitude.speech_scaling=0.0625",
                              f"tester.posterior_sampling.constraint_speech_magnitude.use={'true' if rescale else 'false'}"])
    s = EulerHeunSamplerDPS(torch.nn.Identity(), instantiate(args.diff_params), args)
    s.use_hip_update = False
    return s, args


# sigmas with short mantissas: the torch path squares sigma in the host's fp32 scalar type (t ** 2 of a numpy float32) before it meets the float64
# tensors, the arbiter squares it in double.  0.5 (1 + 0.25) = 0.625, 0.625^2, sqrt(0.625^2 - 0.5^2) = 0.375, 0.25^2 are all exact in fp32, so both
# sides evaluate the same real-number expression and differ in rounding order only.  Likewise speech_scaling = 0.0625: the arbiter rounds it to fp32, as
# the C entry receives it, the torch path keeps the double.
@pytest.mark.parametrize("order,t_next,rescale,gamma", list(itertools.product((1, 2), (0.0, 0.25), (False, True), (0.0, 0.25))))
def test_arbiter_step_equals_torch_path(order, t_next, rescale, gamma):
    """EulerHeunSamplerDPS.step as torch expressions on float64 CPU tensors == _sampler_ref.step to 1e-12 of the abs-max.  The network and the
    operator inside _guided_eval are stubbed by given tensors (the rescale, Tweedie2score and _ode_integrand of _guided_eval itself run)."""
    rs = np.random.RandomState(order * 8 + rescale * 4 + (gamma > 0) * 2 + (t_next > 0))
    x = rs.standard_normal((B, L)) * 0.5
    eps = rs.standard_normal((B, L))
    evals = [(rs.standard_normal((B, L)), ROW_GAIN[[k, (k + 1) % 3, (k + 2) % 3]], rs.standard_normal((B, L)) * np.abs(ROW_GAIN)[:, None] * 0.05)
             for k in range(2)]
    smp, args = _sampler(order, rescale)
    smp.noise = [_Fixed(torch.from_numpy(eps[b:b + 1])) for b in range(B)]
    calls = []
    smp.get_Tweedie_estimate = lambda x_in, t: (calls.append(float(t)), torch.from_numpy(evals[len(calls) - 1][2]))[1]
    smp.get_likelihood_score = lambda x_den, x_in, t: (torch.from_numpy(evals[len(calls) - 1][1][:, None] * evals[len(calls) - 1][0]), None)
    t_i = 0.5
    x_next, x_den = smp.step(torch.from_numpy(x), t_i, t_next, gamma, blind=False)
    (rx, rd), _ = R.step(x, eps, t_i, t_next, gamma, order, evals, rescale, args.tester.posterior_sampling.constraint_speech_magnitude.speech_scaling)
    two = order == 2 and t_next != 0
    assert calls == ([t_i * (1 + gamma), t_next] if two else [t_i * (1 + gamma)])
    assert x_next.dtype == torch.float64 and x_den.dtype == torch.float64
    for name, got, ref in (("x_next", x_next, rx), ("x_den", x_den, rd)):
        err = np.abs(got.numpy() - ref).max() / np.abs(ref).max()
        print(f"step order {order} t_next {t_next} rescale {rescale} gamma {gamma}: {name} rel err {err:.2e}")
        assert err <= 1e-12


@pytest.mark.parametrize("L,M", [(1, 1), (5, 9), (300, 40), (257, 257)])
def test_arbiter_fir_pair_is_a_transpose_pair(L, M):
    """<fir(x), g> == <x, fir_adj(g)> per row to 1e-12, shared and per-row h; and the forward against the plain double loop of its definition"""
    rs = np.random.RandomState(L * 1000 + M)
    x, g = rs.standard_normal((B, L)), rs.standard_normal((B, L))
    for h in (rs.standard_normal(M), rs.standard_normal((B, M)) * ROW_GAIN[:, None]):
        y, gx = R.fir(x, h)[0], R.fir(g, h, adjoint=True)[0]
        for b in range(B):
            hb = h if h.ndim == 1 else h[b]
            lhs, rhs = float(y[b] @ g[b]), float(x[b] @ gx[b])
            scale = float(np.abs(y[b]) @ np.abs(g[b])) + 1e-300
            assert abs(lhs - rhs) <= 1e-12 * scale
            if L <= 300:
                want = np.array([sum(hb[m] * x[b, n - m] for m in range(M) if 0 <= n - m < L) for n in range(L)])
                wadj = np.array([sum(hb[m] * g[b, n + m] for m in range(M) if n + m < L) for n in range(L)])
                assert np.abs(y[b] - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
                assert np.abs(gx[b] - wadj).max() <= 1e-12 * max(np.abs(wadj).max(), 1e-300)


def test_arbiter_row_scale_and_scalars():
    """the arbiter's own definitions at values known in closed form"""
    x = np.array([[1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0], [3.0, 0.0, 4.0, 0.0]])
    v, _ = R.row_scale(x, 0, 0.5)
    assert abs(v[0] - 0.5 / np.sqrt(5.0 / 3.0)) < 1e-15 and np.isposinf(v[1])
    v, _ = R.row_scale(x, 1, 0.5, 2.0)
    assert abs(v[2] - 0.5 / (2.5 + 1e-8)) < 1e-15 and abs(v[1] - 0.5 / 1e-8) < 1e-6
    s, _ = R.edm_scalars(1.0, 0.05)
    assert s[0] == 0.0 and abs(s[2] + (s[3] / 0.05) ** 2 - 1.0) < 1e-15 and abs(s[1] * 0.05 - s[3]) < 1e-15


def test_entries_refuse_bad_arguments_before_any_launch():
    """the argument checks of the sampler entries need no GPU: every one returns BUDDY_ERR_ARG with a message (pointers are never dereferenced)"""
    from buddy_amd import _lib
    lib = _lib.load()
    p, nan = 0x1000, float("nan")
    dps = lambda t, B, L: (p, p, p, p, p, p, p, t, -0.1, 0.5, 0.5, p, p, p, B, L)
    bad = {
        "axpby_rows B": (lib.buddy_axpby_rows, (p, p, p, p, p, 0, 8)), "axpby_rows L": (lib.buddy_axpby_rows, (p, p, p, p, p, 2, 0)),
        "axpby_rows B < 0": (lib.buddy_axpby_rows, (p, None, p, None, p, -1, 8)),
        "row_moments B": (lib.buddy_row_moments, (p, p, 0, 8)), "row_moments L": (lib.buddy_row_moments, (p, p, 2, 0)),
        "perturb n = 0": (lib.buddy_perturb, (p, p, 0.5, p, 0)), "perturb n < 0": (lib.buddy_perturb, (p, p, 0.5, p, -5)),
        "dps_update B": (lib.buddy_dps_update, dps(0.5, 0, 8)), "dps_update L": (lib.buddy_dps_update, dps(0.5, 2, 0)),
        "dps_update t = 0": (lib.buddy_dps_update, dps(0.0, 2, 8)), "dps_update t < 0": (lib.buddy_dps_update, dps(-0.5, 2, 8)),
        "dps_update t NaN": (lib.buddy_dps_update, dps(nan, 2, 8)),
        "fir B": (lib.buddy_fir, (p, p, 0, p, 0, 8, 3, 0)), "fir L": (lib.buddy_fir, (p, p, 0, p, 2, 0, 3, 0)),
        "fir M": (lib.buddy_fir, (p, p, 0, p, 2, 8, 0, 0)), "fir B > 65535": (lib.buddy_fir, (p, p, 0, p, 65536, 8, 3, 1)),
        "row_scale B": (lib.buddy_row_scale, (p, p, 0, 8, 0, 0.05, 1.0)), "row_scale L < 2": (lib.buddy_row_scale, (p, p, 2, 1, 0, 0.05, 1.0)),
        "row_scale mode": (lib.buddy_row_scale, (p, p, 2, 8, 2, 0.05, 1.0)), "row_scale mode < 0": (lib.buddy_row_scale, (p, p, 2, 8, -1, 0.05, 1.0)),
        "row_scale p1 = 0": (lib.buddy_row_scale, (p, p, 2, 8, 1, 0.5, 0.0)), "row_scale p1 < 0": (lib.buddy_row_scale, (p, p, 2, 8, 1, 0.5, -2.0)),
        "row_scale p1 NaN": (lib.buddy_row_scale, (p, p, 2, 8, 1, 0.5, nan)),
        "fill_rows4 B": (lib.buddy_fill_rows4, (p, 0, 1.0, 2.0, 3.0, 4.0)),
    }
    for why, (fn, a) in bad.items():
        assert fn(*a, None) == 2, why
        msg = lib.buddy_last_error().decode()
        assert ("fir" if fn is lib.buddy_fir else "bad arguments" if fn is lib.buddy_fill_rows4 else why.split()[0] + ":") in msg, (why, msg)


def test_fir_function_refuses_a_filter_batch_that_matches_nothing():
    """a 2-D filter whose first dimension is neither 1 nor B used to be read as its row 0 for every utterance"""
    from buddy_amd.utils.reverb_utils import fast_apply_RIR
    x = torch.zeros(3, 16)
    for shape in ((2, 4), (4, 4), (1, 3, 4)):
        with pytest.raises(ValueError):
            fast_apply_RIR(x, torch.zeros(shape))
