"""Float64 arbiter of the stand-alone GroupNorm kernel family (csrc/ops.hip: chan_reduce / group_finalize / csum_collapse / group_finalize_csum /
gn_apply(_m0) / gn_bwd_apply(_m0)): torch only, nothing imported from the library; runs on whatever device its inputs are on.

Every function restates the operation on the fp32 inputs promoted to double (tensors NHWC, a concatenated view handed over as its torch.cat) and
returns the value together with the per-element error bound the fp32 kernel has to meet, so that the tests only compare.  No bound is relative
to a tensor's abs-max.  With u = 2^-24, xh = (x - mean) rstd, z = xh gamma + beta, the bounds count the fp32 roundings on each path:

  e(xh)  = u (3 |xh| + rstd |mean|)                    subtraction, product, rstd's own rounding; the fp32 mean is off by u |mean|
  e(z)   = |gamma| e(xh) + 2u (|xh gamma| + |beta|)
  forward    e(z); behind SiLU 1.1 e(z) + 4u |y| (|SiLU'| <= 1.1; expf, add, divide, product)
  e(da)  = 3u sum|dy| in mode 2 (da is the fp32 sum of four dy), else 0 (one dy, or a quarter of one)
  e(dxh) = |da gamma| (|act''(z)| e(z) + 6u |act'(z)|) + 2u |dxh| + e(da) |gamma act'(z)|
  e(m1)  = group mean of e(dxh) + u |m1| [+ 8u group mean of |dxh|]
  e(m2)  = group mean of (e(dxh) |xh| + |dxh| e(xh) + u |dxh xh|) + u |m2| [+ 8u group mean of |dxh xh|]
           [..]: mode 0 only, whose reduction sums strips of 8 pixels in fp32 before it goes to fp64
  backward   rstd (e(dxh) + e(m1) + |xh| e(m2) + e(xh) |m2| + 4u (|dxh| + |m1| + |xh m2|))
             + 2u |s extra| + u |dx| with an extra gradient (s = extra_scale, a quarter of it in extra_mode 2); + u (|prefill| + |dx|) where the
             destination accumulates
  mode 1 / 2 the same resampling of the per-pixel bounds, + 3u of the result
  stats      mean: u |mean| + 1e-12 E|x|;  rstd: rstd (2u + 1e-12 E[x^2] / (var + eps)) (the kernels form var = E[x^2] - mean^2 in fp64)
  csum       1e-12 of sum|x| and of sum x^2 (fp64 sums)
Behind expf the tests widen a bound to max(bound, 4 e32), e32 from torch's own fp32 ops (fp32_forward / fp32_backward below).

No tests in this module (tests/test_groupnorm_host.py, tests/test_hip_groupnorm.py use it)."""
from collections import namedtuple

import torch

U = 2.0 ** -24
EPS = 1e-6
FP64_SUM = 1e-12
FAMILIES = ("base", "off300", "offm50", "tiny", "off1e4", "const", "gamma", "rows3000")

Stats = namedtuple("Stats", "mean rstd mean_bound rstd_bound")            # (B, G) each
Fwd = namedtuple("Fwd", "y bound pooled_raw pooled_bound stats")
Bwd = namedtuple("Bwd", "dx bound red red_bound")                         # red (B, G, 2) = (m1, m2)
RedSums = namedtuple("RedSums", "n s1 s2 e1 e2 a1 a2")                    # per-group sums over the pixels seen, (B, G) each


def f64(t):
    return None if t is None else t.double()


def f32s(v):
    """a host scalar as the C entry receives it: rounded to fp32, held as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


def per_channel(v, C):
    """(B, G) -> (B, 1, 1, C)"""
    return v.repeat_interleave(C // v.shape[1], dim=1)[:, None, None, :]


def group_sum(a, G):
    """(B, H, W, C) -> (B, G)"""
    B, H, W, C = a.shape
    return a.reshape(B, H * W, G, C // G).sum(dim=(1, 3))


def group_mean(a, G):
    return group_sum(a, G) / (a.shape[1] * a.shape[2] * (a.shape[3] // G))


def pool2(a):
    B, H, W, C = a.shape
    return a.reshape(B, H // 2, 2, W // 2, 2, C).mean(dim=(2, 4))


def up2(a):
    return a.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def stats(x, G, eps=EPS):
    """(mean, rstd) per (utterance, group), the variance two-pass"""
    x = f64(x)
    C = x.shape[3]
    mean = group_mean(x, G)
    var = group_mean((x - per_channel(mean, C)) ** 2, G)
    rstd = 1.0 / torch.sqrt(var + eps)
    return Stats(mean, rstd, U * mean.abs() + FP64_SUM * group_mean(x.abs(), G),
                 rstd * (2 * U + FP64_SUM * group_mean(x * x, G) / (var + eps)))


def chan_sums(x):
    """csum (B, C, 2) = (sum, sum of squares) over the pixels -> (value, bound)"""
    x = f64(x)
    B, H, W, C = x.shape
    v = x.reshape(B, H * W, C)
    return torch.stack([v.sum(1), (v * v).sum(1)], dim=2), FP64_SUM * torch.stack([v.abs().sum(1), (v * v).sum(1)], dim=2)


def _point(x, gamma, beta, st, silu):
    C = x.shape[3]
    mean, rstd = per_channel(st.mean, C), per_channel(st.rstd, C)
    xh = (x - mean) * rstd
    z = xh * gamma + beta
    e_xh = U * (3 * xh.abs() + rstd * mean.abs())
    e_z = gamma.abs() * e_xh + 2 * U * ((xh * gamma).abs() + beta.abs())
    return xh, z, e_xh, e_z, rstd


def forward(x, gamma, beta, G, mode=0, silu=False, st=None):
    """act(GroupNorm(x)), mode 1: its 2x2 mean (pooled_raw: the 2x2 mean of x), mode 2: nearest x2.  st: statistics to use instead of x's own
    (a slab of a larger tensor)."""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    st = st if st is not None else stats(x, G)
    xh, z, e_xh, e_z, _ = _point(x, gamma, beta, st, silu)
    if silu:
        y = z * torch.sigmoid(z)
        e = 1.1 * e_z + 4 * U * y.abs()
    else:
        y, e = z, e_z
    pooled = pooled_b = None
    if mode == 1:
        y, e = pool2(y), pool2(e)
        e = e + 3 * U * y.abs()
        pooled, pooled_b = pool2(x), 4 * U * pool2(x.abs())
    elif mode == 2:
        y, e = up2(y), up2(e)
        e = e + 3 * U * y.abs()
    return Fwd(y, e, pooled, pooled_b, st)


def _bwd_point(x, gamma, beta, dy, st, mode, silu):
    xh, z, e_xh, e_z, rstd = _point(x, gamma, beta, st, silu)
    dy = f64(dy)
    if mode == 0:
        da, e_da = dy, 0.0
    elif mode == 1:
        da, e_da = 0.25 * up2(dy), 0.0
    else:
        da, e_da = 4 * pool2(dy), 3 * U * 4 * pool2(dy.abs())
    if silu:
        s = torch.sigmoid(z)
        a1 = s * (1 + z * (1 - s))
        a2 = s * (1 - s) * (2 + z * (1 - 2 * s))
    else:
        a1, a2 = torch.ones_like(z), torch.zeros_like(z)
    dxh = da * a1 * gamma
    e_dxh = (da * gamma).abs() * (a2.abs() * e_z + 6 * U * a1.abs()) + 2 * U * dxh.abs() + e_da * (gamma * a1).abs()
    return xh, e_xh, rstd, dxh, e_dxh


def backward_sums(x, gamma, beta, G, dy, st, mode=0, silu=False):
    """what the two group means of the backward and their bounds are made of, summed over the pixels of x (add the fields over slabs)"""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    xh, e_xh, _, dxh, e_dxh = _bwd_point(x, gamma, beta, dy, st, mode, silu)
    n = torch.full_like(st.mean, x.shape[1] * x.shape[2] * (x.shape[3] // G))
    return RedSums(n, group_sum(dxh, G), group_sum(dxh * xh, G), group_sum(e_dxh, G),
                   group_sum(e_dxh * xh.abs() + dxh.abs() * e_xh + U * (dxh * xh).abs(), G), group_sum(dxh.abs(), G), group_sum((dxh * xh).abs(), G))


def red_of(sums, mode=0):
    """(red (B, G, 2), bound (B, G, 2)) from backward_sums"""
    m1, m2 = sums.s1 / sums.n, sums.s2 / sums.n
    strip = 8 * U if mode == 0 else 0.0
    e1 = sums.e1 / sums.n + U * m1.abs() + strip * sums.a1 / sums.n
    e2 = sums.e2 / sums.n + U * m2.abs() + strip * sums.a2 / sums.n
    return torch.stack([m1, m2], dim=2), torch.stack([e1, e2], dim=2)


def backward(x, gamma, beta, G, dy, mode=0, silu=False, extra=None, extra_mode=0, extra_scale=1.0, prefill=None, acc=None, st=None, red=None):
    """input-gradient of forward() for dy, + the extra gradient, + prefill where acc (a (C,) 0/1 mask) says the destination accumulates.
    st / red = (value, bound) of red_of: given for a slab of a larger tensor."""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    C = x.shape[3]
    st = st if st is not None else stats(x, G)
    xh, e_xh, rstd, dxh, e_dxh = _bwd_point(x, gamma, beta, dy, st, mode, silu)
    if red is None:
        red = red_of(backward_sums(x, gamma, beta, G, dy, st, mode, silu), mode)
    m1, m2 = per_channel(red[0][:, :, 0], C), per_channel(red[0][:, :, 1], C)
    e1, e2 = per_channel(red[1][:, :, 0], C), per_channel(red[1][:, :, 1], C)
    dx = rstd * (dxh - m1 - xh * m2)
    e = rstd * (e_dxh + e1 + xh.abs() * e2 + e_xh * m2.abs() + 4 * U * (dxh.abs() + m1.abs() + (xh * m2).abs()))
    if extra_mode:
        t = f32s(extra_scale) * f64(extra) if extra_mode == 1 else 0.25 * f32s(extra_scale) * up2(f64(extra))
        dx = dx + t
        e = e + 2 * U * t.abs() + U * dx.abs()
    if acc is not None:
        pre = f64(prefill) * f64(acc)
        dx = dx + pre
        e = e + f64(acc) * U * (pre.abs() + dx.abs())
    return Bwd(dx, e, red[0], red[1])


# ------------------------------------------------------------------------------------------------ torch's own fp32 (the e32 of the SiLU gates)
def fp32_forward(x, gamma, beta, G, st, mode=0):
    """SiLU(GroupNorm(x)) (+ resampling) with torch's fp32 ops on x's device, from the float64 statistics rounded to fp32"""
    C = x.shape[3]
    mean, rstd = per_channel(st.mean.float(), C), per_channel(st.rstd.float(), C)
    y = torch.nn.functional.silu((x - mean) * rstd * gamma + beta)
    return pool2(y) if mode == 1 else up2(y) if mode == 2 else y


def fp32_backward(x, gamma, beta, G, dy, st, red, mode=0):
    """the SiLU backward's core rstd (dxh - m1 - xh m2) with torch's fp32 ops, from the float64 statistics and group means rounded to fp32"""
    C = x.shape[3]
    mean, rstd = per_channel(st.mean.float(), C), per_channel(st.rstd.float(), C)
    m1, m2 = per_channel(red[:, :, 0].float(), C), per_channel(red[:, :, 1].float(), C)
    xh = (x - mean) * rstd
    z = xh * gamma + beta
    s = torch.sigmoid(z)
    da = dy if mode == 0 else 0.25 * up2(dy) if mode == 1 else 4 * pool2(dy)
    return rstd * (da * (s * (1 + z * (1 - s))) * gamma - m1 - xh * m2)


# ------------------------------------------------------------------------------------------------ the input families of the tests
def family(name, B, H, W, C, G, seed):
    """(x (B, H, W, C), gamma, beta) float32 on the CPU"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = torch.randn(B, H, W, C, generator=g)
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    if name in ("base", "gamma", "const", "rows3000"):
        x = r * 1.5 + 0.3
    elif name == "off300":
        x = r + 300.0
    elif name == "offm50":
        x = r * 0.01 - 50.0
    elif name == "tiny":
        x = r * 1e-4
    elif name == "off1e4":
        x = r * 3.0 + 1e4
    else:
        raise ValueError(name)
    if name == "gamma":
        gamma[1] = 0.0
        gamma[C // 2 + 2] = -1.3
    if name == "const":                       # one group of utterance 0 constant: var = 0, rstd = eps^-1/2 = 1000
        cpg = C // G
        g0 = G // 3
        x[0, :, :, g0 * cpg:(g0 + 1) * cpg] = 0.7
    if name == "rows3000":
        x[B - 1] *= 3000.0
    return x.float(), gamma.float(), beta.float()
