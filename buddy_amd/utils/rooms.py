"""Simulated rooms: room impulse responses of shoebox rooms by the image-source method (Allen & Berkley 1979), as defined in DESIGN.md section 20, and
the bookkeeping that turns a folder of clean speech into a paired test set (``tools/make_paired_set.py``).  No reference counterpart: the reference
reads its RIRs from a corpus.

``shoebox_rir`` computes the responses on the GPU through ``csrc/ism.hip`` and has no CPU form.  A room is a row of 16 doubles (``room_row``):
size L (3) [m], source s (3), receiver r (3), the pressure reflection coefficients of the six walls (x = 0, x = Lx, y = 0, y = Ly, z = 0, z = Lz), the
speed of sound c [m/s].  ``eyring_beta`` / ``eyring_t60`` convert between a nominal reverberation time and a uniform coefficient; ``draw_rooms`` draws
one room per file name from the project's counter-based generator; ``room_rows`` / ``write_rooms`` make ``rooms.csv``: what each room is, next to what
``utils/acoustics.rir_acoustics`` measures on its simulated response.  The two are not expected to agree: specular images in a rectangular room decay
more slowly than Eyring's diffuse-field formula says (a 0.30 s nominal room measured T20 = 0.43 s), which is why the file carries both."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib
from . import rng as _rng
from .acoustics import write_report

ROOMS = 4                                            # purpose number of the room draws in the streams of utils/rng.py (0..3 are the sampler's)
MIN_DISTANCE = 0.01                                  # |s - r| below this makes a row invalid [m]
COLUMNS = ("Lx", "Ly", "Lz", "sx", "sy", "sz", "rx", "ry", "rz", "beta_x0", "beta_x1", "beta_y0", "beta_y1", "beta_z0", "beta_z1", "c")
MEASURED = ("EDT", "T20", "T30", "C50", "DRR")       # broadband values of rir_acoustics that rooms.csv carries


def room_row(dims, source, receiver, beta, c=343.0):
    """one room as 16 doubles; ``beta``: one coefficient for all walls, or six"""
    beta = [float(beta)] * 6 if np.isscalar(beta) else [float(v) for v in beta]
    assert len(dims) == 3 and len(source) == 3 and len(receiver) == 3 and len(beta) == 6
    return np.array([*dims, *source, *receiver, *beta, c], dtype=np.float64)


def _surface_volume(dims):
    lx, ly, lz = (float(v) for v in dims)
    return 2.0 * (lx * ly + ly * lz + lx * lz), lx * ly * lz


def eyring_beta(dims, t60, c=343.0):
    """the uniform pressure reflection coefficient sqrt(1 - alpha) whose Eyring reverberation time is ``t60``:
    alpha = 1 - exp(-24 ln 10 V / (c S T60))"""
    S, V = _surface_volume(dims)
    assert t60 > 0 and c > 0, "eyring_beta: T60 and c must be positive"
    return math.sqrt(math.exp(-24.0 * math.log(10.0) * V / (c * S * float(t60))))


def eyring_t60(dims, beta6, c=343.0):
    """Eyring's reverberation time of a room with the six coefficients ``beta6`` (one value: all walls): 24 ln 10 V / (-c S ln(1 - a)) with a the
    area-weighted mean of the absorptions 1 - beta^2; inf for a lossless room"""
    lx, ly, lz = (float(v) for v in dims)
    S, V = _surface_volume(dims)
    b = [float(beta6)] * 6 if np.isscalar(beta6) else [float(v) for v in beta6]
    areas = (ly * lz, ly * lz, lx * lz, lx * lz, lx * ly, lx * ly)
    a = sum(s * (1.0 - v * v) for s, v in zip(areas, b)) / S
    if a <= 0.0:
        return math.inf
    if a >= 1.0:
        return 0.0
    return 24.0 * math.log(10.0) * V / (-float(c) * S * math.log1p(-a))


def images_within_order(k):
    """the number of images of reflection order <= k: (4 k^3 + 6 k^2 + 8 k + 3) / 3 -- 1, 7, 25, 63, ..."""
    k = int(k)
    return (4 * k ** 3 + 6 * k ** 2 + 8 * k + 3) // 3


def estimated_images(rooms, fs, n, max_order=-1):
    """(B,) float64: the images a row's response of ``n`` samples sums, about (4/3) pi (c n / fs)^3 / (Lx Ly Lz), at most those of the order cap;
    NaN for a row whose size or speed is not positive and finite (the kernel writes such a row as zeros)"""
    rooms = np.asarray(rooms, dtype=np.float64).reshape(-1, 16)
    with np.errstate(all="ignore"):
        est = 4.0 / 3.0 * np.pi * (rooms[:, 15] * float(n) / float(fs)) ** 3 / (rooms[:, 0] * rooms[:, 1] * rooms[:, 2])
    est[~(np.isfinite(est) & (est > 0))] = np.nan
    if max_order >= 0:
        est = np.fmin(est, float(images_within_order(max_order)))
    return est


def shoebox_rir(rooms, fs, n, max_order=-1, max_images=2e8):
    """``rooms`` (B, 16) float64, an array or a tensor on the GPU -> (h (B, n) float32 on the GPU, flags (B,) int32 on the CPU: 1 for a valid row; an
    invalid row is zeros).  ``max_order`` caps the reflection order (-1: none).  Sample n sits at time (n - Hw) / fs, Hw = 40.

    The kernel's work grows with the cube of the response length over the room's volume, and the rooms are data: a row whose estimated image count
    (``estimated_images``) exceeds ``max_images`` is refused with ``ValueError`` before anything is launched.  The default is a choice -- about ten
    times the 1.5 s response of the smallest room ``draw_rooms`` makes -- not a measurement of what the GPU takes in a given time."""
    is_tensor = isinstance(rooms, torch.Tensor)
    host = rooms.detach().cpu().numpy() if is_tensor else np.asarray(rooms)
    if host.ndim != 2 or host.shape[1] != 16 or host.dtype != np.float64:
        raise ValueError(f"shoebox_rir takes (B, 16) float64 rooms, got {host.dtype} {tuple(host.shape)}")
    fs, n, max_order = int(fs), int(n), int(max_order)
    est = estimated_images(host, fs, n, max_order)
    for b, v in enumerate(est):
        if v > float(max_images):
            raise ValueError(f"shoebox_rir: row {b} would sum about {v:.3g} images, above max_images = {float(max_images):.3g}; "
                             "shorten the response, cap the order or raise the limit")
    if is_tensor and not rooms.is_cuda:
        raise _lib.BuddyHipError("shoebox_rir: the simulator runs on the MI355X only (got a CPU tensor)")
    lib = _lib.require_gpu()
    dev = rooms.device if is_tensor else torch.device("cuda")
    r = (rooms.detach() if is_tensor else torch.from_numpy(np.ascontiguousarray(host)).to(dev)).contiguous()
    B = r.shape[0]
    h = torch.empty(B, n, dtype=torch.float32, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.buddy_shoebox_rir(r.data_ptr(), B, fs, n, max_order, _lib.ptr(h), n, flags.data_ptr(), _lib.stream_ptr()))
    return h, flags.cpu()


def draw_rooms(names, seed, t60=(0.2, 1.0), dims=((3, 8), (3, 8), (2.4, 3.5)), wall_margin=0.5, min_dist=0.5, c=343.0, max_tries=1000):
    """(len(names), 16) float64: one room per name, a function of (seed, name) alone -- not of the list or its order.  Size and nominal T60 are
    uniform in their ranges, all walls get ``eyring_beta`` of them; source and receiver are uniform at least ``wall_margin`` from every wall and are
    drawn again (at most ``max_tries`` times, then RuntimeError) until they are ``min_dist`` apart.  The numbers come from the Philox stream
    ``rng.stream_key(seed, name)``, purpose ``ROOMS``: draw 0 is the room, draw 1 + i try i of the positions."""
    lo = np.array([d[0] for d in dims], dtype=np.float64)
    hi = np.array([d[1] for d in dims], dtype=np.float64)
    if not (np.all(lo > 2.0 * wall_margin) and np.all(hi >= lo)):
        raise ValueError("draw_rooms: every size range must be ascending and start above twice the wall margin")
    if not (0 < t60[0] <= t60[1]) or min_dist < MIN_DISTANCE:
        raise ValueError("draw_rooms: the T60 range must be positive and ascending, min_dist at least 0.01 m")
    out = np.empty((len(names), 16), dtype=np.float64)
    for b, name in enumerate(names):
        key = _rng.stream_key(seed, name)
        u = _rng.uniforms(key, ROOMS, 0, 4)
        L = lo + u[:3] * (hi - lo)
        T = float(t60[0] + u[3] * (t60[1] - t60[0]))
        for i in range(int(max_tries)):
            v = _rng.uniforms(key, ROOMS, 1 + i, 6)
            s = wall_margin + v[:3] * (L - 2.0 * wall_margin)
            r = wall_margin + v[3:] * (L - 2.0 * wall_margin)
            if float(np.linalg.norm(s - r)) >= min_dist:
                break
        else:
            raise RuntimeError(f"draw_rooms: no source / receiver pair {min_dist} m apart in {max_tries} tries for {name!r}")
        out[b] = room_row(L, s, r, eyring_beta(L, T, c), c)
    return out


def room_rows(names, rooms, fs, n, acoustics, flags=None):
    """one dict per room for ``rooms.csv``: the 16 numbers of the room, the nominal (Eyring) T60, |s - r|, the rate, the response length ``n`` (one
    int, or one per row) and the simulator's flag, then the broadband EDT / T20 / T30 / C50 / DRR that ``rir_acoustics`` (``acoustics``, rows in the
    order of ``names``) measured on the simulated response, with its validity bits"""
    rooms = np.asarray(rooms, dtype=np.float64).reshape(-1, 16)
    ns = [int(n)] * len(names) if np.isscalar(n) else [int(v) for v in n]
    rows = []
    for b, name in enumerate(names):
        rm = rooms[b]
        row = {"file": name}
        for k, col in enumerate(COLUMNS):
            row[col] = float(rm[k])
        row["eyring_T60"] = eyring_t60(rm[0:3], rm[9:15], rm[15])
        row["distance"] = float(np.linalg.norm(rm[3:6] - rm[6:9]))
        row["fs"], row["n"] = int(fs), ns[b]
        row["flag"] = 1 if flags is None else int(flags[b])
        for q, v in enumerate(MEASURED):
            row[v] = float(acoustics.values[b, 0, q])
        row["acoustics_flags"] = int(acoustics.flags[b, 0])
        rows.append(row)
    return rows


def write_rooms(path, rows):
    write_report(path, rows)
