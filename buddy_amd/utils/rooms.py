"""Simulated rooms: room impulse responses of shoebox rooms by the image-source method (Allen & Berkley 1979), as defined in DESIGN.md section 20, and
the bookkeeping that turns a folder of clean speech into a paired test set (``tools/make_paired_set.py``).  No reference counterpart: the reference
reads its RIRs from a corpus.

``shoebox_rir`` computes the responses on the GPU through ``csrc/ism.hip`` and has no CPU form.  A room is a row of 16 doubles (``room_row``):
size L (3) [m], source s (3), receiver r (3), the pressure reflection coefficients of the six walls (x = 0, x = Lx, y = 0, y = Ly, z = 0, z = Lz), the
speed of sound c [m/s].  ``eyring_beta`` / ``eyring_t60`` convert between a nominal reverberation time and a uniform coefficient; ``draw_rooms`` draws
one room per file name from the project's counter-based generator; ``room_rows`` / ``write_rooms`` make ``rooms.csv``: what each room is, next to what
``utils/acoustics.rir_acoustics`` measures on its simulated response.  The two are not expected to agree: specular images in a rectangular room decay
more slowly than Eyring's diffuse-field formula says (a 0.30 s nominal room measured T20 = 0.43 s), which is why the file carries both.
``shoebox_rir_hybrid`` (``--diffuse-tail``) closes that gap: images up to a crossover after the direct sound, then a diffuse
noise tail under the room's nominal decay (``csrc/tail.hip``), so the measured T30 meets the nominal T60 and responses of seconds stay cheap.

Banded rooms give the walls their own coefficients per octave band and the air an attenuation per band:
``shoebox_rir_bands`` computes the band responses in double and combines them through ``octave_bank``; ``draw_band_rooms`` tilts the nominal T60 of
``draw_rooms``' room over the bands; ``room_rows`` takes the band block that adds the per-band columns of ``rooms.csv``.

Arrays: ``array_rows`` turns one room into the rows of a uniform circular microphone array around its receiver (``tools/make_paired_set.py --mics``),
``draw_array_angle`` draws its orientation."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib
from . import noise as _noise
from . import rng as _rng
from .acoustics import write_report

ROOMS = 4                                            # purpose number of the room draws in the streams of utils/rng.py (0..3 are the sampler's)
MIN_DISTANCE = 0.01                                  # |s - r| below this makes a row invalid [m]
COLUMNS = ("Lx", "Ly", "Lz", "sx", "sy", "sz", "rx", "ry", "rz", "beta_x0", "beta_x1", "beta_y0", "beta_y1", "beta_z0", "beta_z1", "c")
MEASURED = ("EDT", "T20", "T30", "C50", "DRR")       # broadband values of rir_acoustics that rooms.csv carries
ROOM_BANDS = 5                                       # purpose number of the per-band draws (draw_band_rooms): the next free one after ROOMS
ARRAY = 6                                            # purpose number of a file's array orientation (draw_array_angle): the next free one
ARRAY_RADIUS = 0.1                                   # default radius of a circular array [m]: the REVERB challenge's 8-microphone array
BAND_CENTRES = (125, 250, 500, 1000, 2000, 4000)     # default octave centres of banded rooms [Hz]
BANK_TAPS = 1023                                     # default length of octave_bank's rows: a choice (see there)
TAIL = 10                                            # purpose number of a file's diffuse-tail noise: the next free one after noise.NOISE_SENSOR = 9
TAIL_MS, TAIL_RAMP, TAIL_WAVES = 80.0, 256, 512      # defaults of the diffuse tail: choices nobody has measured
TAIL_PURE, TAIL_ZERO = 2, 4                          # flag bits 1 and 2 of a hybrid response: no tail (n <= n_e); a fit window without energy


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
    return _draw_rooms(names, seed, t60, dims, wall_margin, min_dist, c, max_tries)[0]


def _draw_rooms(names, seed, t60, dims, wall_margin, min_dist, c, max_tries):
    """``draw_rooms`` and, next to the rows, the nominal T60 each was drawn with"""
    lo = np.array([d[0] for d in dims], dtype=np.float64)
    hi = np.array([d[1] for d in dims], dtype=np.float64)
    if not (np.all(lo > 2.0 * wall_margin) and np.all(hi >= lo)):
        raise ValueError("draw_rooms: every size range must be ascending and start above twice the wall margin")
    if not (0 < t60[0] <= t60[1]) or min_dist < MIN_DISTANCE:
        raise ValueError("draw_rooms: the T60 range must be positive and ascending, min_dist at least 0.01 m")
    out = np.empty((len(names), 16), dtype=np.float64)
    nominal = np.empty(len(names), dtype=np.float64)
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
        nominal[b] = T
    return out, nominal


# ---- banded rooms: wall coefficients and air attenuation per octave band ----------------------------------------------------
def array_rows(room, mics, radius=ARRAY_RADIUS, angle=0.0):
    """(mics, 16) float64: the room's row repeated with the receivers of a uniform circular array, one receiver per row (an array is ``mics`` rows
    of one room for ``shoebox_rir``).  The receivers sit on a horizontal circle of ``radius`` [m] around the room's receiver, microphone m at the
    angle ``angle + 2 pi m / mics`` from the x axis, at the receiver's height.  ValueError for a radius that leaves the room."""
    room = np.asarray(room, dtype=np.float64)
    mics, radius, angle = int(mics), float(radius), float(angle)
    if room.shape != (16,):
        raise ValueError(f"array_rows takes one room of 16 doubles, got {tuple(room.shape)}")
    if mics < 1 or not (radius > 0.0 and math.isfinite(radius)) or not math.isfinite(angle):
        raise ValueError("array_rows: mics >= 1, a positive finite radius and a finite angle")
    out = np.tile(room, (mics, 1))
    phi = angle + 2.0 * np.pi * np.arange(mics) / mics
    out[:, 6] = room[6] + radius * np.cos(phi)
    out[:, 7] = room[7] + radius * np.sin(phi)
    if not (np.all(out[:, 6] > 0.0) and np.all(out[:, 6] < room[0]) and np.all(out[:, 7] > 0.0) and np.all(out[:, 7] < room[1])):
        raise ValueError(f"array_rows: an array of radius {radius} m around ({room[6]:.3f}, {room[7]:.3f}) leaves the room of {room[0]:.3f} x {room[1]:.3f} m")
    return out


def draw_array_angle(seed, name):
    """the orientation of a file's array, uniform in [0, 2 pi): draw 0 of purpose ``ARRAY`` of the Philox stream ``rng.stream_key(seed, name)`` --
    a function of (seed, name) alone, as the room is"""
    return float(2.0 * np.pi * _rng.uniforms(_rng.stream_key(seed, name), ARRAY, 0, 1)[0])


def _check_centres(fs, centres):
    cs = tuple(float(f) for f in centres)
    if not cs or not all(math.isfinite(f) and f > 0 for f in cs):
        raise ValueError("band centres must be positive and finite")
    if any(abs(b / a - 2.0) > 1e-9 for a, b in zip(cs, cs[1:])):
        raise ValueError(f"band centres must ascend by octaves, got {cs}")
    if cs[-1] >= 0.5 * float(fs):
        raise ValueError(f"band centres must lie below fs / 2 = {0.5 * float(fs):g} Hz, got {cs[-1]:g}")
    return cs


def octave_bank(fs, centres=BAND_CENTRES, Nh=BANK_TAPS):
    """(len(centres), Nh) float64 zero-phase FIR rows, centred on tap P = (Nh - 1) / 2, that split a signal into octave bands and sum to the unit
    impulse at tap P exactly.  Magnitudes cross-fade as cos^2(pi / 2 * log2(f / f_k)) between neighbouring centres and are 1 below the lowest and
    above the highest centre; designed by frequency sampling on a grid of the power of two >= 4 Nh points, centred, Hann-tapered
    (w[n] = (1 + cos(pi (n - P) / (P + 1))) / 2) to ``Nh`` taps; the LAST row is then replaced by delta_P minus the sum of the others, so a room
    whose bands are all equal is the broadband room delayed by P.  ``Nh`` must be odd; the centres ascend by octaves and lie below fs / 2.  The
    default Nh = 1023 is a choice: the taper's main lobe is 4 fs / (Nh + 1) wide, 62.5 Hz at 16 kHz -- half of the narrowest cross-fade (125 to
    250 Hz) -- for a delay of P = 511 samples, 32 ms."""
    cs = _check_centres(fs, centres)
    Nh = int(Nh)
    if Nh < 1 or Nh % 2 == 0 or Nh > 65537:
        raise ValueError(f"octave_bank: Nh must be odd and in 1..65537, got {Nh}")
    nb, P = len(cs), (Nh - 1) // 2
    G = 8
    while G < 4 * Nh:
        G *= 2
    f = np.arange(G // 2 + 1, dtype=np.float64) * float(fs) / G
    taper = 0.5 * (1.0 + np.cos(np.pi * np.arange(-P, P + 1, dtype=np.float64) / (P + 1)))
    bank = np.zeros((nb, Nh), dtype=np.float64)
    for k, fc in enumerate(cs[:-1]):
        with np.errstate(divide="ignore"):
            x = np.log2(f / fc)                                          # -inf at f = 0
        x = np.clip(x, 0.0 if k == 0 else -1.0, 1.0)
        mag = np.cos(0.5 * np.pi * x) ** 2
        t = np.fft.irfft(mag, G)                                         # real and even: zero phase
        bank[k] = t[np.arange(-P, P + 1) % G] * taper
    bank[nb - 1] = -bank[:nb - 1].sum(axis=0)
    bank[nb - 1, P] += 1.0
    return bank


def eyring_beta_bands(dims, t60s, c=343.0):
    """(len(t60s), 6) float64: per band the uniform coefficient ``eyring_beta(dims, t60s[k], c)`` on all six walls"""
    return np.array([[eyring_beta(dims, float(t), c)] * 6 for t in t60s], dtype=np.float64).reshape(-1, 6)


def nearest_band(centres, f=1000.0):
    """index of the centre nearest ``f`` on the octave axis (the lower one of a tie)"""
    return int(np.argmin([abs(math.log2(float(v) / f)) for v in centres]))


def draw_band_rooms(names, seed, centres=BAND_CENTRES, t60=(0.2, 1.0), slope=(0.0, 0.3), t60_clip=(0.05, 4.0), dims=((3, 8), (3, 8), (2.4, 3.5)),
                    wall_margin=0.5, min_dist=0.5, c=343.0, max_tries=1000):
    """(rooms (n, 16), beta (n, nb, 6), t60s (n, nb)) float64.  Geometry, positions and the nominal T60 are exactly ``draw_rooms``' for the same seed
    and name; the nominal T60 is the value at 1 kHz.  One further uniform, draw 0 of purpose ``ROOM_BANDS`` of the same stream, gives a slope ``s``
    per octave in ``slope``: T60_k = T60 * 2^(-s log2(f_k / 1000)), clipped to ``t60_clip`` [s] -- a positive slope shortens the high bands -- and
    beta[k] = ``eyring_beta(dims, T60_k)`` on all six walls.  The row's own six coefficients are those of the band nearest 1 kHz."""
    cs = tuple(float(f) for f in centres)
    if not cs or not all(f > 0 for f in cs):
        raise ValueError("draw_band_rooms: band centres must be positive")
    if not (slope[0] <= slope[1]) or not (0 < t60_clip[0] <= t60_clip[1]):
        raise ValueError("draw_band_rooms: the slope range must be ascending, the clip range positive and ascending")
    rows, nominal = _draw_rooms(names, seed, t60, dims, wall_margin, min_dist, c, max_tries)
    beta = np.empty((len(names), len(cs), 6), dtype=np.float64)
    t60s = np.empty((len(names), len(cs)), dtype=np.float64)
    k1 = nearest_band(cs)
    for b, name in enumerate(names):
        v = float(_rng.uniforms(_rng.stream_key(seed, name), ROOM_BANDS, 0, 1)[0])
        s = slope[0] + v * (slope[1] - slope[0])
        t60s[b] = np.clip([nominal[b] * 2.0 ** (-s * math.log2(f / 1000.0)) for f in cs], t60_clip[0], t60_clip[1])
        beta[b] = eyring_beta_bands(rows[b, 0:3], t60s[b], c)
        rows[b, 9:15] = beta[b, k1]
    return rows, beta, t60s


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def shoebox_rir_bands(rooms, beta, fs, n, bank, air=None, max_order=-1, max_images=2e8, return_bands=False, t60s=None, keys=None, tail_ms=None,
                      ramp=TAIL_RAMP):
    """``rooms`` (B, 16), ``beta`` (B, nb, 6) pressure reflection coefficients per band and wall, ``air`` (nb,) or (B, nb) pressure attenuations in
    Np/m (None: zeros), all float64 arrays or GPU tensors; ``bank`` (nb, Nh) float64 (``octave_bank``) -> (h (B, n) float32 on the GPU, flags (B,)
    int32 on the CPU[, u (B, nb, n) float64 on the GPU, the band responses]).  The rows' own six coefficients are not read.  h = sum_k bank[k] * u_k
    applied causally: sample n sits at time (n - Hw - P) / fs, P = (Nh - 1) / 2.  An invalid row is zeros with flag 0.  Refuses above ``max_images``
    exactly as ``shoebox_rir`` does.  No CPU form.

    ``tail_ms`` (default None: nothing changes) gives every band a diffuse late tail (``shoebox_rir_hybrid``): the band responses
    are computed up to n_e = n_x + ``ramp`` samples only -- that length is what ``max_images`` then judges -- and mixed in the band domain with ONE
    noise sequence per row (stream ``keys[b]``, purpose ``TAIL``) under the band's own decay 3 ln 10 / ``t60s[b, k]`` + c air[b, k], before the
    combination.  ``t60s`` (B, nb) float64 [s] and ``keys`` (B, 2) uint32 are then required, and the result gains a third value before ``u``:
    (h, flags, info[, u]) with flags and info as ``shoebox_rir_hybrid`` returns them."""
    is_tensor = isinstance(rooms, torch.Tensor)
    host = _host(rooms)
    if host.ndim != 2 or host.shape[1] != 16 or host.dtype != np.float64:
        raise ValueError(f"shoebox_rir_bands takes (B, 16) float64 rooms, got {host.dtype} {tuple(host.shape)}")
    B = host.shape[0]
    bh = _host(beta)
    if bh.ndim != 3 or bh.shape[0] != B or bh.shape[2] != 6 or bh.dtype != np.float64:
        raise ValueError(f"shoebox_rir_bands takes (B, nb, 6) float64 beta, got {bh.dtype} {tuple(bh.shape)}")
    nb = bh.shape[1]
    lib = _lib.load()
    if not 1 <= nb <= lib.buddy_ism_max_bands():
        raise ValueError(f"shoebox_rir_bands: nb must be in 1..{lib.buddy_ism_max_bands()}, got {nb}")
    bk = np.asarray(bank)
    if bk.ndim != 2 or bk.shape[0] != nb or bk.dtype != np.float64 or bk.shape[1] % 2 == 0 or bk.shape[1] > 65537:
        raise ValueError(f"shoebox_rir_bands takes a (nb = {nb}, Nh odd, at most 65537) float64 bank, got {bk.dtype} {tuple(bk.shape)}")
    ah = None
    if air is not None:
        ah = _host(air)
        if ah.dtype != np.float64 or ah.shape not in ((nb,), (B, nb)):
            raise ValueError(f"shoebox_rir_bands takes (nb,) or (B, nb) float64 air, got {ah.dtype} {tuple(ah.shape)}")
        ah = np.array(np.broadcast_to(ah, (B, nb)))
    fs, n, max_order = int(fs), int(n), int(max_order)
    n_out, tail = n, None
    if tail_ms is not None:
        if t60s is None or keys is None:
            raise ValueError("shoebox_rir_bands: a tail needs t60s (B, nb) and keys (B, 2)")
        th = _host(t60s)
        if th.dtype != np.float64 or th.shape != (B, nb) or not np.all(np.isfinite(th) & (th > 0)):
            raise ValueError(f"shoebox_rir_bands takes (B, nb) = {(B, nb)} positive finite float64 t60s, got {th.dtype} {tuple(th.shape)}")
        kh = _noise._keys_host(keys, B)
        win = tail_window(host, fs, tail_ms, ramp)
        delta = 3.0 * math.log(10.0) / th + host[:, 15:16] * (0.0 if ah is None else ah)
        if not np.all(np.isfinite(delta)):
            raise ValueError("shoebox_rir_bands: a band's decay 3 ln 10 / T60 + c air is not finite")
        if n < 1:
            raise ValueError("shoebox_rir_bands: n >= 1")
        n = min(n_out, int(win[:, 3].max()))                             # the image-source part: what the kernel computes and max_images judges
        tail = (win, delta, kh)
    est = estimated_images(host, fs, n, max_order)
    for b, v in enumerate(est):
        if v > float(max_images):
            raise ValueError(f"shoebox_rir_bands: row {b} would sum about {v:.3g} images, above max_images = {float(max_images):.3g}; "
                             "shorten the response, cap the order or raise the limit")
    if is_tensor and not rooms.is_cuda:
        raise _lib.BuddyHipError("shoebox_rir_bands: the simulator runs on the MI355X only (got a CPU tensor)")
    lib = _lib.require_gpu()
    dev = rooms.device if is_tensor else torch.device("cuda")
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    r = (rooms.detach() if is_tensor else on(host)).contiguous()
    bt = (beta.detach().to(dev) if isinstance(beta, torch.Tensor) else on(bh)).contiguous()
    at = None if ah is None else on(ah)
    kt = on(bk)
    u = torch.empty(B, nb, n, dtype=torch.float64, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    st = _lib.stream_ptr()
    _lib.check(lib.buddy_shoebox_bands(r.data_ptr(), bt.data_ptr(), None if at is None else at.data_ptr(), B, nb, fs, n, max_order, u.data_ptr(), n,
                                       flags.data_ptr(), st))
    info = None
    if tail is not None:
        u, amp, tf = _tail_mix(u, n_out, 1, tail[0], int(ramp), tail[1], None, None, tail[2], fs)
        info = _tail_info(tail[0], tail[1], amp, None, 1, int(ramp), float(tail_ms))
        info["ism_samples"], n = n, n_out
    h = torch.empty(B, n, dtype=torch.float32, device=dev)
    _lib.check(lib.buddy_band_combine(u.data_ptr(), B, nb, n, n, kt.data_ptr(), bk.shape[1], _lib.ptr(h), n, st))
    if tail is None:
        return (h, flags.cpu(), u) if return_bands else (h, flags.cpu())
    fl = flags.cpu() | torch.from_numpy(tf.astype(np.int32))
    return (h, fl, info, u) if return_bands else (h, fl, info)


# ---- diffuse late tail: images up to a crossover after the direct sound, then noise under the room's nominal decay --------
def _half_up(x):
    return int(math.floor(x + 0.5))


def tail_window(rooms, fs, tail_ms, ramp, mics=1):
    """(G, 4) int64, G = B / ``mics`` groups of consecutive rows (the microphones of one room): per group (n_d, n_f, n_x, n_e) -- the sample of the
    direct sound n_d = Hw + half_up(min over the group's rows of |s - r| fs / c), the fit window [n_f, n_x) = n_d + half_up(0.5 ``tail_ms`` fs / 1000)
    .. n_d + half_up(``tail_ms`` fs / 1000), and the length n_e = n_x + ``ramp`` of the image-source part.  Host only.  ValueError for rooms that are
    not (B, 16) float64 with B a multiple of ``mics``, a distance or speed that is not positive and finite, ``tail_ms`` not positive and finite,
    ``ramp`` < 1, or an n_e above 2^20 (what the simulator takes)."""
    host = _host(rooms)
    mics, ramp, fs = int(mics), int(ramp), int(fs)
    if host.ndim != 2 or host.shape[1] != 16 or host.dtype != np.float64:
        raise ValueError(f"tail_window takes (B, 16) float64 rooms, got {host.dtype} {tuple(host.shape)}")
    if not 1 <= mics <= 8 or host.shape[0] < 1 or host.shape[0] % mics != 0:
        raise ValueError(f"tail_window: mics in 1..8 and a multiple of it in rows, got mics = {mics}, B = {host.shape[0]}")
    if not (math.isfinite(float(tail_ms)) and float(tail_ms) > 0.0) or ramp < 1 or fs < 1:
        raise ValueError("tail_window: tail_ms positive and finite, ramp >= 1, fs >= 1")
    with np.errstate(all="ignore"):
        lag = np.linalg.norm(host[:, 3:6] - host[:, 6:9], axis=1) * float(fs) / host[:, 15]
    if not np.all(np.isfinite(lag) & (lag > 0.0)):
        raise ValueError("tail_window: every row needs a positive finite distance |s - r| and speed c")
    Hw = _lib.load().buddy_ism_half_width()
    out = np.empty((host.shape[0] // mics, 4), dtype=np.int64)
    for g, v in enumerate(lag.reshape(-1, mics).min(axis=1)):
        n_d = Hw + _half_up(float(v))
        n_x = n_d + _half_up(float(tail_ms) * 1e-3 * fs)
        out[g] = (n_d, n_d + _half_up(0.5 * float(tail_ms) * 1e-3 * fs), n_x, n_x + ramp)
    if np.any(out[:, 1] >= out[:, 2]) or int(out[:, 3].max()) > 2 ** 20:
        raise ValueError("tail_window: tail_ms of at least two samples, and n_e = n_x + ramp of at most 2^20")
    return out


def _tail_mix(u, n, D, win, R, delta, nu, z, kh, fs):
    """``u`` (B, nb, len) fp32 or fp64 on the GPU, the image-source part; ``win`` (G, 4) of ``tail_window``; ``delta`` (G, nb); ``nu`` (B,) or None;
    ``z`` (B, n) fp32 on the GPU, or None with the rows' stream keys ``kh`` (B, 2) uint32 -> (out (B, nb, n) of u's type, amp (B, nb) float64 as
    ``buddy_tail_fit`` left it (A / nu; 0 for a row without tail), flags (B,): TAIL_PURE for a row of a group with n <= n_e, whose output is u itself,
    TAIL_ZERO from the fit).  The kernels run on the groups that get a tail; a row's bits do not depend on the others."""
    lib = _lib.require_gpu()
    B, nb, ln = u.shape
    G = B // D
    dev, st = u.device, _lib.stream_ptr()
    hyb = n > win[:, 3]
    amp, flags = np.zeros((B, nb), dtype=np.float64), np.where(np.repeat(hyb, D), 0, TAIL_PURE).astype(np.int32)
    if not hyb.any():
        return u, amp, flags                                             # ln = n: every n_e is at least n
    out = torch.empty(B, nb, n, dtype=u.dtype, device=dev)
    if not hyb.all():
        out.copy_(u)                                                     # ln = n here too; the rows with a tail are written again below
    rows = np.nonzero(np.repeat(hyb, D))[0]
    sel = torch.from_numpy(rows).to(dev)
    pick = (lambda a: a) if hyb.all() else (lambda a: a.index_select(0, sel).contiguous())
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    us = pick(u.contiguous())
    Bs = us.shape[0]
    wt, dt = on(win[hyb][:, 1:3].astype(np.int32)), on(np.asarray(delta, dtype=np.float64)[hyb])
    nt = None if nu is None else on(np.asarray(nu, dtype=np.float64)[rows])
    zt = None if z is None else pick(z.contiguous())
    kt = None if kh is None else _noise._keys_device(np.ascontiguousarray(kh[rows]), dev)
    at = torch.empty(Bs, nb, dtype=torch.float64, device=dev)
    ft = torch.empty(Bs // D, dtype=torch.int32, device=dev)
    os_ = out if hyb.all() else torch.empty(Bs, nb, n, dtype=u.dtype, device=dev)
    f64 = int(u.dtype == torch.float64)
    _lib.check(lib.buddy_tail_fit(us.data_ptr(), f64, Bs, nb, D, nb * ln, ln, ln, wt.data_ptr(), dt.data_ptr(), None if nt is None else nt.data_ptr(), fs,
                                  at.data_ptr(), ft.data_ptr(), st))
    _lib.check(lib.buddy_tail_mix(us.data_ptr(), f64, Bs, nb, D, nb * ln, ln, ln, wt.data_ptr(), R, dt.data_ptr(), at.data_ptr(),
                                  None if zt is None else zt.data_ptr(), n, None if kt is None else kt.data_ptr(), TAIL, fs, n, os_.data_ptr(), nb * n, n, st))
    if not hyb.all():
        out.index_copy_(0, sel, os_)
    amp[rows] = at.cpu().numpy()
    flags[rows] |= np.repeat(ft.cpu().numpy(), D)
    return out, amp, flags


def _tail_info(win, delta, amp, nu, D, ramp, tail_ms):
    """what ``shoebox_rir_hybrid`` reports: the windows, the decays and the fitted amplitudes A (G, nb) -- the kernel's A / nu of a group's first row
    times that row's nu"""
    A = amp[::D] * (1.0 if nu is None else np.asarray(nu)[::D, None])
    return dict(tail_ms=float(tail_ms), ramp=int(ramp), windows=win, n_d=win[:, 0], n_f=win[:, 1], n_x=win[:, 2], n_e=win[:, 3], delta=delta, amp=A,
                amp_rows=amp, nu=nu)


def tail_field(rooms, mics, fs, waves=TAIL_WAVES, field="spherical"):
    """host part of an array's tail field: per group of ``mics`` rows the microphone positions relative to their mean (G, mics, 3) and
    nu (B,) float64, nu_m = sqrt(sum_waves sum_j taps[n, m, j]^2 / waves) -- the analytic standard deviation of the plane-wave field of
    ``noise.diffuse_noise`` at microphone m, from ``noise.delay_taps`` with the group's own speed of sound"""
    host = _host(rooms)
    pos = host[:, 6:9].reshape(-1, int(mics), 3)
    pos = pos - pos.mean(axis=1, keepdims=True)
    dirs = _noise.directions(field, waves)
    nu = np.concatenate([np.sqrt((_noise.delay_taps(p, dirs, fs, float(c))[0] ** 2).sum(axis=(0, 2)) / len(dirs))
                         for p, c in zip(pos, host[::int(mics), 15])])
    return pos, nu


def shoebox_rir_hybrid(rooms, fs, n, t60, keys, tail_ms=TAIL_MS, ramp=TAIL_RAMP, mics=1, waves=TAIL_WAVES, field="spherical", max_order=-1, max_images=2e8):
    """The image-source response with a diffuse late tail.  ``rooms`` (B, 16) float64, an array or a tensor on the GPU, in
    groups of ``mics`` consecutive rows (``array_rows``); ``t60`` [s], one value, (G,) or (B,) (a group takes its first row's): the Eyring time the
    room was drawn with; ``keys`` (G, 2) uint32, the stream of each group's file -> (h (B, n) float32 on the GPU, flags (B,) int32 on the CPU,
    info).  Per group the image-source part is computed up to n_e = n_x + ``ramp`` samples only (``tail_window``; one call of ``shoebox_rir`` at the
    largest n_e of the batch, which is what ``max_images`` judges), its energy in [n_f, n_x) over all the group's rows fits ONE amplitude A of the
    envelope A exp(-delta t), delta = 3 ln 10 / T60, and from n_x the response cross-fades over ``ramp`` samples into that envelope times white
    Gaussian noise: kind-0 normals of purpose ``TAIL``, draw 0, of the group's stream for ``mics`` = 1; for an array the plane-wave diffuse field of
    ``noise.diffuse_noise`` (``waves`` draws of purpose ``TAIL``, ``field``) at the microphones, each row divided by its analytic standard deviation.
    Below n_x the result is ``shoebox_rir``'s, bit for bit.  flags: bit 0 the simulator's (valid row), bit 1 (``TAIL_PURE``) n <= n_e, the pure
    response of n samples, bit 2 (``TAIL_ZERO``) a fit window without energy (amplitude 0).  info: ``windows`` (G, 4) with its columns as ``n_d``,
    ``n_f``, ``n_x``, ``n_e``; ``delta`` (G, 1); ``amp`` (G, 1) the fitted A; ``amp_rows`` (B, 1) A / nu as applied; ``nu`` (B,) or None;
    ``ism_samples``.  No CPU form."""
    is_tensor = isinstance(rooms, torch.Tensor)
    host = _host(rooms)
    fs, n, D, R, waves = int(fs), int(n), int(mics), int(ramp), int(waves)
    win = tail_window(host, fs, tail_ms, R, D)
    B, G = host.shape[0], host.shape[0] // D
    if n < 1:
        raise ValueError("shoebox_rir_hybrid: n >= 1")
    th = np.asarray(_host(t60), dtype=np.float64)
    if th.shape == (B,) and D > 1:
        th = th[::D]
    if th.shape not in ((), (1,), (G,)) or not np.all(np.isfinite(th) & (th > 0)):
        raise ValueError(f"shoebox_rir_hybrid takes one positive finite t60, or one per group ({G}) or row ({B}), got {tuple(th.shape)}")
    delta = (3.0 * math.log(10.0) / np.broadcast_to(th, (G,))).reshape(G, 1)
    kh = _noise._keys_host(keys, G)
    if D > 1 and not 1 <= waves <= 4096:
        raise ValueError("shoebox_rir_hybrid: waves in 1..4096")
    pos = nu = None
    if D > 1:
        pos, nu = tail_field(host, D, fs, waves, field)
    ln = min(n, int(win[:, 3].max()))
    u, iflags = shoebox_rir(rooms, fs, ln, max_order=max_order, max_images=max_images)
    z = None
    if D > 1 and bool(np.any(n > win[:, 3])):
        cs = host[::D, 15]
        if np.all(cs == cs[0]):
            z = _noise.diffuse_noise(pos, kh, n, fs, waves=waves, field=field, c=float(cs[0]), purpose=TAIL)
        else:
            z = torch.cat([_noise.diffuse_noise(pos[g], kh[g:g + 1], n, fs, waves=waves, field=field, c=float(cs[g]), purpose=TAIL) for g in range(G)])
        z = z.reshape(B, n)
    out, amp, tf = _tail_mix(u[:, None, :], n, D, win, R, delta, nu, z, kh if D == 1 else None, fs)
    info = _tail_info(win, delta, amp, nu, D, R, tail_ms)
    info["ism_samples"] = ln
    return out[:, 0, :], iflags | torch.from_numpy(tf), info


def band_label(f):
    return f"{float(f):g}"


def _equivalent_beta(dims, beta6):
    """the uniform coefficient with the area-weighted mean absorption of six unequal walls: sqrt(1 - mean(1 - beta^2))"""
    lx, ly, lz = (float(v) for v in dims)
    areas = np.array([ly * lz, ly * lz, lx * lz, lx * lz, lx * ly, lx * ly])
    return float(math.sqrt(max(0.0, float(np.sum(areas * np.asarray(beta6, dtype=np.float64) ** 2) / np.sum(areas)))))


def room_rows(names, rooms, fs, n, acoustics, flags=None, bands=None):
    """one dict per room for ``rooms.csv``: the 16 numbers of the room, the nominal (Eyring) T60, |s - r|, the rate, the response length ``n`` (one
    int, or one per row) and the simulator's flag, then the broadband EDT / T20 / T30 / C50 / DRR that ``rir_acoustics`` (``acoustics``, rows in the
    order of ``names``) measured on the simulated response, with its validity bits.  ``bands`` = (centres, beta (B, nb, 6)) of banded rooms adds per
    band ``beta_<f>`` (the coefficient of the walls; for unequal walls the uniform one of the same area-weighted absorption), ``eyring_T60_<f>``, and
    the ``T20_<f>`` / ``T30_<f>`` / ``acoustics_flags_<f>`` that ``acoustics`` holds for that centre (it must have been analysed at these centres);
    the row's own six coefficients are then those of the band nearest 1 kHz, so the columns above stay meaningful."""
    rooms = np.array(rooms, dtype=np.float64).reshape(-1, 16)
    ns = [int(n)] * len(names) if np.isscalar(n) else [int(v) for v in n]
    if bands is not None:
        centres, bbeta = tuple(float(f) for f in bands[0]), np.asarray(bands[1], dtype=np.float64)
        if bbeta.shape != (len(names), len(centres), 6):
            raise ValueError(f"room_rows: the band block takes beta of shape ({len(names)}, {len(centres)}, 6), got {tuple(bbeta.shape)}")
        where = [list(acoustics.bands).index(f) if f in acoustics.bands else -1 for f in centres]
        if min(where) < 0:
            raise ValueError(f"room_rows: the acoustics were analysed at {tuple(acoustics.bands)}, not at every centre of {centres}")
        rooms[:, 9:15] = bbeta[:, nearest_band(centres)]
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
        if bands is not None:
            for k, f in enumerate(centres):
                bk, tag = bbeta[b, k], band_label(f)
                row["beta_" + tag] = float(bk[0]) if np.all(bk == bk[0]) else _equivalent_beta(rm[0:3], bk)
                row["eyring_T60_" + tag] = eyring_t60(rm[0:3], bk, rm[15])
                row["T20_" + tag] = float(acoustics.values[b, where[k], 1])
                row["T30_" + tag] = float(acoustics.values[b, where[k], 2])
                row["acoustics_flags_" + tag] = int(acoustics.flags[b, where[k]])
        rows.append(row)
    return rows


def write_rooms(path, rows):
    write_report(path, rows)
