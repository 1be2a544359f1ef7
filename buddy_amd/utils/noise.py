"""Diffuse and sensor noise for simulated sets (``tools/make_paired_set.py --snr``): D microphone signals with the spatial
coherence of a diffuse field, by plane-wave superposition (Habets & Gannot 2007), mixed into the simulated speech at a target SNR.  No reference
counterpart: the reference reads its noisy material from a corpus.

The field is the sum of ``N`` uncorrelated white plane waves from fixed directions (``sphere_directions``: a Fibonacci lattice, ``circle_directions``:
equal angles in the horizontal plane); microphone ``d`` at ``p_d`` hears wave ``n`` delayed by ``tau = fs <u_n, p_d> / c`` samples, realised by the
Hann-windowed-sinc fractional delay of the room simulator (``delay_taps``; Hw = 40, |tau| <= M = 64).  ``field_coherence`` is the coherence such a finite
sum has, ``Gamma_N``, which tends to sinc(2 f d / c) (spherical) or J0(2 pi f d / c) (cylindrical).  ``noise_bank_hip`` runs the sum on the GPU through
``csrc/noise.hip`` -- the waves are kind-0 normals of the file's own Philox stream, generated inside the kernel -- and has no CPU form;
``diffuse_noise`` is the whole chain with the optional spectral tilt (``shaping_fir`` through ``buddy_fir``, one kernel for all channels, so the
coherence stays), ``sensor_noise`` independent white noise per microphone, and ``mix_at_snr`` scales both against the speech of channel 0."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib
from . import rng as _rng

HW = 40                                              # half-width of the fractional-delay kernel: buddy_ism_half_width()
MAX_DELAY = 64                                       # M: |tau| above this is refused [samples]: 1.37 m from the array centre at 16 kHz
TAPS = 2 * HW                                        # W: coefficients per (wave, microphone) filter, zero padded
PAD = HW + MAX_DELAY                                 # P: a wave's source runs over j = 0 .. L + 2 P - 1
NOISE_DRAWS, NOISE_FIELD, NOISE_SENSOR = 7, 8, 9     # purposes of utils/rng.py's streams, the next free ones after rooms.ARRAY = 6: the file's SNR
#                                                      draw; draw n = plane wave n; draw d = the sensor noise of microphone d
SHAPING_TAPS = 513
SHAPING_FLOOR_HZ = 50.0                              # the tilt is flat below this: a pink spectrum has no finite power at 0 Hz


def sphere_directions(N):
    """(N, 3) float64 unit vectors of a Fibonacci lattice: z_i = 1 - (2 i + 1) / N, phi_i = pi (1 + sqrt 5) (i + 1/2)"""
    N = int(N)
    if N < 1:
        raise ValueError(f"sphere_directions: N >= 1, got {N}")
    i = np.arange(N, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / N
    phi = np.pi * (1.0 + math.sqrt(5.0)) * (i + 0.5)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def circle_directions(N):
    """(N, 3) float64 unit vectors at N equal angles 2 pi n / N on the horizontal circle"""
    N = int(N)
    if N < 1:
        raise ValueError(f"circle_directions: N >= 1, got {N}")
    phi = 2.0 * np.pi * np.arange(N, dtype=np.float64) / N
    return np.stack([np.cos(phi), np.sin(phi), np.zeros(N)], axis=1)


def directions(field, N):
    if field == "spherical":
        return sphere_directions(N)
    if field == "cylindrical":
        return circle_directions(N)
    raise ValueError(f"the noise field is 'spherical' or 'cylindrical', got {field!r}")


def field_coherence(dirs, pos, freqs, c=343.0):
    """Gamma_N (D, D, F) complex128: the coherence between microphones p and q of the finite sum of equal-power uncorrelated plane waves from
    ``dirs`` (N, 3), Gamma_N[p, q, f] = mean_n exp(-2 pi j f <u_n, p_p - p_q> / c) -- E[X_p conj(X_q)] normalised, for signals delayed by
    <u_n, p_d> / c.  ``pos`` (D, 3) [m], ``freqs`` (F,) [Hz]."""
    dirs, pos, freqs = np.asarray(dirs, dtype=np.float64), np.asarray(pos, dtype=np.float64), np.asarray(freqs, dtype=np.float64).reshape(-1)
    if dirs.ndim != 2 or dirs.shape[1] != 3 or pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError("field_coherence takes (N, 3) directions and (D, 3) positions")
    t = dirs @ pos.T / float(c)                                          # (N, D) seconds
    out = np.empty((pos.shape[0], pos.shape[0], len(freqs)), dtype=np.complex128)
    for p in range(pos.shape[0]):
        diff = t[:, p:p + 1] - t                                         # (N, D)
        out[p] = np.exp(-2j * np.pi * diff[:, :, None] * freqs[None, None, :]).mean(axis=0)
    return out


def delay_taps(pos, dirs, fs, c=343.0):
    """``pos`` (D, 3) [m from the array centre], ``dirs`` (N, 3) -> (taps (N, D, W = 80) float64, first (N, D) int32): per (wave, microphone) the
    fractional-delay filter of tau = fs <u_n, p_d> / c samples, h[lag] = w(lag - tau), w(x) = sinc(x) (1 + cos(pi x / Hw)) / 2 for |x| < Hw and 0
    elsewhere, on the lags first .. first + W - 1 with first = floor(tau) - Hw + 1: all of the support (for an integer tau the last coefficient is the
    zero at x = Hw).  Everything in double.  ValueError for |tau| > M = 64 samples."""
    pos, dirs = np.asarray(pos, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3 or dirs.ndim != 2 or dirs.shape[1] != 3 or not np.all(np.isfinite(pos)) or not np.all(np.isfinite(dirs)):
        raise ValueError("delay_taps takes finite (D, 3) positions and (N, 3) directions")
    fs, c = float(fs), float(c)
    if not (math.isfinite(fs) and fs > 0.0 and math.isfinite(c) and c > 0.0):
        raise ValueError("delay_taps: fs and c must be positive and finite")
    tau = fs * (dirs @ pos.T) / c                                        # (N, D)
    worst = float(np.abs(tau).max())
    if worst > MAX_DELAY:
        raise ValueError(f"delay_taps: a delay of {worst:.2f} samples exceeds M = {MAX_DELAY}: the array is larger than {MAX_DELAY} c / fs = "
                         f"{MAX_DELAY * c / fs:.3f} m from its centre")
    first = np.floor(tau).astype(np.int64) - HW + 1
    x = (first[:, :, None] + np.arange(TAPS)).astype(np.float64) - tau[:, :, None]
    taps = np.where(np.abs(x) < HW, np.sinc(x) * 0.5 * (1.0 + np.cos(np.pi * x / HW)), 0.0)
    taps[(x == np.rint(x)) & (x != 0.0)] = 0.0                           # sinc at an integer is an exact zero (np.sinc leaves 1e-19): an integer tau is a delta
    return taps, first.astype(np.int32)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _keys_host(keys, B=None):
    k = _host(keys)
    if k.dtype == np.int32:
        k = k.view(np.uint32)
    if k.ndim != 2 or k.shape[1] != 2 or k.dtype != np.uint32 or (B is not None and k.shape[0] != B):
        raise ValueError(f"stream keys are (B, 2) uint32 (rng.stream_key per file), got {k.dtype} {tuple(k.shape)}")
    return np.ascontiguousarray(k)


def _keys_device(kh, dev):
    return torch.from_numpy(kh.view(np.int32).copy()).to(dev)


def noise_bank_hip(taps, first, keys, L, purpose=NOISE_FIELD, draw0=0, pad=PAD, scale=None, check_first=True):
    """``taps`` (B, N, D, W) float64, ``first`` (B, N, D) int32 (``delay_taps`` per file), ``keys`` (B, 2) uint32 -- arrays, or tensors on the GPU (the keys then as int32
    holding the uint32 bits, as ``PhiloxStreams`` keeps them) -> (B, D, L) float32 on the GPU: out[b, d, i] = scale sum_n sum_k taps[b, n, d, k] s_{b,n}[i + pad - first[b, n, d] - k] with s_{b,n}[j], j = 0 .. L + 2 pad - 1, the
    kind-0 normals of draw ``draw0 + n`` of ``purpose`` of stream b, and zero outside that range.  ``scale`` defaults to N^(-1/2): unit-power waves sum
    to about unit power.  ValueError for shapes and parameters the kernel does not take and, unless ``check_first`` is off, for a ``first`` whose
    filter leaves the source range (-pad <= first <= pad - W + 1); BuddyHipError for CPU tensors.  No CPU form."""
    given = [a for a in (taps, first, keys) if isinstance(a, torch.Tensor)]
    as_tensor = lambda a: a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))     # checked where it lives
    tt, ft = as_tensor(taps), as_tensor(first)
    if tt.dim() != 4 or tt.dtype != torch.float64:
        raise ValueError(f"noise_bank_hip takes (B, N, D, W) float64 taps, got {tt.dtype} {tuple(tt.shape)}")
    B, N, D, W = tt.shape
    if tuple(ft.shape) != (B, N, D) or ft.dtype != torch.int32:
        raise ValueError(f"noise_bank_hip takes (B, N, D) = {(B, N, D)} int32 first lags, got {ft.dtype} {tuple(ft.shape)}")
    if isinstance(keys, torch.Tensor):
        if tuple(keys.shape) != (B, 2) or keys.dtype != torch.int32:
            raise ValueError(f"stream keys on the GPU are (B, 2) int32 holding the uint32 bits, got {keys.dtype} {tuple(keys.shape)}")
        kt = keys.detach()
    else:
        kt = torch.from_numpy(_keys_host(keys, B).view(np.int32).copy())
    lib = _lib.load()
    L, pad, purpose, draw0 = int(L), int(pad), int(purpose), int(draw0)
    if not (1 <= D <= 8 and 1 <= N <= 4096 and 1 <= W <= lib.buddy_noise_max_taps() and 0 <= pad <= 4096 and 1 <= B <= 65535 and 1 <= L <= 2 ** 33):
        raise ValueError(f"noise_bank_hip: B in 1..65535, N in 1..4096, D in 1..8, W in 1..{lib.buddy_noise_max_taps()}, pad in 0..4096, L in 1..2^33; "
                         f"got B = {B}, N = {N}, D = {D}, W = {W}, pad = {pad}, L = {L}")
    if not (0 <= purpose < 2 ** 32 and 0 <= draw0 and draw0 + N <= 2 ** 32):
        raise ValueError("noise_bank_hip: purpose and the draws draw0 .. draw0 + N - 1 are 32-bit")
    scale = 1.0 / math.sqrt(N) if scale is None else float(scale)
    if not math.isfinite(scale) or not bool(torch.isfinite(tt).all()):
        raise ValueError("noise_bank_hip: the scale and every coefficient must be finite")
    if check_first and (int(ft.min()) < -pad or int(ft.max()) > pad - W + 1):
        raise ValueError(f"noise_bank_hip: a first lag outside {-pad}..{pad - W + 1} reaches outside the source range (got {int(ft.min())}..{int(ft.max())})")
    if any(not a.is_cuda for a in given):
        raise _lib.BuddyHipError("noise_bank_hip: the noise field runs on the MI355X only (got a CPU tensor)")
    lib = _lib.require_gpu()
    dev = given[0].device if given else torch.device("cuda")
    tt, ft, kt = tt.to(dev).contiguous(), ft.to(dev).contiguous(), kt.to(dev).contiguous()
    out = torch.empty(B, D, L, dtype=torch.float32, device=dev)
    _lib.check(lib.buddy_noise_bank(tt.data_ptr(), ft.data_ptr(), kt.data_ptr(), purpose, draw0, _lib.ptr(out), B, D, N, W, pad, L, scale, _lib.stream_ptr()))
    return out


def shaping_fir(fs, tilt, taps=SHAPING_TAPS):
    """(taps,) float64 linear-phase FIR whose POWER gain is ``tilt * log2(max(f, 50 Hz) / 1 kHz)`` dB: 0 is white (a delta), -3 pink, 0 dB at 1 kHz.
    Frequency sampling of the zero-phase magnitude on the power of two >= 4 taps points, centred on tap (taps - 1) / 2, Hann windowed
    (w[n] = (1 + cos(pi (n - P) / (P + 1))) / 2).  ``taps`` odd."""
    fs, tilt, taps = float(fs), float(tilt), int(taps)
    if not (math.isfinite(fs) and fs > 2.0 * SHAPING_FLOOR_HZ) or not math.isfinite(tilt) or abs(tilt) > 24.0:
        raise ValueError("shaping_fir: fs above 100 Hz and a finite tilt of at most 24 dB per octave")
    if taps < 1 or taps % 2 == 0 or taps > 65537:
        raise ValueError(f"shaping_fir: taps must be odd and in 1..65537, got {taps}")
    P = (taps - 1) // 2
    G = 8
    while G < 4 * taps:
        G *= 2
    f = np.arange(G // 2 + 1, dtype=np.float64) * fs / G
    mag = 10.0 ** (tilt * np.log2(np.maximum(f, SHAPING_FLOOR_HZ) / 1000.0) / 20.0)
    t = np.fft.irfft(mag, G)                                             # real and even: zero phase
    return t[np.arange(-P, P + 1) % G] * 0.5 * (1.0 + np.cos(np.pi * np.arange(-P, P + 1, dtype=np.float64) / (P + 1)))


def diffuse_noise(pos, keys, L, fs, waves=512, field="spherical", tilt=0.0, c=343.0, taps=SHAPING_TAPS, purpose=NOISE_FIELD):
    """(B, D, L) float32 on the GPU: per file b a diffuse field of about unit power per channel at the microphones ``pos`` ((D, 3), or (B, D, 3): one
    geometry per file) [m from the array centre], from ``waves`` plane waves of the file's stream ``keys[b]`` (purpose ``NOISE_FIELD``, draw n = wave n).
    ``tilt`` != 0 shapes the spectrum by ``shaping_fir`` -- the field is generated ``taps - 1`` samples longer, all channels go through ``buddy_fir`` with
    the one kernel, and the filter's transient is cut; the power then is that of the shaped spectrum, which ``mix_at_snr`` measures anyway.
    ``purpose`` names the draws' purpose in the stream (default ``NOISE_FIELD``; a room's diffuse tail takes ``rooms.TAIL``)."""
    kh = _keys_host(keys)
    B = kh.shape[0]
    pos = np.asarray(pos, dtype=np.float64)
    if pos.ndim == 2:
        pos = np.broadcast_to(pos, (B,) + pos.shape)
    if pos.ndim != 3 or pos.shape[0] != B or pos.shape[2] != 3:
        raise ValueError(f"diffuse_noise takes (D, 3) or (B = {B}, D, 3) positions, got {tuple(pos.shape)}")
    L = int(L)
    if L < 1:
        raise ValueError("diffuse_noise: L >= 1")
    dirs = directions(field, waves)
    both = [delay_taps(p, dirs, fs, c) for p in pos]
    tp, fr = np.stack([t for t, _ in both]), np.stack([f for _, f in both])
    if float(tilt) == 0.0:
        return noise_bank_hip(tp, fr, kh, L, purpose=purpose)
    h = shaping_fir(fs, tilt, taps)
    M = len(h)
    x = noise_bank_hip(tp, fr, kh, L + M - 1, purpose=purpose)
    D = x.shape[1]
    x = x.reshape(B * D, L + M - 1)
    y = torch.empty_like(x)
    ht = torch.from_numpy(h.astype(np.float32)).to(x.device)
    _lib.check(_lib.load().buddy_fir(_lib.ptr(x), _lib.ptr(ht), 0, _lib.ptr(y), B * D, L + M - 1, M, 0, _lib.stream_ptr()))
    return y[:, M - 1:].reshape(B, D, L).contiguous()


def sensor_noise(keys, D, L):
    """(B, D, L) float32 on the GPU: independent white unit-variance noise per microphone, ``buddy_philox_fill`` kind 0 of purpose ``NOISE_SENSOR``,
    draw d = microphone d of the file's stream"""
    kh = _keys_host(keys)
    B, D, L = kh.shape[0], int(D), int(L)
    if D < 1 or L < 1 or L >= 2 ** 31 or D * B > 65535:
        raise ValueError("sensor_noise: D >= 1, L in 1..2^31 - 1, at most 65535 rows")
    lib = _lib.require_gpu()
    dev = torch.device("cuda")
    out = torch.empty(D, B, L, dtype=torch.float32, device=dev)
    _lib.check(lib.buddy_philox_fill(out.data_ptr(), D, B, L, _keys_device(kh, dev).data_ptr(), NOISE_SENSOR, 0, _rng.NORMAL, _lib.stream_ptr()))
    return out.permute(1, 0, 2).contiguous()


# ---- mixing at a target SNR ---------------------------------------------------------------------------------------------------------------------
class Mix:
    """result of ``mix_at_snr``: ``mixed`` and ``noise`` (B, D, L) float32 where the inputs live (``mixed - noise`` is the speech to fp32 rounding);
    per file, float64 on the host: ``gain_diffuse`` / ``gain_sensor`` as applied (fp32 values; NaN for a kind that was not given), ``speech_power``
    (the reference power of channel 0), ``noise_power`` (of channel 0 of ``noise``), ``snr_measured_db`` = 10 log10 of their ratio; ``reference``:
    per file ``"rms"`` or ``"active"`` as USED; ``flags``: per file ``""``, or ``"ACTIVE_FALLBACK:<the level's flags>"``"""

    def __init__(self, mixed, noise, gain_diffuse, gain_sensor, speech_power, noise_power, snr_measured_db, reference, flags):
        self.mixed, self.noise, self.gain_diffuse, self.gain_sensor = mixed, noise, gain_diffuse, gain_sensor
        self.speech_power, self.noise_power, self.snr_measured_db, self.reference, self.flags = speech_power, noise_power, snr_measured_db, reference, flags


def _is_host(x):
    return isinstance(x, np.ndarray)


def _power(x):
    """mean square per row of (B, L) float32 in double: ``buddy_row_moments`` on the GPU, numpy on host arrays"""
    if _is_host(x):
        return np.sum(x.astype(np.float64) ** 2, axis=1) / x.shape[1]
    x = x.contiguous()
    mom = torch.empty(x.shape[0], 2, dtype=torch.float64, device=x.device)
    _lib.check(_lib.require_gpu().buddy_row_moments(_lib.ptr(x), _lib.ptr(mom), x.shape[0], x.shape[1], _lib.stream_ptr()))
    return mom[:, 1].cpu().numpy() / x.shape[1]


def _axpby(a, x, c, y):
    """a[b] x[b] + c[b] y[b] over the (B, D, L) channels of file b in fp32 (``y`` None: a[b] x[b]): ``buddy_axpby_rows`` on the GPU"""
    B, D, L = x.shape
    a32, c32 = np.repeat(np.asarray(a, dtype=np.float32), D), np.repeat(np.asarray(c, dtype=np.float32), D)
    if _is_host(x):
        out = a32[:, None] * x.reshape(B * D, L)
        if y is not None:
            out = out + c32[:, None] * y.reshape(B * D, L)
        return out.astype(np.float32).reshape(B, D, L)
    x2 = x.reshape(B * D, L).contiguous()
    y2 = None if y is None else y.reshape(B * D, L).contiguous()
    out = torch.empty_like(x2)
    at, ct = torch.from_numpy(a32).to(x.device), torch.from_numpy(c32).to(x.device)
    _lib.check(_lib.require_gpu().buddy_axpby_rows(_lib.ptr(x2), _lib.ptr(y2), _lib.ptr(at), _lib.ptr(ct), _lib.ptr(out), B * D, L, _lib.stream_ptr()))
    return out.reshape(B, D, L)


def mix_at_snr(y, diffuse, sensor, snr_db, sensor_snr_db, fs, reference="rms", level=None):
    """Add noise to the speech ``y`` (B, D, L) float32 -- tensors on the GPU, or numpy arrays for the float64 host form the CPU tests use.

    ``sensor`` (or None) is scaled so that the speech power of channel 0 over the sensor-noise power of channel 0 is ``sensor_snr_db``; ``diffuse``
    (or None) is then scaled so that the speech power over the power of ALL the noise of channel 0, the cross term of the two kinds included, is
    ``snr_db`` (one number, or one per file).  One gain per noise kind serves all channels of a file, so the field's coherence and the level differences
    between the microphones stay.  The powers are sums in double (``buddy_row_moments``), raw (no mean removed).  ``reference``: ``"rms"`` -- the speech
    power is the mean square of channel 0; ``"active"`` -- ``speech_level(..., remove_mean=False).active_rms ** 2``, the ITU-T P.56 power while
    someone speaks; a row whose level carries a flag falls back to ``rms`` and ``Mix.flags`` / ``Mix.reference`` say so.  ``level``: the meter,
    ``(x (B, L), fs) -> SpeechLevel`` (default ``utils.level.speech_level``, which needs the GPU)."""
    if reference not in ("rms", "active"):
        raise ValueError(f"mix_at_snr: reference is 'rms' or 'active', got {reference!r}")
    if diffuse is None and sensor is None:
        raise ValueError("mix_at_snr: no noise given")
    for v in (y, diffuse, sensor):
        if v is None:
            continue
        if isinstance(v, torch.Tensor) and not v.is_cuda:
            raise _lib.BuddyHipError("mix_at_snr: tensors must live on the MI355X (numpy arrays take the float64 host form)")
        if v.ndim != 3 or tuple(v.shape) != tuple(y.shape) or _is_host(v) != _is_host(y) or str(v.dtype).split(".")[-1] != "float32":
            raise ValueError("mix_at_snr takes (B, D, L) float32 speech and noise of one shape, all tensors or all arrays")
    B, D, L = y.shape
    snr = np.broadcast_to(np.asarray(snr_db, dtype=np.float64), (B,)) if diffuse is not None else np.full(B, np.nan)
    if diffuse is not None and not np.all(np.isfinite(snr)):
        raise ValueError("mix_at_snr: snr_db must be finite")
    if sensor is not None and not math.isfinite(float(sensor_snr_db)):
        raise ValueError("mix_at_snr: sensor_snr_db must be finite")
    ch0 = lambda v: v[:, 0, :]
    ps = _power(ch0(y))
    used, flags = ["rms"] * B, [""] * B
    if reference == "active":
        from . import level as _level
        res = (level or (lambda x, r: _level.speech_level(x, r, remove_mean=False)))(ch0(y), fs)
        for b in range(B):
            fl, lv = int(res.flags[b]), float(res.level_db[b])
            if fl == 0 and math.isfinite(lv):
                ps[b], used[b] = 10.0 ** (lv / 10.0), "active"
            else:
                flags[b] = "ACTIVE_FALLBACK:" + _level.flag_text(fl)
    if not np.all(ps > 0.0) or not np.all(np.isfinite(ps)):
        raise ValueError("mix_at_snr: a file's channel 0 has no power")
    f32 = lambda g: np.asarray(g, dtype=np.float32).astype(np.float64)       # the gains as applied
    gs = gd = np.full(B, np.nan)
    scaled = None
    if sensor is not None:
        gs = f32(np.sqrt(ps / (_power(ch0(sensor)) * 10.0 ** (float(sensor_snr_db) / 10.0))))
        scaled = _axpby(gs, sensor, gs, None)
    if diffuse is not None:
        pd, target = _power(ch0(diffuse)), ps / 10.0 ** (snr / 10.0)
        if scaled is None:
            gd = f32(np.sqrt(target / pd))
            noise = _axpby(gd, diffuse, gd, None)
        else:       # gd^2 pd + 2 gd X + pn = target, X the cross term of the diffuse and the scaled sensor noise of channel 0
            pn = _power(ch0(scaled))
            if np.any(pn >= target):
                raise ValueError("mix_at_snr: the sensor noise alone exceeds the noise power snr_db asks for (sensor_snr_db must lie above snr_db)")
            X = 0.5 * (_power(ch0(_axpby(np.ones(B), diffuse, np.ones(B), scaled))) - pd - pn)
            gd = f32((-X + np.sqrt(X * X + pd * (target - pn))) / pd)
            noise = _axpby(gd, diffuse, gs, sensor)
    else:
        noise = scaled
    pn = _power(ch0(noise))
    one = np.ones(B)
    return Mix(_axpby(one, y, one, noise), noise, gd, gs, ps, pn, 10.0 * np.log10(ps / pn), used, flags)
