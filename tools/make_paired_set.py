#!/usr/bin/env python
"""Turn a folder of clean speech into a paired test set with simulated rooms (buddy_amd/utils/rooms.py): one shoebox room per
file, its impulse response computed on the GPU by the image-source method.

    python tools/make_paired_set.py --clean DIR --out DIR [--seed 0] [--fs 16000] [--t60 LO HI] [--dims X0 X1 Y0 Y1 Z0 Z1]
                                    [--rir-seconds S] [--max-order K] [--num N] [--reverberant]
                                    [--bands [F0 F1 ...]] [--t60-slope LO HI] [--air A0 A1 ...]
                                    [--mics N] [--array-radius R]
                                    [--snr LO HI] [--snr-reference rms|active] [--noise-field spherical|cylindrical] [--noise-waves N]
                                    [--noise-tilt DB] [--sensor-snr DB]
                                    [--diffuse-tail [MS]] [--tail-ramp N] [--tail-waves N]

``--clean`` holds ``<spk>/*.wav`` (a flat folder of wavs is the one speaker ``all``); int or float wavs of any rate, several channels averaged to
mono; a file at another rate than ``--fs`` goes through the project's resampler.  Written under ``--out``, the layout ``VCTKTestPaired`` and with it
every paired mode of the tester reads:

    clean/<spk>/<id>.wav        float32 at --fs
    rir/<spk>/<id>.wav          float32, the simulated response as computed: neither trimmed nor normalised (the loader does both)
    rooms.csv                   per file: the room, its nominal (Eyring) T60, and EDT / T20 / T30 / C50 / DRR measured on the response
    reverberant/<spk>/<id>.wav  with --reverberant: the clean file under the loader's form of the RIR (trimmed to its peak, peak 1), through
                                RIROperator.degradation; what the real-recordings mode and tools/srmr.py take

A file's room is a function of ``--seed`` and ``<spk>/<id>`` alone, so the same seed and names reproduce every file byte for byte, whatever else is in
the folder.  The response is 1.5 x the nominal T60 long unless ``--rir-seconds`` fixes it.

``--bands`` gives every room frequency-dependent walls: the nominal T60 holds at 1 kHz and tilts by a drawn slope per octave
(``--t60-slope``), each octave band gets the Eyring coefficient of its own T60, ``--air`` adds a pressure attenuation per band in Np/m (no humidity
model), and the band responses are combined by ``rooms.octave_bank``.  The response then is 1.5 x the longest band's T60 (or ``--rir-seconds``) plus
the bank's delay of (Nh - 1) / 2 samples, which the loader trims with everything else before the peak; ``rooms.csv`` gains per band ``beta_<f>``,
``eyring_T60_<f>`` and the measured ``T20_<f>`` / ``T30_<f>`` / ``acoustics_flags_<f>``.  Without ``--bands`` nothing changes.

``--mics N`` (N > 1) simulates a uniform circular microphone array of radius ``--array-radius`` (default 0.1 m, the REVERB challenge's array) around
the room's receiver, horizontal, its orientation drawn from the file's own stream (``rooms.draw_array_angle``): microphone m sits at
``angle + 2 pi m / N``.  ``rir/`` stays mono -- the response of microphone 0, which the paired modes read as before -- and

    rir_array/<spk>/<id>.wav    all N responses as one N-channel wav, as computed (channel 0 = rir/)
    reverberant/<spk>/<id>.wav  with --reverberant: N channels; all responses are cut at the EARLIEST peak among them and divided by the LARGEST
                                peak, so the delays and level differences between the microphones stay (what MC-WPE and a beamformer use)

``rooms.csv`` gains ``mics``, ``array_radius`` and ``array_angle``; its measured columns are microphone 0's.  Such a folder of N-channel wavs is what
``tester.real_recordings.channels: wpe`` and ``tools/wpe.py`` take.  ``--mics`` with ``--bands`` is refused.  Without ``--mics``, or with
``--mics 1``, nothing changes.

``--snr LO HI`` (with ``--reverberant``) adds noise to the reverberant files (``buddy_amd/utils/noise.py``): a diffuse field at
the array's microphones (``--noise-field``, ``--noise-waves`` plane waves, default 512; one microphone takes 1, because a sum of independent normals
is a normal), white or tilted by ``--noise-tilt`` dB per octave (-3: pink), and with ``--sensor-snr DB`` independent white noise per microphone at
that speech-to-sensor-noise ratio.  A file's SNR is uniform in dB in LO..HI, drawn from the file's own stream, and is the power of the reverberant
speech of channel 0 (``--snr-reference active``: its ITU-T P.56 active power) over the power of ALL the noise of channel 0.  Then

    reverberant/<spk>/<id>.wav  speech plus noise
    noise/<spk>/<id>.wav        the scaled noise alone, same channels: reverberant - noise is the noiseless file

and ``rooms.csv`` gains ``snr_db``, ``snr_reference`` (as used), ``snr_measured_db`` (recomputed in double from the two arrays as written),
``noise_gain_diffuse``, ``noise_gain_sensor`` and ``noise_flags``.  The noise is a function of the seed, the name, the geometry and these flags, so
the same call reproduces every file byte for byte.  ``--snr`` with ``--bands`` is refused.  Without ``--snr`` and ``--sensor-snr`` nothing changes.

``--diffuse-tail [MS]`` (bare: 80) makes every response a hybrid (``rooms.shoebox_rir_hybrid``): the image-source response up
to MS milliseconds after the direct sound, cross-faded over ``--tail-ramp`` samples (default 256) into Gaussian noise under the exponential envelope of
the room's own nominal T60, level-matched to the image-source energy just before the crossover.  Without it a room's measured decay is 1.4 to 2
times the nominal one (specular images of a shoebox decay slowly); with it T20 and T30 land within a few percent of the nominal T60, and responses of
several seconds become simulable, because the images end about MS + ramp after the direct sound whatever the length.  With ``--bands`` the decay is
per band (air included) and one noise sequence serves all bands; with ``--mics`` the tail is a diffuse field at the microphones (``--tail-waves``
plane waves, default 512, the field of ``--noise-field``) with one amplitude for the array.  The length rule (1.5 x nominal) stays.  ``rooms.csv``
gains ``tail_ms``, ``tail_direct`` and ``tail_start`` (the samples of the direct sound and of the crossover), ``tail_ramp``, ``ism_samples`` (the
length of the image-source part), ``tail_amp`` (per band ``tail_amp_<f>``) and ``tail_flags`` (2: the response is shorter than the image-source part
and has no tail; 4: nothing to fit the level to).  The tail is a function of the seed, the name, the geometry and these flags, so the same call
reproduces every file byte for byte.  Without ``--diffuse-tail`` nothing changes."""
import argparse
import os
import sys

import numpy as np
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.datasets.vctk import _read  # noqa: E402
from buddy_amd.utils import acoustics, noise, resample, rng, rooms  # noqa: E402


def read_wav(path):
    """(float32 mono samples, rate) through the loaders' own reader; several channels are averaged, as the real-recordings mode reads them"""
    a, fs = _read(path)
    if a.ndim > 1:
        a = np.mean(a, axis=1)
    if len(a) < 1:
        raise SystemExit(f"make_paired_set: {path} is empty")
    return np.ascontiguousarray(a, dtype=np.float32), int(fs)


def list_clean(base):
    """[(speaker, id, path)] sorted by speaker, then file"""
    wavs = lambda d: sorted(f for f in os.listdir(d) if f.lower().endswith(".wav"))
    out = [("all", f[:-4], os.path.join(base, f)) for f in wavs(base)]
    for spk in sorted(d for d in os.listdir(base) if os.path.isdir(os.path.join(base, d))):
        out += [(spk, f[:-4], os.path.join(base, spk, f)) for f in wavs(os.path.join(base, spk))]
    return out


def add_noise(a, name, y, angle):
    """y (D, L) float32, the reverberant microphone signals of one file -> (y + noise, noise, the file's columns of rooms.csv)"""
    D, L = y.shape
    key = np.array([rng.stream_key(a.seed, name)], dtype=np.uint32)
    yt = torch.from_numpy(np.ascontiguousarray(y))[None].to(a.device)
    diffuse = sensor = None
    snr = float("nan")
    if a.snr is not None:
        snr = a.snr[0] + float(rng.uniforms(key[0], noise.NOISE_DRAWS, 0, 1)[0]) * (a.snr[1] - a.snr[0])
        phi = angle + 2.0 * np.pi * np.arange(D) / D
        pos = np.stack([a.array_radius * np.cos(phi), a.array_radius * np.sin(phi), np.zeros(D)], axis=1) if D > 1 else np.zeros((1, 3))
        try:
            diffuse = noise.diffuse_noise(pos, key, L, a.fs, waves=a.noise_waves if D > 1 else 1, field=a.noise_field, tilt=a.noise_tilt)
        except ValueError as e:
            raise SystemExit(f"make_paired_set: {name}: {e}")
    if a.sensor_snr is not None:
        sensor = noise.sensor_noise(key, D, L)
    m = noise.mix_at_snr(yt, diffuse, sensor, snr, a.sensor_snr, a.fs, reference=a.snr_reference)
    mixed, nz = m.mixed[0].cpu().numpy(), m.noise[0].cpu().numpy()
    pn = float(np.sum(nz[0].astype(np.float64) ** 2))
    ps = float(np.sum((mixed[0].astype(np.float64) - nz[0].astype(np.float64)) ** 2)) if m.reference[0] == "rms" else float(m.speech_power[0]) * L
    cols = dict(snr_db=snr if a.snr is not None else float(a.sensor_snr), snr_reference=m.reference[0], snr_measured_db=10.0 * np.log10(ps / pn),
                noise_gain_diffuse=float(m.gain_diffuse[0]), noise_gain_sensor=float(m.gain_sensor[0]), noise_flags=m.flags[0])
    return mixed, nz, cols


def write_reverberant(a, spk, uid, name, y, angle, row):
    """y (D, L) float32 -> reverberant/<spk>/<id>.wav (mono for D = 1), with the noise flags also noise/<spk>/<id>.wav and the row's noise columns"""
    out = [("reverberant", y)]
    if a.snr is not None or a.sensor_snr is not None:
        mixed, nz, cols = add_noise(a, name, y, angle)
        row.update(cols)
        out = [("reverberant", mixed), ("noise", nz)]
    for sub, v in out:
        os.makedirs(os.path.join(a.out, sub, spk), exist_ok=True)
        wavfile.write(os.path.join(a.out, sub, spk, uid + ".wav"), a.fs, np.ascontiguousarray(v.T) if len(v) > 1 else v[0])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--clean", required=True, help="folder of <spk>/*.wav (or of wavs)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fs", type=int, default=16000)
    ap.add_argument("--t60", type=float, nargs=2, default=(0.2, 1.0), metavar=("LO", "HI"), help="range of the nominal T60 [s]")
    ap.add_argument("--dims", type=float, nargs=6, default=(3, 8, 3, 8, 2.4, 3.5), metavar=("X0", "X1", "Y0", "Y1", "Z0", "Z1"), help="ranges of the room size [m]")
    ap.add_argument("--rir-seconds", type=float, default=None, help="length of every response (default: 1.5 x its nominal T60)")
    ap.add_argument("--max-order", type=int, default=-1, help="cap of the reflection order (default: none)")
    ap.add_argument("--num", type=int, default=0, help="take only the first N files")
    ap.add_argument("--reverberant", action="store_true", help="also write reverberant/<spk>/<id>.wav")
    ap.add_argument("--bands", type=float, nargs="*", default=None, metavar="F",
                    help="banded rooms: octave centres [Hz] with their own wall coefficients (bare: 125 250 500 1000 2000 4000)")
    ap.add_argument("--t60-slope", type=float, nargs=2, default=(0.0, 0.3), metavar=("LO", "HI"),
                    help="with --bands: range of the slope s per octave, T60_k = T60 2^(-s log2(f_k / 1000))")
    ap.add_argument("--air", type=float, nargs="+", default=None, metavar="A", help="with --bands: pressure attenuation of the air per band [Np/m] (default: zeros)")
    ap.add_argument("--mics", type=int, default=1, help="microphones of a uniform circular array around the receiver (default 1: the receiver itself)")
    ap.add_argument("--array-radius", type=float, default=rooms.ARRAY_RADIUS, help="with --mics: radius of the array [m]")
    ap.add_argument("--snr", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="with --reverberant: add noise at a per-file SNR uniform in LO..HI dB")
    ap.add_argument("--snr-reference", choices=("rms", "active"), default="rms", help="the speech power of an SNR: mean square, or ITU-T P.56 active power")
    ap.add_argument("--noise-field", choices=("spherical", "cylindrical"), default="spherical")
    ap.add_argument("--noise-waves", type=int, default=512, help="plane waves of the diffuse field (one microphone: 1)")
    ap.add_argument("--noise-tilt", type=float, default=0.0, help="spectral tilt of the diffuse noise [dB per octave] (0 white, -3 pink)")
    ap.add_argument("--sensor-snr", type=float, default=None, metavar="DB", help="with --reverberant: independent white noise per microphone at this SNR")
    ap.add_argument("--diffuse-tail", type=float, nargs="?", const=rooms.TAIL_MS, default=None, metavar="MS",
                    help="diffuse late tail from MS milliseconds after the direct sound (bare: 80)")
    ap.add_argument("--tail-ramp", type=int, default=rooms.TAIL_RAMP, help="with --diffuse-tail: samples of the cross-fade")
    ap.add_argument("--tail-waves", type=int, default=rooms.TAIL_WAVES, help="with --diffuse-tail and --mics: plane waves of the tail's diffuse field")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    noisy = a.snr is not None or a.sensor_snr is not None
    if noisy and not a.reverberant:
        raise SystemExit("make_paired_set: --snr / --sensor-snr needs --reverberant (the noise is added to the reverberant files)")
    if noisy and a.bands is not None:
        raise SystemExit("make_paired_set: --snr / --sensor-snr with --bands is not supported")
    if a.snr is not None and not a.snr[0] <= a.snr[1]:
        raise SystemExit("make_paired_set: --snr takes LO <= HI")
    if a.snr is not None and not 1 <= a.noise_waves <= 4096:
        raise SystemExit("make_paired_set: --noise-waves takes a count in 1..4096")
    if a.snr is not None and a.sensor_snr is not None and not a.sensor_snr > a.snr[1]:
        raise SystemExit("make_paired_set: --sensor-snr must lie above --snr HI (the SNR counts all the noise, the sensors' included)")
    if a.bands is None and a.air is not None:
        raise SystemExit("make_paired_set: --air needs --bands")
    if a.mics < 1:
        raise SystemExit("make_paired_set: --mics takes a count >= 1")
    if a.mics > 1 and a.bands is not None:
        raise SystemExit("make_paired_set: --mics with --bands is not supported (banded rooms are simulated for one receiver)")
    tailed = a.diffuse_tail is not None
    if tailed and not (a.diffuse_tail > 0.0 and np.isfinite(a.diffuse_tail)):
        raise SystemExit("make_paired_set: --diffuse-tail takes a positive number of milliseconds")
    if tailed and a.tail_ramp < 1:
        raise SystemExit("make_paired_set: --tail-ramp takes a count >= 1")
    if tailed and a.mics > 8:
        raise SystemExit("make_paired_set: --diffuse-tail with --mics takes at most 8 microphones")
    if tailed and a.mics > 1 and not 1 <= a.tail_waves <= 4096:
        raise SystemExit("make_paired_set: --tail-waves takes a count in 1..4096")
    files = list_clean(a.clean)
    if a.num > 0:
        files = files[:a.num]
    if not files:
        raise SystemExit(f"make_paired_set: no wav under {a.clean}")
    names = [f"{spk}/{uid}" for spk, uid, _ in files]
    dims = tuple((a.dims[2 * k], a.dims[2 * k + 1]) for k in range(3))
    if a.bands is None:
        drawn = rooms.draw_rooms(names, a.seed, t60=tuple(a.t60), dims=dims)
    else:
        centres = tuple(a.bands) if a.bands else tuple(float(f) for f in rooms.BAND_CENTRES)
        bank = rooms.octave_bank(a.fs, centres)
        delay = (bank.shape[1] - 1) // 2
        air = np.zeros(len(centres)) if a.air is None else np.array(a.air, dtype=np.float64)
        if air.shape != (len(centres),):
            raise SystemExit(f"make_paired_set: --air takes one value per band ({len(centres)}), got {len(air)}")
        drawn, band_beta, band_t60 = rooms.draw_band_rooms(names, a.seed, centres, t60=tuple(a.t60), slope=tuple(a.t60_slope), dims=dims)
    if a.reverberant:
        from buddy_amd.config import compose
        from buddy_amd.testing.operators.reverb import RIROperator
        op_hp = compose().tester.informed_dereverberation.op_hp
    rows = []
    for u, ((spk, uid, path), name, rm) in enumerate(zip(files, names, drawn)):
        x, fs_in = read_wav(path)
        xt = torch.from_numpy(x).to(a.device)
        if fs_in != a.fs:
            xt = resample.resample(xt, fs_in, a.fs)
        nominal = rooms.eyring_t60(rm[0:3], rm[9:15], rm[15])
        if a.bands is None:
            n = int(round((a.rir_seconds if a.rir_seconds is not None else 1.5 * nominal) * a.fs))
            if a.mics > 1:          # an array is a.mics rows of one room; everything below that reads h[0] reads microphone 0
                angle = rooms.draw_array_angle(a.seed, name)
                try:
                    rm_all = rooms.array_rows(rm, a.mics, a.array_radius, angle)
                except ValueError as e:
                    raise SystemExit(f"make_paired_set: {name}: {e}")
                rm = rm_all[0]
            else:
                rm_all = rm[None]
            rt = torch.from_numpy(np.ascontiguousarray(rm_all)).to(a.device)
            if not tailed:
                h, flags = rooms.shoebox_rir(rt, a.fs, n, max_order=a.max_order)
            else:
                try:
                    h, flags, info = rooms.shoebox_rir_hybrid(rt, a.fs, n, nominal, np.array([rng.stream_key(a.seed, name)], dtype=np.uint32), a.diffuse_tail,
                                                              a.tail_ramp, a.mics, a.tail_waves, a.noise_field, max_order=a.max_order)
                except ValueError as e:
                    raise SystemExit(f"make_paired_set: {name}: {e}")
            ac = acoustics.rir_acoustics(h[:1], a.fs)
            rows += rooms.room_rows([name], rm[None], a.fs, n, ac, flags & 1)
            if a.mics > 1:
                rows[-1].update(mics=a.mics, array_radius=float(a.array_radius), array_angle=angle)
                os.makedirs(os.path.join(a.out, "rir_array", spk), exist_ok=True)
                wavfile.write(os.path.join(a.out, "rir_array", spk, uid + ".wav"), a.fs, np.ascontiguousarray(h.cpu().numpy().astype(np.float32).T))
        else:           # the longest band decides the length, and the bank's delay comes on top of it
            n = int(round((a.rir_seconds if a.rir_seconds is not None else 1.5 * float(band_t60[u].max())) * a.fs)) + delay
            if not tailed:
                h, flags = rooms.shoebox_rir_bands(torch.from_numpy(rm[None]).to(a.device), band_beta[u:u + 1], a.fs, n, bank, air=air, max_order=a.max_order)
            else:
                try:
                    h, flags, info = rooms.shoebox_rir_bands(torch.from_numpy(rm[None]).to(a.device), band_beta[u:u + 1], a.fs, n, bank, air=air,
                                                             max_order=a.max_order, t60s=band_t60[u:u + 1],
                                                             keys=np.array([rng.stream_key(a.seed, name)], dtype=np.uint32), tail_ms=a.diffuse_tail,
                                                             ramp=a.tail_ramp)
                except ValueError as e:
                    raise SystemExit(f"make_paired_set: {name}: {e}")
            ac = acoustics.rir_acoustics(h, a.fs, centres=centres)
            rows += rooms.room_rows([name], rm[None], a.fs, n, ac, flags & 1, bands=(centres, band_beta[u:u + 1]))
        if tailed:
            rows[-1].update(tail_ms=float(a.diffuse_tail), tail_direct=int(info["n_d"][0]), tail_start=int(info["n_x"][0]), tail_ramp=int(a.tail_ramp),
                            ism_samples=int(info["ism_samples"]))
            if a.bands is None:
                rows[-1]["tail_amp"] = float(info["amp"][0, 0])
            else:
                rows[-1].update({"tail_amp_" + rooms.band_label(f): float(info["amp"][0, k]) for k, f in enumerate(centres)})
            rows[-1]["tail_flags"] = int(flags[0]) & (rooms.TAIL_PURE | rooms.TAIL_ZERO)
        for sub, v in (("clean", xt), ("rir", h[0])):
            os.makedirs(os.path.join(a.out, sub, spk), exist_ok=True)
            wavfile.write(os.path.join(a.out, sub, spk, uid + ".wav"), a.fs, v.cpu().numpy().astype(np.float32))
        if a.reverberant and a.mics > 1:      # one cut and one scale for all microphones: the differences between them are the array's signal
            hc = h.cpu()
            start = int(torch.argmax(hc.abs(), dim=1).min())
            hc = hc[:, start:] / hc.abs().max()
            ys = []
            for k in hc:
                op = RIROperator(op_hp, time_kernel_size=len(k), sample_rate=a.fs, device=a.device)
                op.update_params(k)
                ys.append(op.degradation(xt[None])[0].detach().cpu().numpy().astype(np.float32))
            write_reverberant(a, spk, uid, name, np.stack(ys), angle, rows[-1])
        elif a.reverberant:
            hc = h[0].cpu()
            k = hc[int(torch.argmax(hc.abs())):]
            k = k / k.abs().max()
            op = RIROperator(op_hp, time_kernel_size=len(k), sample_rate=a.fs, device=a.device)
            op.update_params(k)
            y = op.degradation(xt[None])[0]
            write_reverberant(a, spk, uid, name, y.detach().cpu().numpy().astype(np.float32)[None], 0.0, rows[-1])
        print(f"{name}: {rm[0]:.2f} x {rm[1]:.2f} x {rm[2]:.2f} m, nominal T60 {nominal:.3f} s, {n} samples, measured T20 {rows[-1]['T20']:.3f} s")
    rooms.write_rooms(os.path.join(a.out, "rooms.csv"), rows)
    print(os.path.join(a.out, "rooms.csv"))
    return rows


if __name__ == "__main__":
    main()
