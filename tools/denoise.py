#!/usr/bin/env python
"""Suppress the noise of wavs with the noise power tracker and spectral post-filter alone (buddy_amd/utils/denoise.py), on the
GPU: the "post-filter alone" baseline, written as a folder that goes next to BUDDy's in ``tools/evaluate.py --estimate``, ``tools/srmr.py`` and
``tools/spectral.py``.  Run on the output folder of ``tools/wpe.py`` it gives the classical chain WPE -> beamformer -> post-filter.

    python tools/denoise.py <wavs or a folder> --out DIR [--gain lsa|wiener] [--floor-db -15] [--fs 16000]

Int or float wavs of any rate and channel count.  Every channel is a row of its own: to ``--fs`` with the project's resampler, through ONE
``denoise`` call per file, and back to its own rate and exactly its sample count.  A folder is mirrored under ``--out`` (``<spk>/<id>.wav`` stays
``<spk>/<id>.wav``); single files are written by their base names.  Output: float32 wavs, and ``denoise.csv`` in ``--out`` with one line per file and
channel: the estimated SNR, the noise level and the attenuation in dB and the flags.  ``--floor-db`` (the lowest gain) is a choice, not a
measurement.  What the post-filter is worth in front of BUDDy on speech and a trained checkpoint is unmeasured."""
import argparse
import glob
import os
import sys

import numpy as np
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.datasets.vctk import _read  # noqa: E402
from buddy_amd.utils import denoise as dn  # noqa: E402
from buddy_amd.utils import resample  # noqa: E402


def list_inputs(paths):
    """[(path, name relative to --out)]: the wavs of a folder keep their place in its tree, single files their base name (as tools/wpe.py)"""
    out = []
    for p in paths:
        if os.path.isdir(p):
            out += [(f, os.path.relpath(f, p)) for f in sorted(glob.glob(os.path.join(p, "**", "*.wav"), recursive=True))]
        else:
            out.append((p, os.path.basename(p)))
    return out


def suppress(audio, fs_in, fs, gain, floor_db, device="cuda:0"):
    """(C, n) float at ``fs_in`` -> ((C, n) float32 on the CPU, the ``Denoised`` of the C rows at ``fs``)"""
    n = audio.shape[1]
    y = resample.resample(torch.from_numpy(np.ascontiguousarray(audio)).float().to(device), fs_in, fs)
    res = dn.denoise(y.contiguous(), gain=gain, floor_db=floor_db)
    return resample.resample(res.out.contiguous(), fs, fs_in)[:, :n].cpu(), res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("paths", nargs="+", help="wav files, or folders of them")
    ap.add_argument("--out", required=True)
    ap.add_argument("--gain", default="lsa", help="lsa (log-spectral amplitude) or wiener")
    ap.add_argument("--floor-db", type=float, default=dn.FLOOR_DB, help="the lowest gain in dB (a choice)")
    ap.add_argument("--fs", type=int, default=16000, help="the rate the post-filter runs at")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.gain not in dn.GAINS:
        raise SystemExit(f"denoise: --gain is one of {list(dn.GAINS)}, got {a.gain!r}")
    if not -120.0 <= a.floor_db <= 0.0:
        raise SystemExit(f"denoise: --floor-db is in [-120, 0] dB, got {a.floor_db}")
    if a.fs < 1000:
        raise SystemExit(f"denoise: --fs is a sample rate of at least 1000 Hz, got {a.fs}")
    inputs = list_inputs(a.paths)
    if not inputs:
        raise SystemExit("denoise: no wav given")
    rows, written = [], []
    for path, rel in inputs:
        audio, fs_in = _read(path)
        audio = audio[None, :] if audio.ndim == 1 else np.ascontiguousarray(audio.T)
        if audio.shape[1] < 1:
            print(f"skipping {path}: no samples")
            continue
        x, res = suppress(audio, int(fs_in), a.fs, a.gain, a.floor_db, a.device)
        C = audio.shape[0]
        names = [rel[:-4] if C == 1 else f"{rel[:-4]}:{c}" for c in range(C)]
        rows += dn.report_rows(names, res)
        dst = os.path.join(a.out, rel)
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        x = x.numpy()
        wavfile.write(dst, int(fs_in), np.ascontiguousarray(x[0] if C == 1 else x.T, dtype=np.float32))
        written.append(dst)
        for r in rows[-C:]:
            print(f"{r['file']}: snr_est {r['snr_est_db']:.6f} dB  noise {r['noise_db']:.6f} dB  att {r['att_db']:.6f} dB  {r['flags']}")
    os.makedirs(a.out, exist_ok=True)
    dn.write_report(os.path.join(a.out, "denoise.csv"), rows)
    if rows:
        print(dn.format_summary(dn.summary_rows(rows)))
    return written, rows


if __name__ == "__main__":
    main()
