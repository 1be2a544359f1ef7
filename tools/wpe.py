#!/usr/bin/env python
"""Dereverberate wavs by multichannel WPE alone (buddy_amd/utils/wpe.py), on the GPU: the classical baseline, written as a
folder that goes next to BUDDy's in ``tools/evaluate.py --estimate``, ``tools/srmr.py`` and ``tools/spectral.py``.

    python tools/wpe.py <wavs or a folder> --out DIR [--taps 10] [--delay 3] [--iterations 3] [--fs 16000] [--channel all|K]
                        [--beamformer wmpdr [--bf-iterations 2] [--loading 1e-6]]

Int or float wavs of any rate and up to 8 channels (channels x taps <= 96).  Every file goes to ``--fs`` with the project's resampler, all its
channels through ONE ``wpe_mc_dereverb`` call (the whole file: its workspace is 257 x frames x (32 channels + 8) bytes), and back to its own rate
and exactly its sample count.  ``--channel all`` writes every channel, ``--channel K`` only channel K.  A folder is mirrored under ``--out``
(``<spk>/<id>.wav`` stays ``<spk>/<id>.wav``); single files are written by their base names.  Output: float32 wavs.  A file the kernel cannot
take (too many channels; fewer frames than channels x taps + delay, where the correlation matrix is rank-deficient) is reported and left out.
``--beamformer wmpdr`` puts the wMPDR beamformer behind the WPE in the same call (``wpe_mc_mpdr_dereverb``) and writes its
ONE channel per file; ``--channel K`` then names the reference channel (``all`` means 0).  The defaults are nara_wpe's.  What the front end is
worth in front of BUDDy on a trained checkpoint is unmeasured."""
import argparse
import glob
import os
import sys

import numpy as np
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from buddy_amd.datasets.vctk import _read  # noqa: E402
from buddy_amd.utils import resample, wpe  # noqa: E402


def list_inputs(paths):
    """[(path, name relative to --out)]: the wavs of a folder keep their place in its tree, single files their base name"""
    out = []
    for p in paths:
        if os.path.isdir(p):
            out += [(f, os.path.relpath(f, p)) for f in sorted(glob.glob(os.path.join(p, "**", "*.wav"), recursive=True))]
        else:
            out.append((p, os.path.basename(p)))
    return out


def dereverberate(audio, fs_in, fs, taps, delay, iterations, device="cuda:0", beamformer=None):
    """(C, n) float at ``fs_in`` -> (C, n) float32 on the CPU: to ``fs``, through WPE, back.  ValueError for a shape the kernel does not take.
    ``beamformer`` = (reference, iterations, loading): WPE and the wMPDR beamformer, -> (1, n)."""
    C, n = audio.shape
    y = resample.resample(torch.from_numpy(np.ascontiguousarray(audio)).float().to(device), fs_in, fs)
    if wpe.supported(C, taps) and wpe.frames(y.shape[1]) < C * taps + delay:
        raise ValueError(f"{wpe.frames(y.shape[1])} frames, fewer than channels x taps + delay = {C * taps + delay}")
    if beamformer is not None:
        x = wpe.wpe_mc_mpdr_dereverb(y[None].contiguous(), taps=taps, delay=delay, iterations=iterations, reference=beamformer[0],
                                     bf_iterations=beamformer[1], loading=beamformer[2])
        return resample.resample(x.contiguous(), fs, fs_in)[:, :n].cpu()
    x = wpe.wpe_mc_dereverb(y[None].contiguous(), taps=taps, delay=delay, iterations=iterations)[0]
    return resample.resample(x.contiguous(), fs, fs_in)[:, :n].cpu()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("paths", nargs="+", help="wav files, or folders of them")
    ap.add_argument("--out", required=True)
    ap.add_argument("--taps", type=int, default=10)
    ap.add_argument("--delay", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--fs", type=int, default=16000, help="the rate WPE runs at")
    ap.add_argument("--channel", default="all", help="all, or the index of the one channel to write")
    ap.add_argument("--beamformer", choices=["wmpdr"], default=None, help="beamform the WPE output to one channel; --channel names the reference")
    ap.add_argument("--bf-iterations", type=int, default=2)
    ap.add_argument("--loading", type=float, default=1e-6, help="relative diagonal loading of the beamformer's covariance (a choice)")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.channel != "all" and not (a.channel.isdigit()):
        ap.error("--channel is 'all' or a channel index")
    if a.bf_iterations < 1 or not 0.0 <= a.loading < float("inf"):
        ap.error("--bf-iterations is >= 1 and --loading finite and >= 0")
    inputs = list_inputs(a.paths)
    if not inputs:
        raise SystemExit("wpe: no wav given")
    written = []
    for path, rel in inputs:
        audio, fs_in = _read(path)
        audio = audio[None, :] if audio.ndim == 1 else np.ascontiguousarray(audio.T)
        if a.channel != "all" and int(a.channel) >= audio.shape[0]:
            print(f"skipping {path}: {audio.shape[0]} channel(s), --channel is {a.channel}")
            continue
        bf = None if a.beamformer is None else (0 if a.channel == "all" else int(a.channel), a.bf_iterations, a.loading)
        try:
            x = dereverberate(audio, int(fs_in), a.fs, a.taps, a.delay, a.iterations, a.device, beamformer=bf)
        except ValueError as e:
            print(f"skipping {path}: {e}")
            continue
        x = x.numpy() if a.channel == "all" or bf is not None else x.numpy()[int(a.channel):int(a.channel) + 1]
        dst = os.path.join(a.out, rel)
        os.makedirs(os.path.dirname(dst) or ".", exist_ok=True)
        wavfile.write(dst, int(fs_in), np.ascontiguousarray(x[0] if x.shape[0] == 1 else x.T, dtype=np.float32))
        written.append(dst)
        print(dst)
    return written


if __name__ == "__main__":
    main()
