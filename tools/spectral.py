#!/usr/bin/env python
"""Score a folder of results with the project's spectral distortion measures (buddy_amd/utils/spectral.py): cepstral distance,
log-likelihood ratio and frequency-weighted segmental SNR of every estimate against its clean signal, on the GPU.

    python tools/spectral.py <mode dir>                                    # its original/, degraded/ and reconstructed/
    python tools/spectral.py --reference DIR --estimate DIR [--input DIR] [--out DIR]
    python tools/spectral.py <mode dir> --align [MS]                       # time-align every pair first, within +-MS ms (default 50)

Wavs are matched by file name; int or float wavs of any ONE rate >= 16 kHz per pair (a pair of two rates is refused; a rate above 16 kHz goes through
the project's resampler).  Nothing is time-aligned unless ``--align`` is given; then the pairs are shifted and trimmed exactly as ``tools/evaluate.py
--align`` does, and the lags, their correlations and flags become further columns.  A pair of different lengths is cut to the
shorter, and ``samples`` says so.  Files of equal length and rate are scored as one batch.  Writes ``spectral.csv`` and ``spectral_summary.csv`` (the
tester's files) into the mode directory or ``--out`` (default: the estimate's directory) and prints the summary.  Without ``--input`` the ``_in``
columns are empty.  This is the way to score a multi-rank run as a whole, or the output folders of another implementation."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from buddy_amd.utils import spectral  # noqa: E402
from evaluate import Kind, read_wav, run, score_pairs, wav_names  # noqa: E402,F401  -- the scoring loop and the command line are tools/evaluate.py's

SPECTRAL = Kind(spectral, spectral.FS, "spectral", "measures", "spectral")


def score(reference, estimate, inp=None, values=spectral.VALUES, device="cuda:0", align=None):
    """``score_pairs`` with ``spectral.evaluate``"""
    return score_pairs(SPECTRAL, reference, estimate, inp, values, device, align)


def main(argv=None):
    return run(SPECTRAL, __doc__, argv)


if __name__ == "__main__":
    main()
