"""Real recordings for ``Tester.test_real_recordings``: a folder of wav files of any rate, channel count and length.  No reference counterpart
(its test sets are clean/RIR pairs at the model's rate, ``datasets/vctk.py``); nothing is checked, cropped or resampled here -- the tester
brings every file to the model's rate on the GPU."""
from __future__ import annotations

import glob
import os

import numpy as np

from .vctk import _read


class AudioFolder:
    """every ``*.wav`` under ``path`` (recursive) in sorted order; ``num_examples`` = 0 takes all of them.  Items are
    ``(audio float64 mono at the file's own rate, fs, filename)``; several channels are mixed down by their mean, as ``VCTKTrain`` does."""

    def __init__(self, path="", num_examples=0):
        self.files = sorted(glob.glob(os.path.join(path, "**", "*.wav"), recursive=True))
        if int(num_examples) > 0:
            self.files = self.files[:int(num_examples)]

    def __getitem__(self, idx):
        audio, fs = _read(self.files[idx])
        if audio.ndim > 1:
            audio = np.mean(audio, axis=1)
        return audio, int(fs), os.path.basename(self.files[idx])

    def channels(self, idx):
        """the file's channels unmixed: ``((C, n) float64 at the file's own rate, fs, filename)``; a mono file is C = 1.  ``__getitem__`` is their
        mean.  For ``tester.real_recordings.channels: reference | wpe`` and ``tools/wpe.py``."""
        audio, fs = _read(self.files[idx])
        audio = audio[None, :] if audio.ndim == 1 else np.ascontiguousarray(audio.T)
        return audio, int(fs), os.path.basename(self.files[idx])

    def __len__(self):
        return len(self.files)
