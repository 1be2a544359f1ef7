"""Paired clean/RIR test set with the preprocessing of reference ``datasets/vctk.py:148-226`` (``VCTKTestPaired``):
RIR trimmed to its absolute maximum (direct path) and peak-normalised; and the training set ``VCTKTrain`` (``datasets/vctk.py:9-69``):
an endless stream of random fixed-length segments.  Reads wavs with scipy (soundfile is absent)."""
from __future__ import annotations

import glob
import os
import random

import numpy as np
import torch
from scipy.io import wavfile


def _read(path):
    fs, d = wavfile.read(path)
    if d.dtype.kind == "i":
        d = d.astype(np.float64) / np.iinfo(d.dtype).max
    return d.astype(np.float64), fs


class VCTKTestPaired:
    def __init__(self, fs=16000, segment_length=65536, path="", speakers_discard=(), speakers_test=(), normalize=False, seed=0,
                 num_examples=8, shuffle=True):
        if normalize:
            raise NotImplementedError("normalization not implemented yet")
        self.test_samples, self.rir_samples = [], []
        for s in sorted(os.listdir(os.path.join(path, "clean"))):      # sorted: the utterance order must not depend on the file system's listing order
            if s in speakers_discard or (len(speakers_test) and s not in speakers_test):
                continue
            new = sorted(glob.glob(os.path.join(path, "clean", s, "*.wav")))
            self.test_samples.extend(new)
            for f in new:
                self.rir_samples.append(os.path.join(path, "rir", s, os.path.splitext(os.path.basename(f))[0] + ".wav"))
        assert len(self.test_samples) >= num_examples, "error in dataloading: not enough examples"
        if num_examples > 0:
            self.test_samples, self.rir_samples = self.test_samples[:num_examples], self.rir_samples[:num_examples]
        self.fs = fs
        self.test_audio, self.test_rir, self.filenames = [], [], []
        for f, fr in zip(self.test_samples, self.rir_samples):
            data, sr = _read(f)
            rir, sr2 = _read(fr)
            assert sr == fs and sr2 == fs, "wrong sampling rate"
            assert data.ndim == 1 and rir.ndim == 1, "wrong number of channels"
            rir = rir[np.argmax(np.abs(rir)):]
            rir = rir / np.abs(rir).max()
            self.test_audio.append(data); self.test_rir.append(rir); self.filenames.append(os.path.basename(f))

    def __getitem__(self, idx):
        return self.test_audio[idx], self.test_rir[idx], self.filenames[idx]

    def __len__(self):
        return len(self.test_samples)


class VCTKTrain(torch.utils.data.IterableDataset):
    """Endless stream of ``segment_length``-sample float64 segments, the rules of the reference's ``VCTKTrain``: every wav of every speaker
    directory under ``path`` except those in ``speakers_discard`` / ``speakers_test``; a file is drawn with ``random``, mixed to mono by the mean
    over channels, cropped at a ``numpy.random`` offset when longer than the segment and otherwise placed at a random offset and padded by
    wrapping around.  ``seed`` seeds both generators at construction, as the reference does."""

    def __init__(self, fs=16000, segment_length=65536, path="", speakers_discard=(), speakers_test=(), normalize=False, seed=0):
        super().__init__()
        random.seed(seed)
        np.random.seed(seed)
        if normalize:
            raise NotImplementedError("normalization not implemented yet")
        self.train_samples = []
        for s in os.listdir(path):
            if s in speakers_discard or s in speakers_test:
                continue
            self.train_samples.extend(glob.glob(os.path.join(path, s, "*.wav")))
        assert len(self.train_samples) > 0, "error in dataloading: empty or nonexistent folder"
        self.segment_length = int(segment_length)
        self.fs = fs

    def __iter__(self):
        while True:
            f = self.train_samples[random.randint(0, len(self.train_samples) - 1)]
            segment, sr = _read(f)
            assert sr == self.fs, "wrong sampling rate"
            if segment.ndim > 1:
                segment = np.mean(segment, axis=1)
            L = len(segment)
            if L > self.segment_length:
                idx = np.random.randint(0, L - self.segment_length)
                segment = segment[idx:idx + self.segment_length]
            else:
                # numpy's randint needs high > low: a file of exactly the segment length has one placement
                idx = np.random.randint(0, self.segment_length - L) if L < self.segment_length else 0
                segment = np.pad(segment, (idx, self.segment_length - L - idx), "wrap")
            yield segment
