"""What every measure of ragged (B, L) rows does before its library calls (utils/metrics.py, utils/spectral.py, utils/srmr.py): the entry check, the
step to the rate the measure is defined at, and the gain that matches an estimate's energy to its clean signal's.  A new measure starts here."""
import torch

from .. import _lib
from . import resample as _rs


def lengths(lens, B, L):
    """(B,) int32 on the CPU: ``lens``, or L per row where it is None; every length must be in 1..L"""
    lens_t = torch.full((B,), L, dtype=torch.int32) if lens is None else torch.as_tensor(lens, dtype=torch.int32).reshape(B).cpu()
    assert int(lens_t.min()) >= 1 and int(lens_t.max()) <= L, "every length must be in 1..L"
    return lens_t


def enter(rows, lens, cpu, shape, fs=None, min_fs=None, rate=None):
    """The entry check of a measure of one or two row tensors -> (the library, the rows contiguous, ``lengths``).  A CPU tensor raises ``BuddyHipError``
    with the text ``cpu``; the rows must be (B, L) float32 of one shape (``shape``: the assertion's text); with ``rate`` given, ``fs`` must be an integer
    >= ``min_fs`` or a ``ValueError`` carries that text."""
    if not all(isinstance(x, torch.Tensor) and x.is_cuda for x in rows):
        raise _lib.BuddyHipError(cpu)
    lib = _lib.require_gpu()
    assert all(x.dim() == 2 and x.shape == rows[0].shape and x.dtype == torch.float32 for x in rows), shape
    if rate is not None and (int(fs) != fs or int(fs) < min_fs):
        raise ValueError(rate)
    return lib, [x.contiguous() for x in rows], lengths(lens, *rows[0].shape)


def to_rate(rows, lens_t, fs, target_fs):
    """``rows`` (tensors of one shape at rate ``fs``) and their lengths at ``target_fs`` -> (rows, lengths); the inputs themselves at equal rates"""
    if fs == target_fs:
        return rows, lens_t
    L, dev = rows[0].shape[1], rows[0].device
    if int(lens_t.min()) < L:                    # the resampler takes whole rows: zero behind each row's end (zero extension is what it assumes there)
        live = torch.arange(L, device=dev)[None, :] < lens_t.to(dev)[:, None]
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        rows = [torch.where(live, x, zero) for x in rows]
    up, down = _rs.ratio(fs, target_fs)
    return [_rs.resample(x, fs, target_fs) for x in rows], torch.tensor([_rs.out_length(int(n), up, down) for n in lens_t], dtype=torch.int32)


def pair_gain(mom):
    """the estimate scaled to the clean signal's energy: sqrt(||x||^2 / ||e||^2) from the (B, 4) moments of ``buddy_pair_moments``, 1 for a silent estimate"""
    ee, xx = mom[:, 0], mom[:, 1]
    return torch.where(ee > 0, torch.sqrt(xx / ee), torch.ones_like(ee)).contiguous()
