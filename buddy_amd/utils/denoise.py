"""Noise power tracker and spectral post-filter of noisy recordings, as defined in DESIGN.md section 27: the speech-presence-probability tracker of
Gerkmann & Hendriks (2012) per bin with a decision-directed Wiener or log-spectral-amplitude gain (Ephraim & Malah 1984, 1985), on frames of 512
samples at hop 128 that overhang both ends of the row, so that every sample lies in exactly four frames.

Everything runs on the GPU through ``csrc/denoise.hip`` and has no CPU form: a CPU tensor raises ``BuddyHipError``, a bad argument ``ValueError``.
``denoise`` is the whole call; ``spectra_hip``, ``gains_hip`` and ``synthesis_hip`` are its stages (the unit tests take them one by one).
``report_rows`` / ``write_report`` make the ``denoise.csv`` of the tester and of ``tools/denoise.py`` in the conventions of utils/report.py."""
import numpy as np
import torch

from .. import _lib
from . import _rows, report
from .report import write_report  # noqa: F401  -- the CSV conventions of every report: NaN as an empty field, repr(float)

N, HOP, PAD, BINS = 512, 128, 384, 257
GAINS = ("wiener", "lsa")                            # the gain rules, in the order of the C entry's ``rule``
FLOOR_DB = -15.0                                     # the gain floor: a choice, not a measurement
ROW_FLOOR = 1e-10                                    # phi = ROW_FLOOR * N * mean(x^2), the lower bound of every noise power: a choice
ZERO, SHORT, NO_SPEECH = 1, 2, 4                     # flag bits: the row is all zeros | no frame lies inside the row (L < 512) | nothing above the noise
_FLAG_NAMES = ((ZERO, "ZERO"), (SHORT, "SHORT"), (NO_SPEECH, "NO_SPEECH"))


def frames(L):
    """frames of a row of L >= 1 samples: frame t covers samples t * 128 - 384 .. t * 128 + 127, zeros outside the row"""
    L = int(L)
    if L < 1:
        raise ValueError(f"denoise.frames: L must be >= 1, got {L}")
    return (L - 1 + PAD) // HOP + 1


def flag_text(flags):
    return "|".join(name for bit, name in _FLAG_NAMES if int(flags) & bit)


def _rule(gain, floor_db):
    if gain not in GAINS:
        raise ValueError(f"denoise: gain is one of {list(GAINS)}, got {gain!r}")
    floor_db = float(floor_db)
    if not -120.0 <= floor_db <= 0.0:
        raise ValueError(f"denoise: floor_db must be in [-120, 0] dB, got {floor_db}")
    return GAINS.index(gain), 10.0 ** (floor_db / 20.0)


def _frames_of(lens_t):
    return torch.tensor([frames(int(n)) for n in lens_t], dtype=torch.int32)


def _enter(name, x, lens):
    if isinstance(x, torch.Tensor) and not x.is_cuda:
        raise _lib.BuddyHipError(f"denoise.{name}: runs on the MI355X only (got a CPU tensor)")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"denoise.{name}: takes a (B, L) float32 tensor")
    if lens is not None:
        ln = torch.as_tensor(lens).reshape(-1)
        if ln.numel() != x.shape[0] or int(ln.min()) < 1 or int(ln.max()) > x.shape[1]:
            raise ValueError(f"denoise.{name}: lens holds one length in 1..L per row")
    lib, (x,), lens_t = _rows.enter((x,), lens, "", "")
    return lib, x, lens_t


def _spectrum_args(name, Y, lens_t):
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in Y):
        raise _lib.BuddyHipError(f"denoise.{name}: runs on the MI355X only (got a CPU tensor)")
    if Y[0].dim() != 4 or tuple(Y[0].shape[2:]) != (BINS, 2) or Y[0].dtype != torch.float32:
        raise ValueError(f"denoise.{name}: Y is (B, frames, 257, 2) float32")
    B, ldt = Y[0].shape[0], Y[0].shape[1]
    if lens_t.numel() != B or int(_frames_of(lens_t).max()) > ldt:
        raise ValueError(f"denoise.{name}: Y holds fewer frames than the longest row has")
    return B, ldt


def spectra_hip(x, lens=None):
    """x (B, L) float32 on the GPU, ``lens`` (B ints, default L) -> Y (B, frames(longest), 257, 2) float32, (re, im) of every frame's bins; the
    frames behind a shorter row's own count are left unwritten"""
    lib, x, lens_t = _enter("spectra_hip", x, lens)
    B, L = x.shape
    ldt = int(_frames_of(lens_t).max())
    Y = torch.zeros(B, ldt, BINS, 2, dtype=torch.float32, device=x.device)
    lens_d = lens_t.to(x.device)                     # named: the device copy must outlive the call
    _lib.check(lib.buddy_denoise_spectra(_lib.ptr(x), lens_d.data_ptr(), B, L, _lib.ptr(Y), ldt, _lib.stream_ptr()))
    return Y


def gains_hip(Y, lens, phi, gain="lsa", floor_db=FLOOR_DB):
    """Y from ``spectra_hip``, ``lens`` (B ints), ``phi`` (B,) float64 row floors (0: an all-zero row) -> (G, sigma2), each (B, frames, 257) float32"""
    rule, g_min = _rule(gain, floor_db)
    lens_t = torch.as_tensor(lens, dtype=torch.int32).reshape(-1).cpu()
    B, ldt = _spectrum_args("gains_hip", (Y,), lens_t)
    lib = _lib.require_gpu()
    ph = torch.as_tensor(phi, dtype=torch.float64).reshape(-1)
    if ph.numel() != B or not bool(torch.isfinite(ph).all()) or float(ph.min()) < 0.0:
        raise ValueError("denoise.gains_hip: phi holds one finite value >= 0 per row")
    Y = Y.contiguous()
    G, S = (torch.zeros(B, ldt, BINS, dtype=torch.float32, device=Y.device) for _ in range(2))
    lens_d, ph_d = lens_t.to(Y.device), ph.to(Y.device)
    _lib.check(lib.buddy_denoise_gains(_lib.ptr(Y), lens_d.data_ptr(), ph_d.data_ptr(), B, ldt, rule, g_min, _lib.ptr(G), _lib.ptr(S), _lib.stream_ptr()))
    return G, S


def synthesis_hip(Y, G, lens, L=None):
    """Y, G as above -> (B, L) float32 (L: default the longest row): sum_t w x^_t / sum_t w^2 over the four frames of every sample, zeros behind a
    row's end"""
    lens_t = torch.as_tensor(lens, dtype=torch.int32).reshape(-1).cpu()
    B, ldt = _spectrum_args("synthesis_hip", (Y, G), lens_t)
    if G.dtype != torch.float32 or tuple(G.shape) != (B, ldt, BINS):
        raise ValueError("denoise.synthesis_hip: G is (B, frames, 257) float32, the frames of Y")
    lib = _lib.require_gpu()
    L = int(lens_t.max()) if L is None else int(L)
    if L < int(lens_t.max()):
        raise ValueError("denoise.synthesis_hip: L is below the longest row")
    Y, G = Y.contiguous(), G.contiguous()
    out = torch.zeros(B, L, dtype=torch.float32, device=Y.device)
    nbytes = int(lib.buddy_denoise_synthesis_workspace(B, ldt))
    if nbytes < 0:
        raise ValueError(f"denoise.synthesis_hip: {B} rows of {ldt} frames are more than one call takes")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=Y.device)
    lens_d = lens_t.to(Y.device)
    _lib.check(lib.buddy_denoise_synthesis(_lib.ptr(Y), _lib.ptr(G), lens_d.data_ptr(), B, ldt, _lib.ptr(out), L, ws.data_ptr(), nbytes, _lib.stream_ptr()))
    return out


def row_floor(x, lens_t):
    """phi (B,) float64 on the CPU: ROW_FLOOR * N * mean(x^2) per row, the sum in double in the fixed order of ``buddy_row_moments``.  ``x`` must be
    zero behind each row's end: the zeros add nothing, so a row's floor does not depend on the stride it lies in"""
    mom = torch.empty(x.shape[0], 2, dtype=torch.float64, device=x.device)
    _lib.check(_lib.require_gpu().buddy_row_moments(_lib.ptr(x), _lib.ptr(mom), x.shape[0], x.shape[1], _lib.stream_ptr()))
    return ROW_FLOOR * N * mom[:, 1].cpu() / lens_t.double()


class Denoised:
    """result of ``denoise``: ``out`` (B, L) float32 on the GPU, zeros behind a row's end; on the CPU ``snr_est_db``, ``noise_db``, ``att_db`` (B,)
    float64 -- the estimated SNR 10 log10(sum max(|Y|^2 - sigma^2, 0) / sum sigma^2), the noise level 10 log10(mean sigma^2 / sum w^2) re full scale
    and the attenuation 10 log10(sum x^2 / sum out^2); NaN for an all-zero row --, ``flags`` (B,) int32 (ZERO | SHORT | NO_SPEECH), ``frames`` and
    ``samples`` (B,) int32, ``gain`` and ``floor_db`` as asked for; ``G`` and ``sigma2`` (B, frames, 257) float32 on the GPU where asked for, else None"""

    def __init__(self, out, snr_est_db, noise_db, att_db, flags, frames, samples, gain, floor_db, G=None, sigma2=None):
        self.out, self.snr_est_db, self.noise_db, self.att_db, self.flags, self.frames, self.samples = out, snr_est_db, noise_db, att_db, flags, frames, samples
        self.gain, self.floor_db, self.G, self.sigma2 = gain, floor_db, G, sigma2


def denoise(x, lens=None, gain="lsa", floor_db=FLOOR_DB, keep_gains=False):
    """x (B, L) float32 on the GPU, ``lens`` (B ints, default L): valid samples per row -> ``Denoised``.  ``gain``: ``lsa`` or ``wiener``;
    ``floor_db``: the lowest gain in dB (a choice; -15 by default); ``keep_gains``: keep G and sigma^2.  A row's bits do not depend on its batch."""
    _rule(gain, floor_db)
    lib, x, lens_t = _enter("denoise", x, lens)
    B, L = x.shape
    dev = x.device
    if int(lens_t.min()) < L:                        # zeros behind each row's end, for the row floor
        x = torch.where(torch.arange(L, device=dev)[None, :] < lens_t.to(dev)[:, None], x, torch.zeros((), dtype=torch.float32, device=dev))
    Y = spectra_hip(x, lens_t)
    G, S = gains_hip(Y, lens_t, row_floor(x, lens_t), gain, floor_db)
    out = synthesis_hip(Y, G, lens_t, L)
    st = torch.empty(B, 4, dtype=torch.float64, device=dev)
    lens_d = lens_t.to(dev)
    _lib.check(lib.buddy_denoise_stats(_lib.ptr(x), _lib.ptr(out), lens_d.data_ptr(), B, L, _lib.ptr(Y), _lib.ptr(S), Y.shape[1], st.data_ptr(), _lib.stream_ptr()))
    st = st.cpu()
    return Denoised(out, st[:, 0].clone(), st[:, 1].clone(), st[:, 2].clone(), st[:, 3].to(torch.int32), _frames_of(lens_t), lens_t.clone(), gain, float(floor_db),
                    G if keep_gains else None, S if keep_gains else None)


# ---- the CSV report ------------------------------------------------------------------------------------------------------------------------
def report_rows(names, res):
    """one dict per file from a ``Denoised``: the samples and frames, the three statistics in dB, the flags as text, and the rule they were made with"""
    return [{"file": name, "samples": int(res.samples[b]), "frames": int(res.frames[b]), "snr_est_db": float(res.snr_est_db[b]),
             "noise_db": float(res.noise_db[b]), "att_db": float(res.att_db[b]), "flags": flag_text(res.flags[b]), "gain": res.gain, "floor_db": res.floor_db}
            for b, name in enumerate(names)]


def _finite(v):
    return v if np.isfinite(v) else float("nan")


def summary_rows(rows):
    """n, mean, median and standard deviation (numpy's, population form) of the three statistics over the rows where they are finite"""
    return report.summarise(rows, {col: (lambda r, col=col: _finite(r[col])) for col in ("snr_est_db", "noise_db", "att_db")})


def format_summary(summary):
    """the summary as lines of text (what the tool prints)"""
    return report.format_summary(summary, 12, 4)
