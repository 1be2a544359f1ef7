"""float64 restatement of multichannel WPE for the tests of ``buddy_wpe_mc`` (not the reference of the comparison: that is
``oracle/wpe_ref.py``).  Its purpose is to state how well-posed a test input is: the same iterations are run with two float64 solvers of
G = R^{-1} P, numpy's LU (``numpy.linalg.solve``) and a Cholesky factorisation, and the distance between the two results is the error any
float64 implementation may show on that input.  The tap order is the oracle's (oldest frame first)."""
import numpy as np

from oracle import wpe_ref


def mc_input(u, L, D):
    """(D, L) float32: channel ch of item u is the clean signal u through its own synthetic response (the recipe of tests/test_hip_wpe.py)"""
    from buddy_amd.synth import synth_clean, synth_rir
    c = synth_clean(u, L).astype(np.float64)
    c = 0.05 * c / c.std()
    return np.stack([np.convolve(c, synth_rir(100 * u + ch, min(8000, L // 2)).astype(np.float64))[:L].astype(np.float32) for ch in range(D)])


def spectrum(y):
    """(D, L) -> (F, D, T) complex128 with the oracle's STFT"""
    return np.ascontiguousarray(wpe_ref.stft(np.asarray(y)).transpose(2, 0, 1))


def signal(X, L):
    """(F, D, T) -> (D, L) float64 with the oracle's iSTFT"""
    return wpe_ref.istft(X.transpose(1, 2, 0))[..., :L]


def _solve(R, P, solver):
    if solver == "lu":
        return np.linalg.solve(R, P)
    Lc = np.linalg.cholesky(R)
    return np.linalg.solve(Lc.conj().T, np.linalg.solve(Lc, P))


def wpe(Y, taps=10, delay=3, iterations=3, solver="lu"):
    """(F, D, T) -> (F, D, T), a bin at a time"""
    out = np.empty_like(Y)
    for f in range(Y.shape[0]):
        Yf = Y[f]
        D, T = Yf.shape
        Yt = np.zeros((taps * D, T), Yf.dtype)
        for k in range(taps):
            s = delay + taps - 1 - k
            if s < T:
                Yt[k * D:(k + 1) * D, s:] = Yf[:, :T - s]
        X = Yf.copy()
        for _ in range(iterations):
            power = np.mean(X.real ** 2 + X.imag ** 2, axis=0)
            Yti = Yt / np.maximum(power, 1e-10 * power.max())
            G = _solve(Yti @ Yt.conj().T, Yti @ Yf.conj().T, solver)
            X = Yf - G.conj().T @ Yt
        out[f] = X
    return out


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))
