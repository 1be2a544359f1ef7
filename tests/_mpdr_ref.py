"""float64 numpy restatement of the wMPDR beamformer after multichannel WPE, a bin at a time: the reference of the
tests of ``buddy_mpdr`` / ``buddy_wpe_mc_mpdr_dereverb``.  ``solver`` chooses how u = R^-1 v is computed (numpy's LU or a Cholesky
factorisation; the distance between the two states how well-posed an input is), ``steering`` how the principal eigenvector of
Phi = sum_t x x^H is found (the ten normalised squarings the kernel does, or ``numpy.linalg.eigh``)."""
import numpy as np

from oracle import wpe_ref

SQUARINGS = 10


def steering_vector(X, reference, steering="squaring"):
    """X (D, T) -> the relative transfer function to channel ``reference`` (D,), or None for pass-through"""
    Phi = X @ X.conj().T
    if steering == "eigh":
        if not np.abs(Phi).max() > 0:
            return None
        v = np.linalg.eigh((Phi + Phi.conj().T) / 2)[1][:, -1]
    else:
        A = Phi
        for _ in range(SQUARINGS):
            m = np.abs(A).max()
            if m == 0:
                return None
            A = A / m
            A = A @ A
            A = (A + A.conj().T) / 2
        v = A[:, reference]
    vr2, nv = abs(v[reference]) ** 2, float(np.sum(np.abs(v) ** 2))
    if vr2 < 1e-12 * nv or vr2 == 0:
        return None
    return v / v[reference]


def _solve(R, v, solver):
    if solver == "lu":
        return np.linalg.solve(R, v)
    Lc = np.linalg.cholesky(R)                                      # raises LinAlgError on a pivot <= 0
    return np.linalg.solve(Lc.conj().T, np.linalg.solve(Lc, v))


def mpdr_bin(X, reference=0, iterations=2, loading=1e-6, solver="cholesky", steering="squaring"):
    """X (D, T) complex128 -> z (T,)"""
    D, T = X.shape
    if D == 1:
        return X[0].copy()
    v = steering_vector(X, reference, steering)
    if v is None:
        return X[reference].copy()
    p = np.mean(X.real ** 2 + X.imag ** 2, axis=0)
    z = None
    for _ in range(iterations):
        if p.max() == 0:
            return np.zeros(T, X.dtype)
        lam = np.maximum(p, 1e-10 * p.max())
        R = (X / lam) @ X.conj().T
        R = R + loading * np.trace(R).real / D * np.eye(D)
        try:
            if solver == "cholesky" and not np.all(np.isfinite(R)):
                raise np.linalg.LinAlgError
            u = _solve(R, v, solver)
        except np.linalg.LinAlgError:
            return X[reference].copy()
        q = np.vdot(v, u)                                           # v^H u
        if q == 0 or not np.isfinite(q):
            return X[reference].copy()
        w = u / q
        z = w.conj() @ X
        p = z.real ** 2 + z.imag ** 2
    return z


def mpdr(X, reference=0, iterations=2, loading=1e-6, solver="cholesky", steering="squaring"):
    """(F, D, T) complex128 -> (F, T)"""
    return np.stack([mpdr_bin(X[f], reference, iterations, loading, solver, steering) for f in range(X.shape[0])])


def signal(Z, L):
    """(F, T) -> (L,) float64 with the oracle's iSTFT"""
    return wpe_ref.istft(Z.T[None])[0, :L]


def bound(D, loading):
    """what the kernel may differ from the restatement by, relative to the largest output magnitude: cond(R) <= D / loading after loading, one
    backward-stable solve, a factor 64 for the D-term sums and the normalisation"""
    return 64.0 * (D / loading) * 2.0 ** -53


def noisy_array(snr_db, L=16000):
    """the noise-property input: (clean reference-channel signal (L,), array signal (4, L) float64, noise variance).  One source through gains
    (1, 0.9, 1.1, 0.8) and delays (0, 1.3, 2.7, 0.6) samples (FFT phases on 2 L points, cut to L) plus white noise of RandomState(0)"""
    from buddy_amd.synth import synth_clean
    s = synth_clean(0, L).astype(np.float64)
    s = 0.05 * s / s.std()
    gains, delays = (1.0, 0.9, 1.1, 0.8), (0.0, 1.3, 2.7, 0.6)
    S = np.fft.rfft(s, 2 * L)
    k = np.arange(S.shape[0])
    clean = np.stack([g * np.fft.irfft(S * np.exp(-2j * np.pi * k * d / (2 * L)), 2 * L)[:L] for g, d in zip(gains, delays)])
    sigma2 = float(np.var(clean[0])) / 10.0 ** (snr_db / 10.0)
    noise = np.sqrt(sigma2) * np.random.RandomState(0).standard_normal((4, L))
    return clean[0], clean + noise, sigma2


def noise_ratio(z_time, clean0, sigma2):
    """var(beamformed - clean reference channel) / noise variance of one channel"""
    return float(np.var(z_time - clean0) / sigma2)
