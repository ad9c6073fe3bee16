"""numpy restatement of the spectral score (srmi_spectra, srmi.spectra.SpectralScore).  The
reference has no counterpart, so this oracle is the definition written the obvious way:
explicit windows, one 2-D DFT per field, every bin binned by its own shell number.

``dtype='float64'`` is the definition.  ``dtype='complex64'`` runs the two transforms of
every window in single precision through scipy.fft (everything before and after them
stays fp64): the fp32 reference arithmetic from which the device tests take their bars.
"""
import numpy as np
import scipy.fft

QUANTITIES = ("power_pred", "power_truth", "power_error", "cross")


def origins(L: int, P: int, Q: int) -> np.ndarray:
    """min(i Q, L - P) for i < n = ceil((L - P) / Q) + 1 (the overlap plan)."""
    if not 1 <= Q <= P <= L:
        raise ValueError((L, P, Q))
    n = -((P - L) // Q) + 1
    return np.minimum(np.arange(n) * Q, L - P)


def check_window(P: int, H: int, W: int, Q: int) -> None:
    if P < 16 or P > 256 or P & (P - 1) or P > min(H, W) or not 1 <= Q <= P:
        raise ValueError(f"window {P} stride {Q} on a field {(H, W)}")


def hann(P: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(P) / P)


def shells(P: int) -> np.ndarray:
    """[P, P] shell number of every DFT bin (index order of the transform)."""
    k = np.fft.fftfreq(P, 1.0 / P)  # signed integers in [-P/2, P/2)
    return np.floor(np.sqrt(k[:, None] ** 2 + k[None, :] ** 2) + 0.5).astype(np.int64)


def tapered(win: np.ndarray) -> np.ndarray:
    """One window plane [P, P] fp32 -> detrended (fp64 mean and subtraction, rounded to
    fp32) and tapered, fp64."""
    P = win.shape[0]
    w64 = win.astype(np.float64)
    d32 = (w64 - w64.mean()).astype(np.float32)
    h = hann(P)
    return d32.astype(np.float64) * (h[:, None] * h[None, :])


def densities(a_win: np.ndarray, b_win: np.ndarray, dtype: str = "float64") -> np.ndarray:
    """[4, P, P]: Eaa, Ebb, Eee, Cab of every bin of one window plane."""
    P = a_win.shape[0]
    ta, tb = tapered(a_win), tapered(b_win)
    if dtype == "complex64":
        Fa = scipy.fft.fft2(ta.astype(np.complex64)).astype(np.complex128)
        Fb = scipy.fft.fft2(tb.astype(np.complex64)).astype(np.complex128)
    elif dtype == "float64":
        Fa, Fb = np.fft.fft2(ta), np.fft.fft2(tb)
    else:
        raise ValueError(dtype)
    h = hann(P)
    W2 = ((h[:, None] * h[None, :]) ** 2).sum()
    n = P * P * W2
    return np.stack([np.abs(Fa) ** 2, np.abs(Fb) ** 2, np.abs(Fa - Fb) ** 2, (Fa * np.conj(Fb)).real]) / n


def shell_sums(dens: np.ndarray) -> np.ndarray:
    """[4, P, P] -> [4, K]: sums over shells 0 .. P/2, the corners dropped."""
    P = dens.shape[-1]
    K = P // 2 + 1
    j = shells(P).ravel()
    keep = j < K
    return np.stack([np.bincount(j[keep], weights=d.ravel()[keep], minlength=K) for d in dens])


def skipped(a: np.ndarray, b: np.ndarray, P: int, Q: int) -> np.ndarray:
    """[ny * nx] bool, row-major: the window holds a non-finite pixel of a or b in any channel."""
    _, H, W = a.shape
    bad = ~(np.isfinite(a).all(axis=0) & np.isfinite(b).all(axis=0))
    return np.array([bad[y0:y0 + P, x0:x0 + P].any() for y0 in origins(H, P, Q) for x0 in origins(W, P, Q)])


def spectra(a: np.ndarray, b: np.ndarray, P: int, Q: int, dtype: str = "float64"):
    """a, b [C, H, W] fp32 -> (out [C, 4, K] fp64, nused): the shell sums averaged over the
    used windows; NaN everywhere when none is used."""
    C, H, W = a.shape
    check_window(P, H, W, Q)
    K = P // 2 + 1
    skip = skipped(a, b, P, Q)
    wins = [(y0, x0) for y0 in origins(H, P, Q) for x0 in origins(W, P, Q)]
    out = np.zeros((C, 4, K))
    nused = int((~skip).sum())
    for (y0, x0), s in zip(wins, skip):
        if s:
            continue
        for c in range(C):
            out[c] += shell_sums(densities(a[c, y0:y0 + P, x0:x0 + P], b[c, y0:y0 + P, x0:x0 + P], dtype))
    if nused == 0:
        return np.full((C, 4, K), np.nan), 0
    return out / nused, nused


def derived(out: np.ndarray):
    """error_ratio, power_ratio, coherence [C, K] of out [C, 4, K]."""
    with np.errstate(invalid="ignore", divide="ignore"):
        Eaa, Ebb, Eee, Cab = out[:, 0], out[:, 1], out[:, 2], out[:, 3]
        return Eee / Ebb, Eaa / Ebb, Cab * Cab / (Eaa * Ebb)


def red_field(n: int, slope: float, seed: int) -> np.ndarray:
    """[n, n] fp64 noise with amplitude spectrum k^-slope (k the radial wavenumber, the
    mean removed), normalised to unit standard deviation."""
    rng = np.random.default_rng(seed)
    F = np.fft.fft2(rng.standard_normal((n, n)))
    k = np.fft.fftfreq(n, 1.0 / n)
    kr = np.sqrt(k[:, None] ** 2 + k[None, :] ** 2)
    kr[0, 0] = 1.0
    F *= kr ** (-slope)
    F[0, 0] = 0.0
    f = np.fft.ifft2(F).real
    return f / f.std()
