"""numpy fp64 oracle of the consistency correction of srmi.superres.RegionSuperResolver.

D and U are F.interpolate(align_corners=False) at 1 / s and at s, written out from the
ATen formulas (UpSample.h) as one matrix per axis; ``residual`` / ``iterate`` / ``apply``
are the three device steps in LR space; ``backproject_hr`` is the literal loop
x <- x + U(M (lr - D x)) at HR size they must reproduce; ``du_dense`` is D U as a dense
matrix and ``spectral_radius`` that of M E M, E = I - D U, on a 2-D field.

Modes are 'bilinear' / 'bicubic'.  Arrays are [..., H, W]; the resampling acts on the last
two axes.  Non-finite values: D is NaN exactly where one of its taps is not finite.
"""
import numpy as np

A = -0.75


def cubic_weights(t):
    """ATen's cubic convolution coefficients (A = -0.75) at fraction t: the weights of
    i0 - 1 .. i0 + 2."""
    def c1(x):
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def c2(x):
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return np.array([c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)])


def interp_matrix(n_in: int, n_out: int, ratio: float, mode: str) -> np.ndarray:
    """[n_out, n_in]: F.interpolate along one axis; ratio = 1 / scale_factor.  Source
    coordinate ratio (d + 0.5) - 0.5; bilinear clamps it at 0, i0 = min(floor, n - 1),
    lambda = clip(src - i0, 0, 1) on i0 and min(i0 + 1, n - 1); bicubic reads i0 - 1 ..
    i0 + 2 clamped to the edge with the cubic weights of src - floor(src)."""
    m = np.zeros((n_out, n_in))
    for d in range(n_out):
        src = ratio * (d + 0.5) - 0.5
        if mode == "bilinear":
            src = max(src, 0.0)
            i0 = min(int(np.floor(src)), n_in - 1)
            lam = min(max(src - i0, 0.0), 1.0)
            m[d, i0] += 1.0 - lam
            m[d, min(i0 + 1, n_in - 1)] += lam
        elif mode == "bicubic":
            i0 = int(np.floor(src))
            for k, c in enumerate(cubic_weights(src - i0)):
                m[d, min(max(i0 - 1 + k, 0), n_in - 1)] += c
        else:
            raise ValueError(mode)
    return m


def _sep(x, my, mx):
    """my x mx^T over the last two axes; NaN exactly where a non-zero tap meets a
    non-finite value."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    y = my @ np.where(fin, x, 0.0) @ mx.T
    hit = (my != 0).astype(np.float64) @ (~fin).astype(np.float64) @ (mx != 0).astype(np.float64).T
    return np.where(hit > 0, np.nan, y)


def D(x, s: int, mode: str):
    H, W = x.shape[-2:]
    return _sep(x, interp_matrix(H, H // s, float(s), mode), interp_matrix(W, W // s, float(s), mode))


def U(r, s: int, mode: str):
    h, w = r.shape[-2:]
    return _sep(r, interp_matrix(h, h * s, 1.0 / s, mode), interp_matrix(w, w * s, 1.0 / s, mode))


def abs_D(x, s: int, mode: str):
    """sum |weight| |value| over D's taps (for error bars); x finite."""
    H, W = x.shape[-2:]
    return np.abs(interp_matrix(H, H // s, float(s), mode)) @ np.abs(x) @ np.abs(
        interp_matrix(W, W // s, float(s), mode)).T


def abs_U(r, s: int, mode: str):
    h, w = r.shape[-2:]
    return np.abs(interp_matrix(h, h * s, 1.0 / s, mode)) @ np.abs(r) @ np.abs(
        interp_matrix(w, w * s, 1.0 / s, mode)).T


# ------------------------------------------------------------ the LR-space form
def residual(x, lr, s: int, dmode: str):
    """(r0, active): active = lr finite and every tap of D in x finite; r0 = lr - D x there,
    0 elsewhere."""
    lr = np.asarray(lr, dtype=np.float64)
    d = D(x, s, dmode)
    active = np.isfinite(lr) & np.isfinite(d)
    return np.where(active, np.where(active, lr, 0.0) - np.where(active, d, 0.0), 0.0), active


def du_coeffs(s: int, umode: str, dmode: str) -> np.ndarray:
    """g[-2 .. 2] of D U along one axis: over the taps j of D (the HR phases p_j of a block)
    k_j times U's weight of the LR offset at that phase."""
    g = np.zeros(5)
    if dmode == "bicubic":
        taps = [(s // 2 - 2 + j, k) for j, k in enumerate(cubic_weights(0.5))]
    else:
        taps = [(s // 2 - 1, 0.5), (s // 2, 0.5)]
    for p, k in taps:
        src = (p + 0.5) / s - 0.5
        i0 = int(np.floor(src))
        t = src - i0
        if umode == "bicubic":
            for q, c in enumerate(cubic_weights(t)):
                g[i0 - 1 + q + 2] += k * c
        else:
            g[i0 + 2] += k * (1.0 - t)
            g[i0 + 3] += k * t
    return g


def du_stencil_matrix(n: int, g) -> np.ndarray:
    """[n, n]: the clamped-index form of g -- row d reads clamp(d + o), o = -2 .. 2."""
    m = np.zeros((n, n))
    for d in range(n):
        for o in range(-2, 3):
            m[d, min(max(d + o, 0), n - 1)] += g[o + 2]
    return m


def du_dense(n: int, s: int, umode: str, dmode: str) -> np.ndarray:
    """[n, n]: D U along one axis of n LR samples, as the product of the two matrices."""
    return interp_matrix(n * s, n, float(s), dmode) @ interp_matrix(n, n * s, 1.0 / s, umode)


def iterate(r, active, s: int, umode: str, dmode: str):
    """r <- M (r - (D U) r) on [..., h, w]."""
    h, w = r.shape[-2:]
    g = du_coeffs(s, umode, dmode)
    return np.where(active, r - du_stencil_matrix(h, g) @ r @ du_stencil_matrix(w, g).T, 0.0)


def abs_iterate(r, s: int, umode: str, dmode: str):
    """|r| + sum |g g| |r| over the stencil's taps (for error bars)."""
    h, w = r.shape[-2:]
    g = np.abs(du_coeffs(s, umode, dmode))
    return np.abs(r) + du_stencil_matrix(h, g) @ np.abs(r) @ du_stencil_matrix(w, g).T


def accumulate(r0, active, s: int, umode: str, dmode: str, K: int):
    """(R_K, r_K): R_K = sum_{k < K} r_k, r_{k+1} = M E r_k."""
    R, r = np.zeros_like(r0), r0
    for _ in range(K):
        R = R + r
        r = iterate(r, active, s, umode, dmode)
    return R, r


def apply(x, R, s: int, umode: str):
    """x + U(R) at the finite pixels of x, x itself elsewhere."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    return np.where(fin, np.where(fin, x, 0.0) + U(R, s, umode), x)


def correct(x, lr, s: int, umode: str, dmode: str, K: int):
    """The whole correction in LR space: (x_K, r0, r_K, active)."""
    r0, active = residual(x, lr, s, dmode)
    R, rK = accumulate(r0, active, s, umode, dmode, K)
    return apply(x, R, s, umode), r0, rK, active


# ------------------------------------------------------------ the literal loop
def backproject_hr(x, lr, s: int, umode: str, dmode: str, K: int):
    """K steps of x <- x + U(M (lr - D x)) at HR size, M the active mask of the FIRST
    iterate (the finite set of x never changes); returns (x_K, M (lr - D x_K))."""
    x = np.asarray(x, dtype=np.float64)
    _, active = residual(x, lr, s, dmode)
    for _ in range(K):
        r, _ = residual(x, lr, s, dmode)
        x = apply(x, np.where(active, r, 0.0), s, umode)
    r, _ = residual(x, lr, s, dmode)
    return x, np.where(active, r, 0.0)


# ------------------------------------------------------------ contraction
def mem_matrix(active2d, s: int, umode: str, dmode: str) -> np.ndarray:
    """M E M on a 2-D LR field [h, w] as a dense [h w, h w] matrix (row-major cells)."""
    active2d = np.asarray(active2d, dtype=bool)
    h, w = active2d.shape
    g = du_coeffs(s, umode, dmode)
    E = np.eye(h * w) - np.kron(du_stencil_matrix(h, g), du_stencil_matrix(w, g))
    m = active2d.reshape(-1).astype(np.float64)
    return m[:, None] * E * m[None, :]


def spectral_radius(active2d, s: int, umode: str, dmode: str) -> float:
    return float(np.max(np.abs(np.linalg.eigvals(mem_matrix(active2d, s, umode, dmode)))))
