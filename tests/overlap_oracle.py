"""numpy restatement of the overlapped tiling plan, its cut and its feathered blend
(srmi_region_to_tiles_overlap, srmi_tiles_blend, srmi.superres).  The reference has no
counterpart (get_tiles cuts a disjoint floor grid, assemble_images concatenates it), so
this oracle is the definition written the slow, obvious way: explicit origins, scatter
of weighted tiles into a sum and a weight image, one division.  Everything is computed
in the dtype it is given (the tests hand in float64)."""
import numpy as np

LNORM, LSCALE, AFFINE = 0, 1, 2  # SRMI_NORM_*


def origins(L: int, t: int, S: int) -> np.ndarray:
    """min(i S, L - t) for i < n = ceil((L - t) / S) + 1."""
    if not 1 <= S <= t <= L:
        raise ValueError((L, t, S))
    n = int(np.ceil((L - t) / S)) + 1
    return np.minimum(np.arange(n) * S, L - t)


def weights(t: int, S: int) -> np.ndarray:
    """w(p) = min(p + 1, t - p, R + 1), R = t - S, as integers."""
    p = np.arange(t)
    return np.minimum(np.minimum(p + 1, t - p), t - S + 1)


def cut(region: np.ndarray, ty: int, tx: int, sy: int, sx: int, mode: int, off=None, div=None):
    """region [C, H, W] -> (tiles [n, C, ty, tx] normalised by mode, off [n, C],
    div [n, C], bad [n]); tile iy * nx + ix at (origins_y[iy], origins_x[ix])."""
    C, H, W = region.shape
    oy, ox = origins(H, ty, sy), origins(W, tx, sx)
    n = len(oy) * len(ox)
    tiles = np.empty((n, C, ty, tx), region.dtype)
    o = np.empty((n, C), region.dtype)
    d = np.empty((n, C), region.dtype)
    bad = np.zeros(n, np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for iy, y0 in enumerate(oy):
            for ix, x0 in enumerate(ox):
                k = iy * len(ox) + ix
                raw = region[:, y0:y0 + ty, x0:x0 + tx]
                bad[k] = not np.isfinite(raw).all()
                if mode == LNORM:
                    o[k], d[k] = raw.mean(axis=(1, 2)), raw.std(axis=(1, 2))
                elif mode == LSCALE:
                    o[k] = raw.min(axis=(1, 2))
                    d[k] = raw.max(axis=(1, 2)) - o[k]
                else:
                    o[k], d[k] = off[k], div[k]
                tiles[k] = (raw - o[k][:, None, None]) / d[k][:, None, None]
    return tiles, o, d, bad


def blend(tiles: np.ndarray, off, div, bad, Sy: int, Sx: int, Ho: int, Wo: int):
    """tiles [n, C, Ty, Tx] -> (out [C, Ho, Wo], M [C, Ho, Wo]): out = sum w v / sum w
    over the non-bad covering tiles, v = x * div + off (off None: x), NaN where none is
    left; M = the largest |x * div| + |off| among them (the scale of the device's
    rounding-error bound), 0 where none."""
    n, C, Ty, Tx = tiles.shape
    oy, ox = origins(Ho, Ty, Sy), origins(Wo, Tx, Sx)
    assert n == len(oy) * len(ox)
    w2 = np.outer(weights(Ty, Sy), weights(Tx, Sx)).astype(tiles.dtype)
    num = np.zeros((C, Ho, Wo), tiles.dtype)
    den = np.zeros((Ho, Wo), tiles.dtype)
    M = np.zeros((C, Ho, Wo), tiles.dtype)
    for iy, y0 in enumerate(oy):
        for ix, x0 in enumerate(ox):
            k = iy * len(ox) + ix
            if bad is not None and bad[k]:
                continue
            x = tiles[k]
            if off is not None:
                sd, m = div[k][:, None, None], off[k][:, None, None]
                v, mag = x * sd + m, np.abs(x * sd) + np.abs(m)
            else:
                v, mag = x, np.abs(x)
            num[:, y0:y0 + Ty, x0:x0 + Tx] += w2 * v
            den[y0:y0 + Ty, x0:x0 + Tx] += w2
            M[:, y0:y0 + Ty, x0:x0 + Tx] = np.maximum(M[:, y0:y0 + Ty, x0:x0 + Tx], mag)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(den > 0, num / den, np.nan)
    return out, M


def cover_count(L: int, t: int, S: int) -> np.ndarray:
    """How many tiles of the axis plan cover each pixel."""
    c = np.zeros(L, np.int64)
    for o in origins(L, t, S):
        c[o:o + t] += 1
    return c
