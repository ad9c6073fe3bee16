"""numpy restatement of the land-aware forms (srmi_region_to_tiles_overlap_masked,
srmi_tiles_blend_masked, srmi_rmse_partial_masked; srmi.superres with land=True).  The
reference has no counterpart: it drops every tile that touches land.  As in
overlap_oracle, this is the definition written the slow, obvious way.

"wet" = finite.  The statistics and the normalisation are computed in the dtype they are
given (the tests hand in float64).  The fill exists twice: as float64, and as the float32
BIT MODEL of the kernel -- per dry pixel plain float32 adds of the already filled
8-neighbours in the fixed order NEIGH, starting from 0, then one float32 multiply by
RECIP[count - 1] -- which the device must reproduce bit for bit."""
import numpy as np

import overlap_oracle as oo

LNORM, LSCALE, AFFINE = oo.LNORM, oo.LSCALE, oo.AFFINE
NEIGH = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
RECIP = (1.0 / np.arange(1, 9)).astype(np.float32)  # 1 / k rounded to fp32
assert all(RECIP[k - 1] == np.float32(1) / np.float32(k) for k in range(1, 9))


def fill(plane: np.ndarray, wet: np.ndarray, dtype=np.float32):
    """plane [ty, tx] (values at ~wet are ignored) -> (filled [ty, tx] of dtype, stamp
    [ty, tx]: 0 = wet, j = filled in pass j, passes).  Pass j gives every pixel not filled
    before it that has a filled 8-neighbour inside the plane the mean of those
    neighbours; passes are simultaneous.  Needs one wet pixel."""
    wet = np.asarray(wet, bool)
    if not wet.any():
        raise ValueError("fill: no wet pixel")
    dtype = np.dtype(dtype).type
    ty, tx = plane.shape
    f = np.where(wet, plane, 0).astype(dtype)
    stamp = np.where(wet, 0, -1).astype(np.int64)
    recip = RECIP if dtype is np.float32 else 1.0 / np.arange(1, 9).astype(dtype)
    j = 0
    while (stamp < 0).any():
        j += 1
        assert j <= max(ty, tx) - 1, "more passes than a plane of this size can need"
        fp = np.zeros((ty + 2, tx + 2), dtype)
        fp[1:-1, 1:-1] = f
        done = np.zeros((ty + 2, tx + 2), bool)
        done[1:-1, 1:-1] = stamp >= 0
        acc = np.zeros((ty, tx), dtype)
        cnt = np.zeros((ty, tx), np.int64)
        for dy, dx in NEIGH:  # the fixed add order
            ok = done[1 + dy:1 + dy + ty, 1 + dx:1 + dx + tx]
            v = fp[1 + dy:1 + dy + ty, 1 + dx:1 + dx + tx]
            with np.errstate(invalid="ignore"):
                acc = np.where(ok, (acc + v).astype(dtype), acc)
            cnt += ok
        take = (stamp < 0) & (cnt > 0)
        with np.errstate(invalid="ignore"):
            mean = (acc * recip[np.maximum(cnt, 1) - 1]).astype(dtype)
        f = np.where(take, mean, f)
        stamp = np.where(take, j, stamp)
    return f, stamp, j


def chebyshev_to_wet(wet: np.ndarray) -> np.ndarray:
    """Per pixel, the Chebyshev distance to the nearest wet pixel (brute force)."""
    ys, xs = np.nonzero(wet)
    yy, xx = np.mgrid[0:wet.shape[0], 0:wet.shape[1]]
    return np.maximum(np.abs(yy[..., None] - ys), np.abs(xx[..., None] - xs)).min(axis=-1)


def cut(region: np.ndarray, ty: int, tx: int, sy: int, sx: int, mode: int, min_wet: int, off=None, div=None):
    """region [C, H, W] with NaN for land -> (norm [n, C, ty, tx]: the wet pixels
    normalised by mode over the wet pixels, NaN at the dry ones (NOT filled; all 0 for a
    bad tile), off [n, C], div [n, C], bad [n], nwet [n, C]).  bad[k] = some channel of
    tile k has nwet < min_wet.  Asserts that no used plane with two or more wet pixels is
    constant (a single wet pixel has zero spread by construction: IEEE NaN in the
    tile-local modes)."""
    assert min_wet >= 1
    C, H, W = region.shape
    oy, ox = oo.origins(H, ty, sy), oo.origins(W, tx, sx)
    n = len(oy) * len(ox)
    norm = np.zeros((n, C, ty, tx), region.dtype)
    o = np.full((n, C), np.nan, region.dtype)
    d = np.full((n, C), np.nan, region.dtype)
    bad = np.zeros(n, np.int32)
    nwet = np.zeros((n, C), np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for iy, y0 in enumerate(oy):
            for ix, x0 in enumerate(ox):
                k = iy * len(ox) + ix
                raw = region[:, y0:y0 + ty, x0:x0 + tx]
                wet = np.isfinite(raw)
                nwet[k] = wet.sum(axis=(1, 2))
                bad[k] = (nwet[k] < min_wet).any()
                for c in range(C):
                    w = raw[c][wet[c]]
                    if mode == AFFINE:
                        o[k, c], d[k, c] = off[k, c], div[k, c]
                    elif w.size:
                        if mode == LNORM:
                            o[k, c] = w.mean()
                            d[k, c] = np.sqrt(((w - o[k, c]) ** 2).mean())
                        else:
                            o[k, c], d[k, c] = w.min(), w.max() - w.min()
                    if bad[k]:
                        continue
                    assert w.size < 2 or w.max() > w.min(), f"constant wet plane: tile {k} channel {c}"
                    norm[k, c] = np.where(wet[c], (raw[c] - o[k, c]) / d[k, c], np.nan)
    return norm, o, d, bad, nwet


def fill_tiles(norm: np.ndarray, wet: np.ndarray, bad: np.ndarray, dtype=np.float32):
    """Every plane of the non-bad tiles filled -> (tiles of dtype, passes [n, C])."""
    out = np.zeros(norm.shape, dtype)
    passes = np.zeros(norm.shape[:2], np.int64)
    for k in range(norm.shape[0]):
        if bad[k]:
            continue
        for c in range(norm.shape[1]):
            out[k, c], _, passes[k, c] = fill(norm[k, c], wet[k, c], dtype)
    return out, passes


def wet_tiles(region: np.ndarray, ty: int, tx: int, sy: int, sx: int) -> np.ndarray:
    """[n, C, ty, tx] bool: the finite pixels of every tile plane."""
    oy, ox = oo.origins(region.shape[1], ty, sy), oo.origins(region.shape[2], tx, sx)
    return np.stack([np.isfinite(region[:, y0:y0 + ty, x0:x0 + tx]) for y0 in oy for x0 in ox])


def dry_hr(mask_src: np.ndarray, scale: int) -> np.ndarray:
    """[C, h, w] -> [C, h scale, w scale] bool: the nearest-neighbour upsampled dry set."""
    return np.repeat(np.repeat(~np.isfinite(mask_src), scale, axis=1), scale, axis=2)


def blend(tiles, off, div, bad, Sy, Sx, Ho, Wo, mask_src, scale):
    """overlap_oracle.blend, then NaN where mask_src[c][Y // scale][X // scale] is not
    finite -> (out, M)."""
    assert Ho % scale == 0 and Wo % scale == 0 and mask_src.shape[1:] == (Ho // scale, Wo // scale)
    out, M = oo.blend(tiles, off, div, bad, Sy, Sx, Ho, Wo)
    return np.where(dry_hr(mask_src, scale), np.nan, out), M


def rmse(pred: np.ndarray, target: np.ndarray):
    """(sqrt(mean (p - t)^2) over the elements where both are finite, their count);
    count 0: NaN."""
    p, t = np.asarray(pred, np.float64).ravel(), np.asarray(target, np.float64).ravel()
    both = np.isfinite(p) & np.isfinite(t)
    count = int(both.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.sqrt(np.float64(((p[both] - t[both]) ** 2).sum()) / count)), count


# ------------------------------------------------------------ the GPU tests' inputs
def coast_region(seed: int = 41, scale: float = 3.0, shift: float = 1.0) -> np.ndarray:
    """The [2, 40, 54] float32 region of the cut and blend tests (tile 16, stride 12: the
    3 x 5 plan with origins y 0 12 24, x 0 12 24 36 38).  Its dry set, in both channels:
    tile (0, 0) reduced to its corner pixel (0, 0), so the fill there takes 15 passes;
    an all-land tile (2, 4) = rows 24.., columns 38..; a staircase coast along the bottom
    crossing tiles (2, 0) .. (2, 2); the isolated dry pixel (20, 30); the land block rows
    2..10, columns 30..40 with the 3 x 3 lake rows 5..7, columns 34..36.  Channel 1 only:
    the dry pixel (20, 45), and columns 36, 37 of rows 24.., which leaves tile (2, 3) with
    32 wet pixels in channel 0 and none in channel 1 -- bad through the other channel."""
    rng = np.random.RandomState(seed)
    r = (rng.randn(2, 40, 54) * scale + shift).astype(np.float32)
    dry = np.zeros((40, 54), bool)
    dry[0:16, 0:16] = True
    dry[0, 0] = False
    dry[24:40, 38:54] = True
    yy, xx = np.mgrid[0:40, 0:54]
    dry |= (xx < 36) & (yy >= 30 + xx // 4)
    dry[20, 30] = True
    dry[2:11, 30:41] = True
    dry[5:8, 34:37] = False
    r[:, dry] = np.nan
    r[1, 20, 45] = np.nan
    r[1, 24:40, 36:38] = np.nan
    return r


def coast_planes():
    """(plane, wet) pairs at the sizes of the fill-accuracy check: the tile planes of
    coast_region that are neither all wet nor all dry, and 48 x 48, 32 x 40 and 17 x 23
    planes of N(0, 1) data with a smooth coast and an island."""
    out = []
    reg = coast_region(scale=1.0, shift=0.0)
    for raw in (reg[:, y0:y0 + 16, x0:x0 + 16] for y0 in oo.origins(40, 16, 12) for x0 in oo.origins(54, 16, 12)):
        for c in range(2):
            wet = np.isfinite(raw[c])
            if wet.any() and not wet.all():
                out.append((raw[c], wet))
    rng = np.random.RandomState(42)
    for ty, tx in ((48, 48), (32, 40), (17, 23)):
        yy, xx = np.mgrid[0:ty, 0:tx]
        wet = xx < 0.55 * tx + 0.2 * tx * np.sin(yy * 7.0 / ty)
        wet[ty // 2 - 1:ty // 2 + 2, tx - 4:tx - 1] = True  # an island of water in the land
        out.append((rng.randn(ty, tx).astype(np.float32), wet))
    return out
