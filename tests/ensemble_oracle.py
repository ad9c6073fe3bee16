"""numpy restatement of the geometric self-ensemble (srmi_tiles_dihedral,
srmi_tiles_blend_ensemble; srmi.superres with ensemble > 1), built on overlap_oracle.blend.
The reference has no counterpart (it flips training batches only), so, as in
overlap_oracle, this is the definition written the slow, obvious way: every slab is
transformed back as a whole, blended alone, and the mean and the standard deviation
(ddof 0) are taken over the slabs.  Everything is computed in the dtype it is given (the
tests hand in float64).

Variant f is the reference's xyflip (sres/base/source/batch.py:37-49, pinned by
tests/golden/xyflip.npz): flip x if bit 0, flip y if bit 1, then swap the last two axes
if bit 2."""
import numpy as np

import overlap_oracle as oo


def variants_of(mask: int):
    """The variant indices a bit mask 1 .. 255 selects, ascending."""
    if not 1 <= int(mask) <= 255:
        raise ValueError(mask)
    return tuple(f for f in range(8) if mask >> f & 1)


def dihedral(x: np.ndarray, f: int) -> np.ndarray:
    """Variant f of x [..., h, w]."""
    if not 0 <= f <= 7:
        raise ValueError(f)
    if f & 1:
        x = x[..., :, ::-1]
    if f & 2:
        x = x[..., ::-1, :]
    if f & 4:
        x = np.swapaxes(x, -1, -2)
    return np.ascontiguousarray(x)


def undo(x: np.ndarray, f: int) -> np.ndarray:
    """The inverse of dihedral(., f): the steps undone in reverse order."""
    if not 0 <= f <= 7:
        raise ValueError(f)
    if f & 4:
        x = np.swapaxes(x, -1, -2)
    if f & 2:
        x = x[..., ::-1, :]
    if f & 1:
        x = x[..., :, ::-1]
    return np.ascontiguousarray(x)


def expand(x: np.ndarray, mask: int) -> np.ndarray:
    """x [..., h, w] -> [K, ..., h, w]: the selected variants in ascending f."""
    return np.stack([dihedral(x, f) for f in variants_of(mask)])


def blend_ensemble(tiles, variants, off, div, bad, Sy, Sx, Ho, Wo, mask=None, scale=1):
    """tiles [K, n, C, Ty, Tx], slab j in the frame of variant variants[j] (a bit mask is
    taken as variants_of) -> (mean [C, Ho, Wo], spread [C, Ho, Wo], M [C, Ho, Wo]): every
    slab is undone, blended by overlap_oracle.blend (NaN again where mask[c][Y // scale]
    [X // scale] is not finite, when a mask is given), then the mean and the ddof-0 standard
    deviation over j; M is the blend's bound, maximised over j."""
    if isinstance(variants, (int, np.integer)):
        variants = variants_of(int(variants))
    assert len(variants) == tiles.shape[0]
    outs, M = [], None
    for j, f in enumerate(variants):
        o, m = oo.blend(undo(tiles[j], f), off, div, bad, Sy, Sx, Ho, Wo)
        outs.append(o)
        M = m if M is None else np.maximum(M, m)
    outs = np.stack(outs)
    if mask is not None:
        assert Ho % scale == 0 and Wo % scale == 0 and mask.shape[1:] == (Ho // scale, Wo // scale)
        dry = np.repeat(np.repeat(~np.isfinite(mask), scale, axis=1), scale, axis=2)
        outs = np.where(dry[None], np.nan, outs)
    with np.errstate(invalid="ignore"):
        mean = outs.mean(axis=0)
        spread = np.sqrt(((outs - mean[None]) ** 2).mean(axis=0))
    return mean, spread, M
