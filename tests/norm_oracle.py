"""numpy restatement of the reference's normalisation statistics and of the six
``task.norm`` branches (sres/base/source/swot/raw.py), as oracle/rcan_oracle.py
restates 'lnorm': raw.py itself imports xarray and parse, which are not
available, so nothing is imported from it (the statistics half is pinned by golden
vectors of the reference's own NormData, tests/golden/make_golden_norm.py).  Arrays replace the xarray objects:
a time slice is [ntiles, C, ty, tx] (get_tiles' result, raw.py:230-233), the
statistics are [ntiles, C, 4] in STATS order.  Everything is computed in the
dtype it is given (the tests hand in float64)."""
import numpy as np

STATS = ["mean", "var", "max", "min"]  # raw.py:18


def compute_normalization(timeslices) -> np.ndarray:
    """_compute_normalization (raw.py:89-106) with NormData's bookkeeping (raw.py:46-63)
    as array reductions -> [ntiles, C, 4]: per (tile position, variable) the mean over
    the time slices of the plane's mean and of its variance (ddof 0), the largest of
    its maxima and the smallest of its minima."""
    x = np.stack(timeslices)  # [ntimes, ntiles, C, ty, tx]
    planes = x.reshape(x.shape[:3] + (-1,))
    return np.stack([planes.mean(axis=-1).mean(axis=0), planes.var(axis=-1).mean(axis=0),
                     planes.max(axis=-1).max(axis=0), planes.min(axis=-1).min(axis=0)], axis=-1)


def globalize_norm(tstats: np.ndarray) -> np.ndarray:
    """globalize_norm (raw.py:23-30) per variable: [ntiles, C, 4] -> [C, 4]."""
    res = []
    for i, stat in enumerate(STATS):
        d = tstats[..., i]
        res.append(d.max(axis=0) if stat == "max" else d.min(axis=0) if stat == "min" else d.mean(axis=0))
    return np.stack(res, axis=-1)


def norm(batch: np.ndarray, ntype: str, tile_range=None, tstats: np.ndarray = None):
    """norm (raw.py:169-214) of batch [B, C, ty, tx] -> (normalised batch, attrs with
    [B, C, 1, 1] entries).  tstats [ntiles, C, 4]: norm_stats; the global statistics
    are globalize_norm of it (raw.py:121-123).  'tscale' takes the rows tile_range, as
    'tnorm' does (the reference aligns un-sliced arrays by xarray label; the two agree
    when no tile was dropped)."""
    B, C = batch.shape[:2]
    tr = slice(*(tile_range or (0, B)))
    out, attrs = [], {}
    for c in range(C):
        b = batch[:, c]
        bd = (B, 1, 1, 1)
        if ntype == "lnorm":  # :177-181
            m, s = b.mean(axis=(1, 2)), b.std(axis=(1, 2))
            attrs.setdefault("mean", []).append(m.reshape(bd))
            attrs.setdefault("std", []).append(s.reshape(bd))
            out.append((b - m[:, None, None]) / s[:, None, None])
        elif ntype == "lscale":  # :182-186
            mx, mn = b.max(axis=(1, 2)), b.min(axis=(1, 2))
            attrs.setdefault("max", []).append(mx.reshape(bd))
            attrs.setdefault("min", []).append(mn.reshape(bd))
            out.append((b - mn[:, None, None]) / (mx - mn)[:, None, None])
        elif ntype == "gnorm":  # :187-191
            g = globalize_norm(tstats)[c]
            out.append((b - g[0]) / np.sqrt(g[1]))
        elif ntype == "gscale":  # :192-195
            g = globalize_norm(tstats)[c]
            out.append((b - g[3]) / (g[2] - g[3]))
        elif ntype == "tnorm":  # :196-203
            m, s = tstats[tr, c, 0], np.sqrt(tstats[tr, c, 1])
            attrs.setdefault("mean", []).append(m.reshape(bd))
            attrs.setdefault("std", []).append(s.reshape(bd))
            out.append((b - m.reshape(-1, 1, 1)) / s.reshape(-1, 1, 1))
        elif ntype == "tscale":  # :204-209
            mn, mx = tstats[tr, c, 3], tstats[tr, c, 2]
            attrs.setdefault("max", []).append(mx.reshape(bd))
            attrs.setdefault("min", []).append(mn.reshape(bd))
            out.append((b - mn.reshape(-1, 1, 1)) / (mx - mn).reshape(-1, 1, 1))
        else:
            raise Exception(f"Unknown norm: {ntype}")  # :210
    return np.stack(out, axis=1), {k: np.concatenate(v, axis=1) for k, v in attrs.items()}


def denorm(normed: np.ndarray, attrs) -> np.ndarray:
    """denorm (sres/controller/dual_trainer.py:67-77)."""
    if "mean" in attrs:
        normed = normed * attrs["std"] + attrs["mean"]
    if "max" in attrs:
        normed = normed * (attrs["max"] - attrs["min"]) + attrs["min"]
    return normed
