"""Training-batch preparation on the device.

The reference prepares every training batch on the host in xarray:

* ``norm`` with ``task.norm == 'lnorm'`` (sres/base/source/swot/raw.py:169-181):
  per tile and channel ``(x - mean) / std`` over (y, x), ddof 0, the statistics
  kept as ``attrs['mean'] / attrs['std']`` of shape [B, C, 1, 1];
* ``xyflip`` (sres/base/source/batch.py:37-49, called by ``load_batch`` :301):
  when ``task.xyflip`` is set, one ``random.randint(0, 7)`` per batch picks a
  dihedral variant (bit 0 flips x, bit 1 flips y, bit 2 swaps the axes),
  recorded as ``attrs['xyflip']``;
* ``apply_network`` then feeds ``downsample(target)`` (dual_trainer.py:557-571,
  array.py:72-76) to the model.

``prep_batch`` does the three in one HIP kernel (``srmi_batch_prep``, tiles.hip):
one HBM read of the raw tiles, one write of the HR target and of the LR input.
The flip index is drawn on the host exactly as the reference draws it.

The other five ``task.norm`` modes (raw.py:182-209) go through
``srmi_batch_prep_norm`` (``prep_batch(norm=...)``, srmi.norm).
"""
from __future__ import annotations

import random
from typing import Dict, Optional, Tuple

import torch

from ._lib import call, ptr, stream_handle


def xyflip_index(enabled: bool, rng: Optional[random.Random] = None) -> int:
    """The reference's draw (batch.py:38-40): ``random.randint(0, 7)`` if
    ``task.xyflip`` else 0 (module-level ``random``, unseeded, unless ``rng``)."""
    if not enabled:
        return 0
    return (rng or random).randint(0, 7)


def prep_batch(raw: torch.Tensor, flip_index: int = 0, scale: int = 4, with_lr: bool = True,
               hr: Optional[torch.Tensor] = None, lr: Optional[torch.Tensor] = None,
               stream=None, norm: str = "lnorm", stats=None,
               tile_range: Optional[Tuple[int, int]] = None, land: bool = False,
               min_wet: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """raw [B, C, T, T] fp32 device tiles -> {'hr': xyflip(lnorm(raw)), 'lr':
    downsample(hr, scale), 'mean': [B, C, 1, 1], 'std': [B, C, 1, 1],
    'xyflip': flip_index}.  Raises SrmiError on bad shapes (T odd, T % scale,
    flip_index outside 0..7).

    norm: task.norm (srmi.norm.NORM_TYPES; anything else raises the reference's
    ``Exception("Unknown norm: ...")``).  The statistics returned are the ones the
    reference's norm() puts in attrs (raw.py:169-214): 'mean' / 'std' for lnorm and
    tnorm, 'max' / 'min' for lscale and tscale, none for gnorm and gscale.  The
    dataset modes (gnorm, gscale, tnorm, tscale) need ``stats``, a finalised
    srmi.norm.NormStats (ValueError without), and tnorm / tscale the batch's
    ``tile_range`` (start, end) in the time slice, default (0, B); tscale takes its
    rows positionally, as tnorm does (srmi.norm's docstring).

    land=True (no reference counterpart): NaN (any non-finite value) in raw is land.
    One ``srmi_batch_prep_masked``: the statistics over each plane's wet pixels, 'hr'
    NaN on land, 'lr' downsampled from it (NaN iff a tap is dry) and flood-filled, and
    'nwet' [B, C] int32, the wet pixels per plane.  lnorm, lscale, gnorm and gscale;
    tnorm / tscale raise (their statistics rows belong to the tiles of the all-wet keep
    list, the reason srmi.superres refuses them).  lscale returns 'min' and 'max' of the
    wet pixels.  min_wet, a fraction of the tile plane, is checked by whoever selects
    the tiles (srmi.llc.get_tiles, TimesliceFeed); here it is only validated."""
    if land:
        return _prep_batch_land(raw, flip_index, scale, with_lr, hr, lr, stream, norm, stats, min_wet)
    if norm != "lnorm":
        from .norm import DATASET_NORMS, check_norm
        if check_norm(norm) in DATASET_NORMS and stats is None:
            raise ValueError(f"prep_batch: norm {norm!r} needs the dataset statistics (stats=NormStats)")
    if raw.dtype != torch.float32 or raw.dim() != 4 or not raw.is_contiguous():
        raise ValueError("prep_batch: raw must be a contiguous fp32 [B, C, T, T] tensor")
    B, C, T, T2 = raw.shape
    if T != T2:
        raise ValueError("prep_batch: tiles must be square (xyflip swaps the axes)")
    if hr is None:
        hr = torch.empty_like(raw)
    if with_lr and lr is None:
        lr = torch.empty(B, C, T // scale, T // scale, device=raw.device, dtype=torch.float32)
    if norm != "lnorm":
        from .norm import prep_norm
        out = {"hr": hr, "xyflip": int(flip_index)}
        out.update(prep_norm(raw, norm, flip_index, scale, hr, lr if with_lr else None, stats, tile_range, stream))
        if with_lr:
            out["lr"] = lr
        return out
    mean = torch.empty(B, C, 1, 1, device=raw.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    call("srmi_batch_prep", ptr(raw), B, C, T, int(flip_index), int(scale), ptr(hr),
         ptr(lr) if with_lr else None, ptr(mean), ptr(std), stream_handle(stream))
    out = {"hr": hr, "mean": mean, "std": std, "xyflip": int(flip_index)}
    if with_lr:
        out["lr"] = lr
    return out


def _prep_batch_land(raw, flip_index, scale, with_lr, hr, lr, stream, norm, stats, min_wet):
    from .norm import DATASET_NORMS, MODES, check_norm
    if check_norm(norm) in ("tnorm", "tscale"):
        raise ValueError(f"prep_batch: norm {norm!r} with land=True: its statistics rows belong to the tiles of the "
                         "all-wet keep list (use lnorm, lscale, gnorm or gscale)")
    if norm in DATASET_NORMS and stats is None:
        raise ValueError(f"prep_batch: norm {norm!r} needs the dataset statistics (stats=NormStats)")
    if min_wet is not None and not 0.0 < float(min_wet) <= 1.0:
        raise ValueError(f"prep_batch: min_wet {min_wet!r} outside (0, 1]")
    if raw.dtype != torch.float32 or raw.dim() != 4 or not raw.is_contiguous():
        raise ValueError("prep_batch: raw must be a contiguous fp32 [B, C, T, T] tensor")
    B, C, T, T2 = raw.shape
    if T != T2:
        raise ValueError("prep_batch: tiles must be square (xyflip swaps the axes)")
    dev = raw.device
    if hr is None:
        hr = torch.empty_like(raw)
    if with_lr and lr is None:
        lr = torch.empty(B, C, T // scale, T // scale, device=dev, dtype=torch.float32)
    off = div = None
    if norm in DATASET_NORMS:  # gnorm / gscale: one constant pair per channel, whatever the tile
        off, div = (v.to(dev) for v in stats.offsets(norm, (0, B)))
        if tuple(off.shape) != (B, C):  # the kernel reads B * C of each
            raise ValueError(f"{norm}: statistics rows {tuple(off.shape)} for a batch of {B} x {C}")
    a = torch.empty(B, C, 1, 1, device=dev, dtype=torch.float32)
    b = torch.empty_like(a)
    nwet = torch.empty(B, C, device=dev, dtype=torch.int32)
    call("srmi_batch_prep_masked", ptr(raw), B, C, T, int(flip_index), int(scale), MODES[norm], ptr(off), ptr(div),
         ptr(hr), ptr(lr) if with_lr else None, ptr(a), ptr(b), ptr(nwet), stream_handle(stream))
    out = {"hr": hr, "xyflip": int(flip_index), "nwet": nwet}
    if norm == "lnorm":
        out.update(mean=a, std=b)
    elif norm == "lscale":  # the exact maximum of the wet pixels (as prep_norm: min + (max - min) need not give it)
        wet = torch.isfinite(raw)
        out.update(min=a, max=torch.where(wet, raw, torch.full_like(raw, float("-inf"))).amax(dim=(2, 3), keepdim=True))
    if with_lr:
        out["lr"] = lr
    return out
