"""Super-resolve a low-resolution region: overlapping tiles, blended into one mosaic.

No reference counterpart -- a deliberate extension, not a parity item.  The reference
(and srmi.inference.TiledInference, its drop-in) starts from a HIGH-resolution region,
downsamples it, runs the model and scores the result against the region it started
from: an evaluation harness.  Its tiles are the disjoint floor grid of get_tiles
(sres/base/source/swot/raw.py:216-233) and its mosaic the plain concatenation of
assemble_images (sres/controller/dual_trainer.py:482-512), so the rows and columns past
the last whole tile are dropped and neighbouring tiles, each normalised and convolved
alone with zero padding, disagree along every seam.

``RegionSuperResolver`` takes the coarse field itself, [C, h, w], and returns the
[C, s h, s w] field: the LR region is cut into overlapping tiles
(``srmi_region_to_tiles_overlap``), the tiles go through the inference engine, and the
outputs are blended with a feathered window (``srmi_tiles_blend``) -- full coverage,
all on the device.  ``score`` gives the result one number, its RMSE against a truth;
``score_spectra`` adds the windowed radial power spectra of srmi.spectra.

The plan
--------
Each axis is three integers, in LR pixels for cutting and in output pixels (times the
model scale) for blending: length ``L``, tile ``t``, stride ``S`` with 1 <= S <= t <= L;
the overlap is ``R = t - S``.  It has ``n = ceil((L - t) / S) + 1`` tiles, tile ``i`` at
the origin ``min(i S, L - t)``: the last tile is shifted inward, so the axis is always
covered completely.  A pixel may be covered by THREE tiles of an axis (the shifted last
tile next to two regular ones) whenever ``L - t - (n - 2) S < R``.

The blend weight along an axis is the integer ramp ``w(p) = min(p + 1, t - p, R + 1)``
at tile-local position ``p``; the 2-D weight is ``wy wx`` and the blended value
``sum_k w_k v_k / sum_k w_k`` over the non-bad tiles covering the pixel.  Across a
regular overlap the two weights are ``(R - q) / (R + 1)`` and ``(q + 1) / (R + 1)``: a
linear ramp that never reaches zero.  With ``R = 0`` every weight is 1, so a ragged edge
at ``R = 0`` AVERAGES the shifted last tile with its neighbour where the two overlap
(and a region the tile divides is the plain mosaic).

Bad tiles: by default (``land=False``) a tile holding a non-finite value is flagged by
the cut, rides through the forward, and is ignored by the blend (its values are never
read).  A pixel whose covering tiles are all bad is NaN -- so one land pixel blanks up
to a whole tile of ocean around it.

Land (``land=True``)
--------------------
For regions whose land, ice or missing data is NaN (srmi.llc writes land as NaN).  The
cut is ``srmi_region_to_tiles_overlap_masked``: a tile's statistics are taken over its
finite ("wet") pixels only, its dry pixels are flood-filled in normalised space from
the wet ones (pass by pass, the mean of the already filled 8-neighbours), and it is bad
only when some channel has fewer than ``min_wet`` (a fraction of the tile plane) wet
pixels; a bad tile is all zeros and, as above, ignored by the blend.  The blend is
``srmi_tiles_blend_masked``: every HR pixel whose LR parent is not finite is NaN again,
every other pixel is the plain blend of the non-bad tiles covering it.  So the holes of
the result are the land itself (plus the pixels all of whose tiles are bad), not the
tiles around it.  'interpolated' becomes the TILED baseline: the upsample of the filled,
normalised LR tiles, blended and re-masked the same way (upsampling is affine-invariant,
so the blend's x * div + off de-normalises it) -- the whole-region upsample of a NaN
field would lose a strip of ocean along every coast.  ``score`` takes an HR truth with
NaN and counts only the pixels where both sides are finite
(``srmi_rmse_partial_masked``).  No host synchronisation anywhere: the fill's trip count
is decided on the device, so ``graph=True`` works and one captured graph serves regions
with different coasts.

Self-ensemble (``ensemble=4`` or ``8``)
---------------------------------------
The "+" variant of the RCAN / EDSR papers, and a per-pixel spread.  No retraining: the
model runs on K dihedral variants of every tile (``srmi_tiles_dihedral``; variant f is
the reference's xyflip -- bit 0 flips x, bit 1 flips y, bit 2 then swaps the axes; 4
takes the flips, 8 the swaps as well, which need a square tile), and the blend
(``srmi_tiles_blend_ensemble``) reads every output back through the inverse map, blends
each variant exactly as above and returns their mean as 'model' and their standard
deviation (ddof 0) as 'spread'.  The network is not dihedral-equivariant (zero padding,
PixelShuffle and the learned filters break the symmetry), so the mean is a real gain and
the spread the cheapest honest proxy for where to trust the field.  With ``land=True`` the
variants are transforms of the FILLED tile, and both images are re-masked.  The cost is
K forwards; the two added launches are noise beside them.

Members (``members=True``, with ``ensemble`` > 1)
-------------------------------------------------
The K blended, back-transformed member fields as a product, 'members' [K, C, s h, s w]: member j
is the blend of variant ``variants[j]`` alone, de-normalised -- the B_j whose mean and standard
deviation 'model' and 'spread' are.  No kernel of its own: ``srmi_tiles_blend_ensemble`` called on
slab j with the single-bit mask ``1 << variants[j]`` and no spread returns B_j bit for bit (the K
= 1 case of its contract), so K such calls behind the blend, inside the captured graph, write
them (``land=True``: re-masked as 'model' is).  The members are the RAW blended outputs: they
come BEFORE ``quantile_map`` and BEFORE ``consistent=K``, which change 'model' and leave
'members' and 'spread' as they are; with neither, the pairwise fp32 mean and spread of
'members' are 'model' and 'spread' bit for bit.  ``score_ensemble`` verifies them against a truth
(srmi.ensemble_score: CRPS, rank histogram, spread-skill ratio, reliability table).

Consistency (``consistent=K``, 1 <= K <= 16)
--------------------------------------------
Nothing above ties D('model') to the input, D being the task's downsample: the tiles are
normalised with LR statistics, the seams are blended and the network is unconstrained.
``consistent=K`` runs K steps of iterative back-projection, x <- x + U(input - D x) with U
the task's upsample, on the blended 'model' (after the ensemble mean), in physical units and
in place.  At an even scale D reads only the s x s children of an LR pixel, so the loop
never runs at HR size: with r0 = input - D x0 and E = I - D U it is x_K = x0 + U(R_K), R_K =
sum_{k < K} E^k r0, and D U is a 5-tap (3-tap for a bilinear U) clamped-index stencil per
axis in LR space.  One read of the HR field (``srmi_consistency_residual``), K stencils on
LR-size buffers (``srmi_consistency_iterate``) and one read-modify-write of the HR field
(``srmi_consistency_apply``).  E contracts for all four mode pairs at s = 4 and 8 (spectral
radius 0.03 for cubic / cubic at s = 4, 0.43 for linear / linear).
The images gain 'residual' = r0 [C, h, w], the raw model's inconsistency, and
'residual_left' = E^K r0, what the corrected field still misses.  An LR cell takes part iff
its input is finite and every tap of D in 'model' is; the others have a zero residual at
every step, and a non-finite pixel of 'model' is never written, so with ``land=True`` and
bad tiles the NaN set and bits of 'model' are what they were.  'interpolated' and 'spread'
are untouched; ``score`` and ``score_spectra`` score the corrected field.

Quantile mapping (``quantile_map=QuantileMap``)
-----------------------------------------------
An RMSE-trained network pulls its output to the mean and under-fills the tails
(``score_distribution``'s 'q_bias').  With a fitted srmi.quantile_map.QuantileMap, 'model' is
mapped in place through its transfer table (``srmi_quantile_map_apply``): x <- x + qm_strength
(T(v) - v), with v = x - 'interpolated' for a map on="detail" and v = x for on="value".  The
order is fixed: AFTER the blend (the ensemble's included, so the mean is mapped, and 'spread'
is what it is without) and BEFORE the consistency correction, so ``consistent=K`` re-imposes
the coarse constraint on the mapped field -- the map moves values, the back-projection
restores what it moved at the coarse scale.  A NaN pixel is written back as it was, so
``land=True`` needs nothing more.  ``fit_quantile_map`` calibrates a map on regions whose
truth is known.  Out of scope: srmi.inference.TiledInference, training through the map, and a
map that varies in space or with the season.
"""
from __future__ import annotations

import math
import numbers
from typing import Dict, List, Mapping, Optional, Tuple

import torch

from ._lib import (SRMI_ERR_ARG, SRMI_INTERP_BICUBIC, SRMI_INTERP_BILINEAR, SRMI_NORM_AFFINE, call, load, ptr,
                   stream_handle)
from .engine import Engine, NetSpec, downsample, engine_stream, upsample

SUPPORTED_NORMS = ("lnorm", "lscale", "gnorm", "gscale")


# ------------------------------------------------------------------ the plan
def overlap_count(L: int, t: int, S: int) -> int:
    """Number of tiles of the axis plan (L, t, S): ceil((L - t) / S) + 1."""
    L, t, S = int(L), int(t), int(S)
    if not 1 <= S <= t <= L:
        raise ValueError(f"overlap plan needs 1 <= S <= t <= L, got L={L} t={t} S={S}")
    return -((t - L) // S) + 1


def overlap_plan(L: int, t: int, S: int) -> List[int]:
    """Tile origins of the axis plan (L, t, S): min(i S, L - t) for i < n -- strictly
    increasing, the first 0, the last L - t.  At S == t on a ragged axis (L % t != 0)
    the shifted last tile overlaps its neighbour, and the blend averages the two there."""
    n = overlap_count(L, t, S)
    return [min(i * int(S), int(L) - int(t)) for i in range(n)]


def blend_weight(p: int, t: int, S: int) -> int:
    """Integer blend weight at tile-local position p of a tile t at stride S."""
    if not 0 <= p < t:
        raise ValueError(f"position {p} outside a tile of {t}")
    return min(p + 1, t - p, t - S + 1)


def lib_overlap_count(L: int, t: int, S: int) -> int:
    """srmi_overlap_count of the library (host only): n, or ValueError where it returns
    SRMI_ERR_ARG."""
    n = load().srmi_overlap_count(int(L), int(t), int(S))
    if n == SRMI_ERR_ARG:
        raise ValueError(f"overlap plan needs 1 <= S <= t <= L, got L={L} t={t} S={S}")
    return n


def ensemble_variants(ensemble, tile_lr: Tuple[int, int]) -> Tuple[int, ...]:
    """The dihedral variants of a self-ensemble, ascending: 1 -> (0,), 4 -> the flips
    (0, 1, 2, 3), 8 -> all of (0, .., 7); or a sequence of variant indices -- non-empty,
    unique, within 0 .. 7 and holding 0 (the untransformed tile) -- returned sorted.
    Variant f is xyflip's: bit 0 flips x, bit 1 flips y, bit 2 swaps the axes, so f >= 4
    needs a square tile.  Anything else: ValueError."""
    ty, tx = (int(v) for v in tile_lr)
    if isinstance(ensemble, bool):
        raise ValueError(f"ensemble {ensemble!r}: 1, 4, 8 or a sequence of variant indices")
    if isinstance(ensemble, numbers.Integral):
        if ensemble not in (1, 4, 8):
            raise ValueError(f"ensemble {ensemble!r}: 1, 4, 8 or a sequence of variant indices")
        var = tuple(range(int(ensemble)))
    else:
        try:
            items = list(ensemble)
        except TypeError:
            raise ValueError(f"ensemble {ensemble!r}: 1, 4, 8 or a sequence of variant indices") from None
        if not items or any(isinstance(f, bool) or not isinstance(f, numbers.Integral) for f in items):
            raise ValueError(f"ensemble {ensemble!r}: a non-empty sequence of integer variant indices")
        items = [int(f) for f in items]
        if len(set(items)) != len(items) or min(items) < 0 or max(items) > 7 or 0 not in items:
            raise ValueError(f"ensemble {ensemble!r}: unique variant indices within 0 .. 7, variant 0 among them")
        var = tuple(sorted(items))
    if var[-1] >= 4 and ty != tx:
        raise ValueError(f"ensemble {ensemble!r}: the variants that swap the axes (>= 4) need a square tile, tile_lr "
                         f"is {(ty, tx)}; use ensemble=4 (the flips only)")
    return var


INTERP_MODES = {"bilinear": SRMI_INTERP_BILINEAR, "bicubic": SRMI_INTERP_BICUBIC}
MAX_CONSISTENT = 16


def check_consistent(consistent, scale: int, dmode: str, umode: str) -> int:
    """The ``consistent`` argument of RegionSuperResolver as an int: an integer 0 .. 16, and,
    when positive, an even scale (>= 4 under a bicubic downsample, whose taps would leave
    the s x s block otherwise) and bilinear / bicubic modes.  Anything else: ValueError."""
    if isinstance(consistent, bool) or not isinstance(consistent, numbers.Integral):
        raise ValueError(f"consistent {consistent!r}: an integer 0 .. {MAX_CONSISTENT}")
    k = int(consistent)
    if not 0 <= k <= MAX_CONSISTENT:
        raise ValueError(f"consistent {consistent!r} outside 0 .. {MAX_CONSISTENT}")
    if k == 0:
        return 0
    if dmode not in INTERP_MODES or umode not in INTERP_MODES:
        raise ValueError(f"consistent={k} needs bilinear / bicubic resampling, the task has {dmode!r} / {umode!r}")
    smin = 4 if dmode == "bicubic" else 2
    if int(scale) % 2 or int(scale) < smin:
        raise ValueError(f"consistent={k} needs an even scale >= {smin} under a {dmode} downsample, the model's is "
                         f"{scale}")
    return k


# ---------------------------------------------------------------- the class
class RegionSuperResolver:
    def __init__(self, spec: NetSpec, params: torch.Tensor, region_chw_lr: Tuple[int, int, int],
                 tile_lr: Tuple[int, int] = (48, 48), overlap: Tuple[int, int] = (8, 8), norm: Optional[str] = None,
                 task=None, stats=None, micro: Optional[int] = None, max_batch: int = 512, graph: bool = False,
                 device: Optional[torch.device] = None, land: bool = False, min_wet: float = 0.25, ensemble=1,
                 consistent: int = 0, quantile_map=None, qm_strength: float = 1.0, members: bool = False):
        """region_chw_lr: (C, h, w) of the LR regions; tile_lr: the LR tile the engine
        runs; overlap: LR pixels per axis, 0 <= overlap <= tile // 2 (stride = tile -
        overlap).

        norm / task: resolved as in TiledInference (task.norm, task.upsample_mode /
        downsample_mode; the active ConfigContext's task when neither is given).  The
        tile-local modes 'lnorm' and 'lscale' take their statistics from the LR tile
        itself; the global modes 'gnorm' and 'gscale' take the dataset's global
        constants from ``stats`` (srmi.norm.NormStats), one row per tile, as the AFFINE
        mode.  'tnorm' and 'tscale' are refused: their statistics belong to the cells
        of a floor grid, which overlapping tiles are not.  The output is ALWAYS
        de-normalised (x * div + off, gnorm and gscale included): the purpose is a
        physical field, not the reference's normalised mosaics.

        An approximation, by construction: the model was trained on LR tiles that are
        the downsampled HR tile NORMALISED BY THE HR TILE'S statistics; with no HR, the
        LR tile's own statistics stand in for them (the mean of a bicubic 1/s of a
        tile is close to the tile's, its spread somewhat smaller).

        micro engines on their own streams share the tiles as TiledInference's do;
        each runs its share in equal chunks of at most max_batch tiles (the forward
        computes every tile alone, so neither changes a bit of the result).  An engine's
        workspace grows with its chunk, and it refuses a chunk whose largest activation
        map reaches 4 GiB (about 900 tiles of 48 x 48 at scale 4): lower max_batch for
        larger tiles.  One chunk per engine is fastest (the inference RCAB runs one
        workgroup per tile, so every chunk ends in a partly filled round of the engine's
        CUs: 1024^2 LR at overlap 8 lost 2 % to chunks of 169).  graph: capture the
        whole sequence in a HIP graph and replay it per region (bit-identical).
        Multi-rank mode is not offered.  set_params as in TiledInference.

        land: the region may hold NaN (land); see the module docstring.  min_wet, in
        (0, 1]: the share of a tile plane that must be wet in every channel for the tile
        to be used (the ABI gets max(1, ceil(min_wet ty tx)) pixels).  land=False is the
        object as it was, bit for bit.

        ensemble: 1, 4, 8 or a sequence of variant indices (``ensemble_variants``); see
        the module docstring.  With K > 1 variants the K n transformed tiles go through
        the same engines (micro and max_batch split K n tiles), 'model' is the mean of
        the K blended outputs and the images gain 'spread'.  The tile and output buffers
        and the forward's time grow K-fold, and the 4 GiB bound above is reached by a
        chunk of K n tiles as by any other: keep max_batch.  ensemble=1 is the object as
        it was, bit for bit.

        consistent: an integer 0 .. 16, the steps of back-projection applied to 'model'
        (see the module docstring).  It needs an even scale, >= 4 when the task's
        downsample is bicubic: ValueError otherwise.  consistent=0 is the object as it
        was, bit for bit.

        quantile_map: a fitted srmi.quantile_map.QuantileMap of C channels on this device,
        applied to 'model' with qm_strength in [0, 1] (see the module docstring); ValueError
        for another channel count or device, an unfitted map or a strength outside [0, 1].
        The apply sits inside the captured graph (graph=True), which reads the map's device
        buffers: a refit of the SAME object (accumulate, fit, load_state_dict) takes effect at
        the next replay, with no recapture -- as long as the map's ``on`` stays what it was,
        because whether the base is passed is part of the captured launch; qm_strength and
        ``on`` are fixed at construction (a state of another ``on`` needs a new resolver).
        quantile_map=None is the object as it was, bit for bit.

        members: with ensemble > 1 (ValueError otherwise), the images gain 'members' [K, C, s h,
        s w], the K blended member fields before ``quantile_map`` and ``consistent`` (see the
        module docstring), at K more blend launches and K output-sized planes.  members=False is
        the object as it was, bit for bit: no buffer, image key or launch is added."""
        if task is None:  # the active srmi ConfigContext's task section, if any
            from . import config as _config
            task = _config._CURRENT.get("task") if _config._CURRENT is not None else None
        from .config import interp_mode
        from .norm import MODES, check_norm, norm_type
        self.norm = check_norm(norm) if norm is not None else norm_type(task)
        if self.norm not in SUPPORTED_NORMS:
            raise ValueError(f"norm {self.norm!r}: its statistics belong to floor-grid cells; overlapping tiles take "
                             f"one of {SUPPORTED_NORMS}")
        self.norm_mode = MODES[self.norm]
        if self.norm_mode == SRMI_NORM_AFFINE and stats is None:
            raise ValueError(f"norm {self.norm!r} needs the dataset statistics (stats=NormStats)")
        self.dmode, self.umode = interp_mode(task, True), interp_mode(task, False)
        self.consistent = check_consistent(consistent, spec.scale, self.dmode, self.umode)
        self.spec = spec
        self.device = device or params.device
        self.quantile_map, self.qm_strength = quantile_map, float(qm_strength)
        self._qm_on = None if quantile_map is None else quantile_map.on
        if quantile_map is not None:
            dv = torch.device(self.device)
            if dv.type == "cuda" and dv.index is None:
                dv = torch.device("cuda", torch.cuda.current_device())
            if quantile_map.C != int(region_chw_lr[0]):
                raise ValueError(f"quantile_map holds {quantile_map.C} channels, the region has {int(region_chw_lr[0])}")
            if quantile_map.device != dv:
                raise ValueError(f"quantile_map lives on {quantile_map.device}, the resolver on {dv}")
            if not quantile_map.fitted:
                raise ValueError("quantile_map has no table yet: fit() or load_state_dict() it first")
            if not (math.isfinite(self.qm_strength) and 0.0 <= self.qm_strength <= 1.0):
                raise ValueError(f"qm_strength {qm_strength!r}: a number in [0, 1]")
        C, h, w = (int(v) for v in region_chw_lr)
        if C != spec.nchannels_in or spec.nchannels_in != spec.nchannels_out:
            raise ValueError("region channels must equal the model's input/output channels")
        ty, tx = (int(v) for v in tile_lr)
        ry, rx = (int(v) for v in overlap)
        if ty < 1 or tx < 1 or h < ty or w < tx:
            raise ValueError(f"region {(h, w)} smaller than one tile {(ty, tx)}")
        if not (0 <= ry <= ty // 2 and 0 <= rx <= tx // 2):
            raise ValueError(f"overlap {(ry, rx)} outside 0 .. tile // 2 = {(ty // 2, tx // 2)}")
        self.variants = ensemble_variants(ensemble, (ty, tx))
        self.vmask = sum(1 << f for f in self.variants)
        K = self.K = len(self.variants)
        self.members = bool(members)
        if self.members and K == 1:
            raise ValueError("members=True needs ensemble > 1: one variant has no members beside 'model'")
        s = spec.scale
        self.C, self.h, self.w, self.ty, self.tx, self.s = C, h, w, ty, tx, s
        self.land = bool(land)
        if self.land:
            if not 0.0 < float(min_wet) <= 1.0:
                raise ValueError(f"min_wet {min_wet!r} outside (0, 1]")
            self.min_wet = max(1, math.ceil(float(min_wet) * ty * tx))
        self.sy, self.sx = ty - ry, tx - rx
        self.ny, self.nx = overlap_count(h, ty, self.sy), overlap_count(w, tx, self.sx)
        n = self.n = self.ny * self.nx
        self.params = params
        d = self.device
        f32 = dict(dtype=torch.float32, device=d)
        self.region = torch.empty((C, h, w), **f32)
        self.tiles = torch.empty((n, C, ty, tx), **f32)
        self.off = torch.empty((n, C), **f32)
        self.div = torch.empty((n, C), **f32)
        if self.norm_mode == SRMI_NORM_AFFINE:
            # filled once, before any capture: the cut reads them, the blend undoes them
            off, div = stats.offsets(self.norm, (0, n))
            if tuple(off.shape) != (n, C):
                raise ValueError(f"stats hold {tuple(off.shape[1:])} channels, the region has {C}")
            self.off.copy_(off)
            self.div.copy_(div)
        self.bad = torch.zeros(n, dtype=torch.int32, device=d)
        if K == 1:
            self.sr = torch.empty((n, C, ty * s, tx * s), **f32)
            self._fin, self._fout = self.tiles, self.sr  # what the forward reads and writes
        else:
            self.vtiles = torch.empty((K, n, C, ty, tx), **f32)  # the variants of self.tiles
            self.sr = torch.empty((K, n, C, ty * s, tx * s), **f32)  # their outputs, in the transformed frame
            self._fin, self._fout = self.vtiles.view(K * n, C, ty, tx), self.sr.view(K * n, C, ty * s, tx * s)
        self.images = {"input": self.region, "interpolated": torch.empty((C, h * s, w * s), **f32),
                       "model": torch.empty((C, h * s, w * s), **f32)}
        if K > 1:
            self.images["spread"] = torch.empty((C, h * s, w * s), **f32)
        if self.members:
            self.images["members"] = torch.empty((K, C, h * s, w * s), **f32)
        if self.land:
            self.nwet = torch.zeros((n, C), dtype=torch.int32, device=d)
            self.up = torch.empty((n, C, ty * s, tx * s), **f32)  # the tiled baseline's tiles
            self.images["nwet"] = self.nwet
        if self.consistent:
            # r0, the ping-pong pair of the iteration, its sum R and the active mask: LR size
            self._cr = [torch.empty((C, h, w), **f32) for _ in range(3 if self.consistent > 1 else 2)]
            self._cR = torch.empty((C, h, w), **f32)
            self._cact = torch.empty((C, h, w), dtype=torch.int32, device=d)
            self.images["residual"] = self._cr[0]
            self.images["residual_left"] = self._cr[1 + (self.consistent - 1) % 2]
        n = self.nfwd = K * n  # the forward's tiles: the split and the chunks are taken over all of them
        if micro is None:
            micro = 2 if n >= 32 else 1
        self.micro = max(1, min(int(micro), n))
        per = (n + self.micro - 1) // self.micro
        self.split = [max(1, min(per, n - k * per)) for k in range(self.micro)]
        self.max_batch = max(1, int(max_batch))
        budget = 256 // self.micro if self.micro > 1 else 0
        # an engine's share in the fewest chunks max_batch allows, of equal size
        self.engs = [Engine(spec, -(-m // -(-m // self.max_batch)), (ty, tx), train=False, device=d, cu_budget=budget)
                     for m in self.split]
        self.eng = self.engs[0]
        for e in self.engs:
            e.pack(params)
        self.streams = [None] + [engine_stream(d) for _ in range(self.micro - 1)]
        self.ev_fork = torch.cuda.Event()
        self.ev_join = [torch.cuda.Event() for _ in range(self.micro - 1)]
        self.loss_m = torch.zeros(4, **f32)
        self.loss_i = torch.zeros(4, **f32)
        self._graph = None
        self._spectra = {}  # (window, stride) -> the SpectralScore of each image (score_spectra)
        self._ssim = {}  # (data_range, maps) -> the SSIMScore of each image (score_ssim)
        self._distribution = {}  # (bins, joint, probs, value_range) -> the DistributionScore of each image
        self._gradient = {}  # (spacing, maps, distribution) -> (GradientScore, DistributionScore | None) of each image
        self._fss = {}  # (thresholds, probs, scales, on) -> the scorers of each image (score_fss)
        self._ens = {}  # (edges, probs, crps_map) -> (DistributionScore | None, EnsembleScore) (score_ensemble)
        self._use_graph = bool(graph) and self.device.type == "cuda"

    # ---------------------------------------------------------------- pieces
    def _cut(self):
        if self.land:
            call("srmi_region_to_tiles_overlap_masked", ptr(self.region), self.C, self.h, self.w, self.ty, self.tx,
                 self.sy, self.sx, self.norm_mode, ptr(self.off), ptr(self.div), ptr(self.tiles), ptr(self.off),
                 ptr(self.div), ptr(self.bad), self.min_wet, ptr(self.nwet), stream_handle())
            return
        call("srmi_region_to_tiles_overlap", ptr(self.region), self.C, self.h, self.w, self.ty, self.tx, self.sy,
             self.sx, self.norm_mode, ptr(self.off), ptr(self.div), ptr(self.tiles), ptr(self.off), ptr(self.div),
             ptr(self.bad), stream_handle())

    def _forward(self):
        main = torch.cuda.current_stream(self.device)
        self.ev_fork.record(main)
        for sk in self.streams[1:]:
            sk.wait_event(self.ev_fork)
        a = 0
        for k, e in enumerate(self.engs):
            b = min(self.nfwd, a + self.split[k])
            for c0 in range(a, b, e.batch):
                c1 = min(b, c0 + e.batch)
                if self.streams[k] is None:
                    e.forward(self.params, self._fin[c0:c1], out=self._fout[c0:c1])
                else:
                    with torch.cuda.stream(self.streams[k]):
                        e.forward(self.params, self._fin[c0:c1], out=self._fout[c0:c1])
            a = b
        for sk, ev in zip(self.streams[1:], self.ev_join):
            ev.record(sk)
            main.wait_event(ev)

    def _blend_masked(self, tiles: torch.Tensor, out: torch.Tensor):
        s = self.s
        call("srmi_tiles_blend_masked", ptr(tiles), ptr(self.off), ptr(self.div), ptr(self.bad), self.C, self.ty * s,
             self.tx * s, self.sy * s, self.sx * s, self.h * s, self.w * s, ptr(self.region), s, ptr(out),
             stream_handle())

    def _expand(self):
        """self.tiles -> self.vtiles: the K dihedral variants of every tile plane."""
        call("srmi_tiles_dihedral", ptr(self.tiles), self.n * self.C, self.ty, self.tx, self.vmask, ptr(self.vtiles),
             stream_handle())

    def _blend(self):
        s = self.s
        if self.K > 1:
            call("srmi_tiles_blend_ensemble", ptr(self.sr), self.vmask, ptr(self.off), ptr(self.div), ptr(self.bad),
                 self.C, self.ty * s, self.tx * s, self.sy * s, self.sx * s, self.h * s, self.w * s,
                 ptr(self.region) if self.land else None, s, ptr(self.images["model"]), ptr(self.images["spread"]),
                 stream_handle())
            return
        if self.land:
            self._blend_masked(self.sr, self.images["model"])
            return
        call("srmi_tiles_blend", ptr(self.sr), ptr(self.off), ptr(self.div), ptr(self.bad), self.C, self.ty * s,
             self.tx * s, self.sy * s, self.sx * s, self.h * s, self.w * s, ptr(self.images["model"]), stream_handle())

    def _members(self):
        """'members'[j] <- the blend of slab j alone: the ensemble blend's K = 1 case, B_j bit for bit."""
        s = self.s
        for j, f in enumerate(self.variants):
            call("srmi_tiles_blend_ensemble", ptr(self.sr[j]), 1 << f, ptr(self.off), ptr(self.div), ptr(self.bad),
                 self.C, self.ty * s, self.tx * s, self.sy * s, self.sx * s, self.h * s, self.w * s,
                 ptr(self.region) if self.land else None, s, ptr(self.images["members"][j]), None, stream_handle())

    def _run(self, use_map: bool = True, correct: bool = True):
        self._cut()
        if self.K > 1:
            self._expand()
        self._forward()
        if self.land:  # the tiled baseline: every tile plane upsampled alone, blended like the model's
            upsample(self.tiles, self.s, out=self.up, mode=self.umode)
            self._blend_masked(self.up, self.images["interpolated"])
        else:
            upsample(self.region[None], self.s, out=self.images["interpolated"][None], mode=self.umode)
        self._blend()
        if self.members:
            self._members()
        if use_map and self.quantile_map is not None:
            qm, model = self.quantile_map, self.images["model"]
            if qm.on != self._qm_on:
                raise ValueError(f"quantile_map was on={self._qm_on!r} when this resolver was built and is "
                                 f"on={qm.on!r} now: build a new resolver")
            qm.apply(model, self.images["interpolated"] if qm.on == "detail" else None, self.qm_strength, out=model)
        if self.consistent and correct:
            self._correct()

    def _correct(self):
        """'model' <- 'model' + U(R_K) at its finite pixels; 'residual', 'residual_left'."""
        C, h, w, s, st = self.C, self.h, self.w, self.s, stream_handle()
        um, dm = INTERP_MODES[self.umode], INTERP_MODES[self.dmode]
        model = self.images["model"]
        call("srmi_consistency_residual", ptr(model), ptr(self.region), C, h, w, s, dm, ptr(self._cr[0]),
             ptr(self._cact), st)
        src = self._cr[0]
        for k in range(self.consistent):
            dst = self._cr[1 + k % 2]
            call("srmi_consistency_iterate", ptr(src), ptr(self._cact), C, h, w, s, um, dm, int(k == 0), ptr(self._cR),
                 ptr(dst), st)
            src = dst
        call("srmi_consistency_apply", ptr(self._cR), C, h, w, s, um, ptr(model), st)

    def _capture(self):
        self._run()  # warm-up outside capture (uploads engine tables)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                self._run()
        torch.cuda.current_stream(self.device).wait_stream(s)
        self._graph = g

    # ------------------------------------------------------------------- API
    def super_resolve(self, lr_region: torch.Tensor) -> Dict[str, torch.Tensor]:
        """lr_region [C, h, w] fp32 (device) -> {'input': the LR region, 'interpolated':
        task.upsample_mode of the whole LR region (untiled) [C, s h, s w], 'model': the
        blended model output [C, s h, s w], de-normalised}.  Device tensors, views of
        this object's buffers: valid until the next region.

        land=True: lr_region may hold NaN; 'model' and 'interpolated' (then the tiled
        baseline) are NaN exactly on the upsampled dry pixels and where every covering
        tile is bad, and 'nwet' [n, C] int32 holds the wet count of every tile plane.

        ensemble > 1: 'model' is the mean of the K back-transformed, blended outputs and
        'spread' [C, s h, s w] their standard deviation (ddof 0), in the physical units
        of 'model' and NaN where 'model' is; 'interpolated' is what it is without.

        consistent > 0: 'model' is the corrected field (the module docstring), 'residual'
        [C, h, w] the input minus the downsample of the uncorrected one and
        'residual_left' [C, h, w] what the corrected one still misses, both 0 at the LR
        cells that take no part; 'interpolated' and 'spread' are what they are without.

        members=True: 'members' [K, C, s h, s w], member j the blended, de-normalised output of
        variant ``variants[j]`` alone, NaN where 'model' is -- the raw blended outputs, before
        the quantile map and the consistency correction."""
        if tuple(lr_region.shape) != (self.C, self.h, self.w):
            raise ValueError(f"region shape {tuple(lr_region.shape)} != {(self.C, self.h, self.w)}")
        self.region.copy_(lr_region)
        if self._use_graph:
            if self._graph is None:
                self._capture()
            self._graph.replay()
        else:
            self._run()
        return self.images

    def score(self, hr_region: torch.Tensor) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
        """A number for choosing ``overlap``: hr_region [C, s h, s w] is downsampled
        whole by task.downsample_mode, super-resolved, and the whole-region RMSE of
        'model' and of 'interpolated' against it returned as 1-element device tensors
        (srmi_rmse_partial / _finalize): (images, {'model', 'interpolated'}).

        land=True: hr_region may hold NaN (its downsample is then NaN wherever a tap
        touches one); both losses are taken over the pixels where the image and
        hr_region are both finite (srmi_rmse_partial_masked), and the dict gains
        'count', that number of pixels for 'model' (no such pixel: the losses are NaN)."""
        s = self.s
        if tuple(hr_region.shape) != (self.C, self.h * s, self.w * s):
            raise ValueError(f"region shape {tuple(hr_region.shape)} != {(self.C, self.h * s, self.w * s)}")
        hr = hr_region.contiguous()
        images = self.super_resolve(downsample(hr[None], s, mode=self.dmode)[0])
        for name, l4 in (("model", self.loss_m), ("interpolated", self.loss_i)):
            if self.land:
                self.eng.rmse_partial_masked(images[name], hr, l4)
            else:
                self.eng.rmse_partial(images[name], hr, l4, float(hr.numel()))
            Engine.rmse_finalize(l4)
        losses = {"model": self.loss_m[3:4], "interpolated": self.loss_i[3:4]}
        if self.land:
            losses["count"] = self.loss_m[1:2]
        return images, losses

    def score_spectra(self, hr_region: torch.Tensor, window: int = 256, stride: Optional[int] = None):
        """``score``, then the spectral score (srmi.spectra.SpectralScore) of 'model' and of
        'interpolated' against hr_region: (images, losses, {'model': ..., 'interpolated':
        ...}), each entry the dict of SpectralScore.measure -- the windowed radial spectra
        of the image, of the truth and of their difference, the coherence, and the ratios
        from which srmi.spectra.effective_resolution reads the wavelength down to which an
        image beats the truth's variance.  window: the side in HR pixels, a power of two in
        16 .. 256; stride: window // 2 when None.  images and losses are ``score``'s, bit for
        bit; the spectra are views valid until the next call with the same window and
        stride.  No host synchronisation.  With graph=True the spectra are measured after
        the replay, outside the captured graph.

        land=True: a window that touches a NaN of the image or of hr_region is skipped
        ('nused' counts the rest), so a coast costs every window it crosses.  Filling the
        land before the transform is out of scope here."""
        from .spectra import SpectralScore
        s = self.s
        images, losses = self.score(hr_region)
        hr = hr_region.contiguous()
        key = (int(window), None if stride is None else int(stride))
        if key not in self._spectra:
            self._spectra[key] = {name: SpectralScore((self.C, self.h * s, self.w * s), window, stride,
                                                      device=self.device) for name in ("model", "interpolated")}
        return images, losses, {name: sc.measure(images[name], hr) for name, sc in self._spectra[key].items()}

    def score_ssim(self, hr_region: torch.Tensor, data_range: Optional[float] = None, maps: bool = False):
        """``score``, then the SSIM / PSNR score (srmi.ssim.SSIMScore) of 'model' and of
        'interpolated' against hr_region: (images, losses, {'model': ..., 'interpolated':
        ...}), each entry the dict of SSIMScore.measure -- per channel 'ssim', 'cs' (the
        contrast-structure factor, the number that falls when the output is too smooth),
        'mse', 'psnr', 'data_range', 'nwin', 'npix' and, with maps=True, 'map' [C, s h, s w],
        the per-pixel SSIM that belongs beside 'spread' and 'residual'.  data_range: L for
        every channel; None takes each channel's max - min of hr_region.  images and losses
        are ``score``'s, bit for bit; the entries are views valid until the next call with
        the same data_range and maps.  No host synchronisation.  With graph=True the score
        is measured after the replay, outside the captured graph.  ``ensemble`` and
        ``consistent`` change 'model' and nothing in how it is scored.

        land=True: the NaN of the image and of hr_region are the mask -- a position whose
        11 x 11 window touches one is not used ('nwin' counts the rest, 'map' is NaN
        there), so a coast costs a 5-pixel rim, not whole windows."""
        from .ssim import SSIMScore
        s = self.s
        images, losses = self.score(hr_region)
        hr = hr_region.contiguous()
        key = (None if data_range is None else float(data_range), bool(maps))
        if key not in self._ssim:
            self._ssim[key] = {name: SSIMScore((self.C, self.h * s, self.w * s), data_range, maps, device=self.device)
                               for name in ("model", "interpolated")}
        return images, losses, {name: sc.measure(images[name], hr) for name, sc in self._ssim[key].items()}

    def score_distribution(self, hr_region: torch.Tensor, bins: int = 256, joint: int = 32,
                           probs=(0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999), value_range=None):
        """``score``, then the distribution score (srmi.distribution.DistributionScore) of
        'model' and of 'interpolated' against hr_region: (images, losses, {'model': ...,
        'interpolated': ...}), each entry the dict of DistributionScore.measure -- per channel
        the histograms of the image and of the truth on the truth's range ('hist_pred',
        'hist_truth', 'lo', 'hi'), their joint histogram ('joint', which
        srmi.distribution.contingency turns into hits and misses above a threshold), 'count',
        the Perkins score 'pss', the Wasserstein-1 distance 'w1', the shares 'under' and
        'over' of the image outside the truth's range, and the quantiles 'q_pred', 'q_truth'
        with 'q_bias', the number that shows output pulled to the mean: positive at low
        probabilities and negative at high ones.  bins, joint, probs, value_range: as
        DistributionScore takes them.  images and losses are ``score``'s, bit for bit; the
        entries are views valid until the next call with the same arguments.  No host
        synchronisation.  With graph=True the score is measured after the replay, outside the
        captured graph.

        land=True: the NaN of the image and of hr_region are the mask, pixel by pixel
        ('count' is what is left)."""
        from .distribution import DistributionScore
        s = self.s
        images, losses = self.score(hr_region)
        hr = hr_region.contiguous()
        key = (int(bins), int(joint), tuple(float(p) for p in probs),
               None if value_range is None else tuple(float(v) for v in value_range))
        if key not in self._distribution:
            self._distribution[key] = {name: DistributionScore((self.C, self.h * s, self.w * s), bins, joint, probs,
                                                               value_range, device=self.device)
                                       for name in ("model", "interpolated")}
        return images, losses, {name: sc.measure(images[name], hr) for name, sc in self._distribution[key].items()}

    def score_gradient(self, hr_region: torch.Tensor, spacing=(1.0, 1.0), maps: bool = False, distribution=None):
        """``score``, then the gradient score (srmi.gradient.GradientScore) of 'model' and of
        'interpolated' against hr_region: (images, losses, {'model': ..., 'interpolated':
        ...}), each entry the dict of GradientScore.measure -- per channel 'count' (the used
        positions), 'mean_pred', 'mean_truth' (the mean Sobel gradient magnitudes, in the
        field's units per unit of ``spacing`` = (dy, dx)), 'sharpness' (their ratio: below 1
        the fronts are too smooth), 'rmse_mag', 'rmse_vec', 'cosine' (1: every front points
        as the truth's does), 'sums', and with maps=True 'gmag_pred', 'gmag_truth' [C, s h,
        s w], NaN where a position is not used.

        distribution: None, or dict(bins=256, joint=32, value_range=None): each entry gains
        'distribution', srmi.distribution.DistributionScore.measure run on the two magnitude
        maps (their NaN are its mask), whose 'joint' table srmi.distribution.contingency turns
        into hits, misses, false alarms, CSI and frequency bias of fronts above a threshold.
        The maps are then produced (and returned) whether or not maps=True.

        images and losses are ``score``'s, bit for bit; the entries are views valid until the
        next call with the same arguments.  No host synchronisation.  With graph=True the
        score is measured after the replay, outside the captured graph.

        land=True: the NaN of the image and of hr_region are the mask -- a position whose 3 x
        3 window touches one is not used, so a coast costs a one-pixel rim."""
        from .distribution import DistributionScore
        from .gradient import GradientScore, check_spacing
        s = self.s
        check_spacing(spacing)
        dcfg = None
        if distribution is not None:
            if not isinstance(distribution, Mapping):
                raise ValueError(f"distribution: a dict(bins=, joint=, value_range=) or None, got {distribution!r}")
            extra = set(distribution) - {"bins", "joint", "value_range"}
            if extra:
                raise ValueError(f"distribution: unknown keys {sorted(extra)}")
            vr = distribution.get("value_range")
            try:
                dcfg = (int(distribution.get("bins", 256)), int(distribution.get("joint", 32)),
                        None if vr is None else tuple(float(v) for v in vr))
            except (TypeError, ValueError):
                raise ValueError(f"distribution {dict(distribution)!r}: bins and joint whole numbers, value_range "
                                 "None or a (lo, hi) pair") from None
        key = (tuple(float(v) for v in spacing), bool(maps), dcfg)
        shape = (self.C, self.h * s, self.w * s)
        if tuple(hr_region.shape) != shape:
            raise ValueError(f"region shape {tuple(hr_region.shape)} != {shape}")
        if key not in self._gradient:  # before the region is inferred: the constructors refuse bad arguments
            self._gradient[key] = {
                name: (GradientScore(shape, spacing, bool(maps) or dcfg is not None, device=self.device),
                       DistributionScore(shape, dcfg[0], dcfg[1], value_range=dcfg[2], device=self.device)
                       if dcfg is not None else None)
                for name in ("model", "interpolated")}
        images, losses = self.score(hr_region)
        hr = hr_region.contiguous()
        out = {}
        for name, (gs, ds) in self._gradient[key].items():
            res = dict(gs.measure(images[name], hr))
            if ds is not None:
                res["distribution"] = ds.measure(res["gmag_pred"], res["gmag_truth"])
            out[name] = res
        return images, losses, out

    def score_fss(self, hr_region: torch.Tensor, thresholds=None, probs=(0.9, 0.99),
                  scales=(1, 3, 5, 9, 17, 33, 65), on: str = "value"):
        """``score``, then the fractions skill score (srmi.fss.FractionsSkillScore) of 'model' and
        of 'interpolated' against hr_region: (images, losses, {'model': ..., 'interpolated':
        ...}), each entry the dict of FractionsSkillScore.measure -- per channel and threshold
        the integer tables 'num', 'den' over the ladder ``scales`` of odd neighbourhood sizes,
        'events_pred', 'events_truth', 'used', 'fss', 'f_pred', 'f_truth', 'bias', 'target',
        'afss' and 'skilful_scale', the smallest neighbourhood at which the image is useful --
        plus 'thresholds' [C, T] fp32, the ones used.

        thresholds: T floats (the same for every channel), a [C, T] array or a [C, T] fp32 device
        tensor (kept by reference).  None: the truth's quantiles at ``probs``, taken on the
        device from a srmi.distribution.DistributionScore (1024 bins) of the same two fields
        ('q_truth', cast to fp32 on the device) -- no host read.

        on="value" scores the fields themselves; on="gradient" scores the fronts: the two fields
        are srmi.gradient.GradientScore's magnitude maps of the image and of hr_region at unit
        spacing, whose NaN rim and coast are the mask, and the quantiles are of the truth's map.

        images and losses are ``score``'s, bit for bit; the entries are views valid until the
        next call with the same arguments.  No host synchronisation.  With graph=True the score
        is measured after the replay, outside the captured graph.

        land=True: the NaN of the image and of hr_region are the mask, pixel by pixel: what is
        not used is "no event" in both fields ('used' is what is left)."""
        from .distribution import DistributionScore
        from .fss import FractionsSkillScore, check_scales
        from .gradient import GradientScore
        s = self.s
        if on not in ("value", "gradient"):
            raise ValueError(f"on {on!r}: 'value' or 'gradient'")
        sc = check_scales(scales)
        shape = (self.C, self.h * s, self.w * s)
        if tuple(hr_region.shape) != shape:
            raise ValueError(f"region shape {tuple(hr_region.shape)} != {shape}")
        if thresholds is None:
            pr = tuple(float(p) for p in probs)
            if not 1 <= len(pr) <= 8:
                raise ValueError(f"probs {probs!r}: 1 .. 8 probabilities strictly inside (0, 1)")
            tkey = None
        elif isinstance(thresholds, torch.Tensor):
            pr, tkey = (), ("tensor", thresholds.data_ptr(), tuple(thresholds.shape))
        else:
            import numpy as np
            pr, tkey = (), tuple(np.asarray(thresholds, dtype=np.float32).reshape(-1).tolist())
        key = (tkey, pr, sc, on)
        if key not in self._fss:  # before the region is inferred: the constructors refuse bad arguments
            made = {}
            for name in ("model", "interpolated"):
                ds = DistributionScore(shape, 1024, 0, pr, device=self.device) if thresholds is None else None
                thr = (torch.zeros((self.C, len(pr)), dtype=torch.float32, device=self.device) if thresholds is None
                       else thresholds)
                fs = FractionsSkillScore(shape, thr, sc, device=self.device)
                gs = GradientScore(shape, (1.0, 1.0), True, device=self.device) if on == "gradient" else None
                made[name] = (gs, ds, fs)
            self._fss[key] = made
        images, losses = self.score(hr_region)
        hr = hr_region.contiguous()
        out = {}
        for name, (gs, ds, fs) in self._fss[key].items():
            a, b = images[name], hr
            if gs is not None:
                g = gs.measure(a, b)
                a, b = g["gmag_pred"], g["gmag_truth"]
            if ds is not None:
                fs.thresholds.copy_(ds.measure(a, b)["q_truth"])
            res = dict(fs.measure(a, b))
            res["thresholds"] = fs.thresholds
            out[name] = res
        return images, losses, out

    def score_ensemble(self, hr_region: torch.Tensor, edges=None,
                       probs=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9), crps_map: bool = False):
        """``score``, then the ensemble score (srmi.ensemble_score.EnsembleScore) of 'members'
        against hr_region: (images, losses, result), result the dict of EnsembleScore.measure --
        per channel the exact tables 'used', 'rank_hist', 'tied', 'bin_count', the fp64 'sums',
        and 'crps', 'crps_fair', 'rmse_mean', 'spread_rms', 'ssr', 'spread_error_corr',
        'outliers', 'outliers_expected', 'reliability_index', the reliability table 'bin_spread'
        / 'bin_rmse' over the spread bins, 'edges' [C, B - 1] fp32, the ones used, and with
        crps_map=True 'crps_map' [C, s h, s w].  It needs members=True: ValueError otherwise.

        edges: the interior edges of the spread bins -- B - 1 floats (the same for every
        channel), a [C, B - 1] array or a [C, B - 1] fp32 device tensor (kept by reference).
        None: the quantiles of 'spread' at ``probs`` (1 .. 15 probabilities), taken on the device
        from a srmi.distribution.DistributionScore (1024 bins) of 'spread' and cast to fp32 on
        the device -- no host read -- so that the bins hold about equal numbers of pixels.

        What is scored are the members, the raw blended outputs: on a resolver with a
        quantile_map or consistent=K the rmse_mean here is that of the members' own mean, not of
        the mapped or corrected 'model' (scoring those is out of scope).

        images and losses are ``score``'s, bit for bit; the entries are views valid until the
        next call with the same arguments.  No host synchronisation.  With graph=True the score
        is measured after the replay, outside the captured graph.

        land=True: the NaN of the members and of hr_region are the mask, pixel by pixel ('used'
        is what is left)."""
        from .distribution import DistributionScore
        from .ensemble_score import MAX_BINS, EnsembleScore
        if not self.members:
            raise ValueError("score_ensemble needs the member fields: build the resolver with members=True (and "
                             "ensemble > 1)")
        s = self.s
        shape = (self.C, self.h * s, self.w * s)
        if tuple(hr_region.shape) != shape:
            raise ValueError(f"region shape {tuple(hr_region.shape)} != {shape}")
        if edges is None:
            pr = tuple(float(p) for p in probs)
            if not 1 <= len(pr) <= MAX_BINS - 1:
                raise ValueError(f"probs {probs!r}: 1 .. {MAX_BINS - 1} probabilities strictly inside (0, 1)")
            ekey = None
        elif isinstance(edges, torch.Tensor):
            pr, ekey = (), ("tensor", edges.data_ptr(), tuple(edges.shape))
        else:
            import numpy as np
            pr, ekey = (), tuple(np.asarray(edges, dtype=np.float32).reshape(-1).tolist())
        key = (ekey, pr, bool(crps_map))
        if key not in self._ens:  # before the region is inferred: the constructors refuse bad arguments
            ds = DistributionScore(shape, 1024, 0, pr, device=self.device) if edges is None else None
            ed = torch.zeros((self.C, len(pr)), dtype=torch.float32, device=self.device) if edges is None else edges
            self._ens[key] = (ds, EnsembleScore((self.K,) + shape, ed, bool(crps_map), device=self.device))
        images, losses = self.score(hr_region)
        hr = hr_region.contiguous()
        ds, es = self._ens[key]
        if ds is not None:
            es.edges.copy_(ds.measure(images["spread"], images["spread"])["q_truth"])
        return images, losses, es.measure(images["members"], hr)

    def fit_quantile_map(self, hr_regions, bins: int = 256, on: str = "detail", value_range=None,
                         tail_count: int = 16):
        """Calibrate a srmi.quantile_map.QuantileMap on regions whose truth is known:
        hr_regions, a sequence of [C, s h, s w] fp32 device tensors (NaN allowed: a pixel
        counts where both binned values are finite).  Each is downsampled whole by
        task.downsample_mode and super-resolved as ``score`` does, eagerly and with NO map
        applied -- and, a deliberate step away from ``score``'s path on a resolver with
        consistent=K, WITHOUT the consistency correction, because the map is applied to the
        blended field before it and must be calibrated on what it will see -- then accumulated as (src 'model', truth hr_region, base
        'interpolated'); the fitted map is returned, ready for RegionSuperResolver(...,
        quantile_map=).  This object's own quantile_map, if any, is neither used nor changed.

        value_range: one (lo, hi) pair or one per channel; None takes each channel's
        NaN-aware min and max of the FIRST region's truth values (on="value") or truth detail,
        hr_region - 'interpolated' (on="detail"), with torch -- a host read, at fit time
        only.  Later regions that leave it land in the outer entries and map by the constant
        shifts.  bins, on, tail_count: as QuantileMap takes them.

        Out of scope: srmi.inference.TiledInference, training through the map, and a map
        that varies in space or with the season."""
        from .quantile_map import MODES, QuantileMap
        if on not in MODES:
            raise ValueError(f"on {on!r}: one of {MODES}")
        regions = list(hr_regions)
        if not regions:
            raise ValueError("fit_quantile_map needs at least one region")
        s, qm = self.s, None
        for hr_region in regions:
            if tuple(hr_region.shape) != (self.C, self.h * s, self.w * s):
                raise ValueError(f"region shape {tuple(hr_region.shape)} != {(self.C, self.h * s, self.w * s)}")
            hr = hr_region.contiguous()
            self.region.copy_(downsample(hr[None], s, mode=self.dmode)[0])
            self._run(use_map=False, correct=False)
            model, interp = self.images["model"], self.images["interpolated"]
            if qm is None:
                if value_range is None:
                    t = hr - interp if on == "detail" else hr
                    t = t.reshape(self.C, -1)
                    fin = torch.isfinite(t)
                    lo = torch.where(fin, t, torch.full_like(t, float("inf"))).amin(1)
                    hi = torch.where(fin, t, torch.full_like(t, float("-inf"))).amax(1)
                    value_range = torch.stack([lo, hi], 1).cpu().numpy()
                qm = QuantileMap(self.C, value_range, bins=bins, on=on, tail_count=tail_count, device=self.device)
            qm.accumulate(model, hr, interp if on == "detail" else None)
        qm.fit()
        return qm

    def set_params(self, params: torch.Tensor) -> None:
        """Load new weights: copied into the parameter buffer the engines (and the
        captured graph) read, filter packs rebuilt."""
        self.params.copy_(params)
        for e in self.engs:
            e.pack(self.params)
