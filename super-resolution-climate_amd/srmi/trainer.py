"""Fused training step on the native engine.

Restates one iteration of ModelTrainer.train (sres/controller/dual_trainer.py:310-323)
with apply_network (:557-571) for the RCAN/EDSR plugins:

    HR tile batch -> bicubic 1/s (array.py:72-76) -> network -> loss
    [-> interp-baseline loss metric, dual_trainer.py:315-318]
    -> backward -> Adam (lr = task.lr, weight_decay = task.weight_decay or 0)

The loss is model.loss_fn (single_product_loss, dual_trainer.py:205-212): 'l2' =
RMSE (l2loss, stats.py:5-8), 'charbonnier' = mean(sqrt(d^2 + 1e-6)) (:196-198);
anything else raises, as the reference does.

Everything runs asynchronously on one HIP stream: the per-step losses stay on
the device (no .item() sync) until the caller asks for them.
With a DistInfo of world > 1 the batch is this rank's shard and the loss /
gradients are all-reduced as described in srmi/dist.py.
"""
from __future__ import annotations

import math
from typing import Dict, Mapping, Optional, Tuple

import torch

from . import checkpoint as ckpt
from ._lib import SRMI_LOSS_MEAN, SRMI_LOSS_RMSE, TILE_LOSS_SUB, call, ptr
from .config import check_fused_task, data_downsample_factor, interp_mode
from .dist import DistInfo, GradReducer, allreduce_sum_
from .engine import (Engine, NetSpec, adam_step, adam_step_guarded, axpy, downsample, engine_stream, grad_norm,
                     grad_norm_workspace, interp_size, upsample)
from .consistency import ConsistencyLayer
from .optim import check_clip_norm, check_ema, check_guard, ema_decay_at, make_lr_schedule
from .spectra import SpectralLoss
from .gradient import GradientLoss
from .ssim import SSIMLoss
from .superres import check_consistent

LOSS_KINDS = {"l2": SRMI_LOSS_RMSE, "charbonnier": SRMI_LOSS_MEAN}
CHARBONNIER_EPS = 1e-6  # ModelTrainer.eps, sres/controller/dual_trainer.py:122


def _term_config(cls, cfg, hr_hw) -> Optional[Dict[str, object]]:
    """The checked configuration of the loss term ``cls`` (a srmi.loss_term.LossTerm) given to
    FusedTrainer as ``<name>=cfg``, None for None; a missing key takes the term's default.
    ValueError for what is not a dict, an unknown key, a value the term refuses, or a window
    larger than the HR tile -- in this order, and before anything is allocated."""
    if cfg is None:
        return None
    if not isinstance(cfg, Mapping):
        raise ValueError(f"{cls.name}: a dict({', '.join(f'{k}=' for k in cls.DEFAULTS)}) or None, got {cfg!r}")
    extra = set(cfg) - set(cls.DEFAULTS)
    if extra:
        raise ValueError(f"{cls.name}: unknown keys {sorted(extra)}")
    cfg = cls.check_config(**{**cls.DEFAULTS, **cfg})
    window = cfg.get("window", cls.window)
    if window > min(hr_hw):
        raise ValueError(f"{cls.name} loss window {window} larger than the HR tile {tuple(hr_hw)}")
    return cfg


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def default_init_(flat: torch.Tensor, table, seed: int = 0) -> None:
    """PyTorch's default Conv2d init distribution, U(+-1/sqrt(fan_in)), seeded."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    host = torch.empty(flat.numel(), dtype=torch.float32)
    shapes = {nm: s for nm, _, _, s in table}
    for name, off, n, shape in table:
        ws = shape if name.endswith("weight") else shapes[name[:-4] + "weight"]
        b = 1.0 / math.sqrt(float(math.prod(ws[1:])))
        host[off:off + n].uniform_(-b, b, generator=g)
    flat.copy_(host)


class FusedTrainer:
    """One training step = dual_trainer.py:310-323 on the native engine.

    micro > 1 splits the batch into `micro` equal micro-batches, each with its own
    engine (workspace, filter packs, side stream) on its own HIP stream, launches
    sized for 1/micro of the chip (cu_budget).  RCAN/EDSR have no coupling between
    tiles except the loss scale and the gradient sum, so the step is exact: the
    micro-batches' squared-error partials are added before the RMSE is finalised
    (one global L, as with data parallelism) and their gradients are summed before
    the all-reduce / Adam.  The two streams overlap each layer's launch ramp and
    drain with the other micro-batch's work.
    """

    def __init__(self, spec: NetSpec, batch: int, lr_hw=(48, 48), lr: float = 1e-4, betas=(0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0, interp_loss: bool = True,
                 info: Optional[DistInfo] = None, device: Optional[torch.device] = None, seed: int = 0,
                 params: Optional[torch.Tensor] = None, micro: Optional[int] = None, loss_fn: str = "l2",
                 cu_budget: Optional[int] = None, task=None, dp_reducer_stream: bool = False,
                 land: bool = False, spectral: Optional[Mapping] = None, consistent: int = 0,
                 clip_norm: Optional[float] = None, guard: Optional[bool] = None, ema: Optional[Mapping] = None,
                 lr_schedule=None, ssim: Optional[Mapping] = None, gradient: Optional[Mapping] = None):
        """task: the task config section (default: the active srmi ConfigContext's,
        if any).  apply_network's target selection is followed: when
        task.target_variables names fewer channels than the input, the loss target is
        those HR channels (index_select in the input's order, dual_trainer.py:564-568)
        and the model has that many output channels.  task.data_downsample = ds > 1
        downsamples every HR batch by ds first, as apply_network does (:561-563):
        step() then takes tiles T with floor(T / ds) = lr_hw * scale.
        dp_reducer_stream (data parallel, A/B): the gradient all-reduce on a reducer
        stream of its own that waits for each residual group's event of the whole
        enqueued backward, instead of (the default) enqueuing the backward stage by stage
        with each bucket's all-reduce behind its stage on an engine stream.
        task.downsample_mode / upsample_mode select the resampling of the model input
        and of the interp baseline ('cubic' -> bicubic, 'linear' -> bilinear,
        array.py:37-41; others raise).
        land (no reference counterpart; DESIGN.md §1 "Land in training"): step() takes HR
        tiles whose NaN are the land mask.  The LR input is formed as always and then
        flood-filled in place (srmi_tiles_fill), the loss and the interp metric are taken
        over the elements where prediction and target are both finite
        (srmi_tile_loss_parts_masked, the count summed on the device), and the backward
        runs from an upstream gradient that is zero on land (srmi_loss_dy_masked) for
        both loss functions.  Refused with task.data_downsample > 1.
        spectral (no reference counterpart; DESIGN.md §1 "Spectral loss"): None, or the
        configuration of a spectral loss term, dict(weight=1.0, window=64, stride=32,
        eps=1e-12) (srmi.spectra.SpectralLoss's arguments; a missing key takes that
        default).  The step's loss is then loss_fn + weight * L_spec, L_spec the windowed
        Fourier amplitudes of sr - target over the global batch, and the backward runs from
        the sum of both upstream gradients.  Windows that touch a non-finite pixel are
        skipped, so land=True needs nothing more.  A bad window, stride, weight (finite,
        >= 0) or eps raises ValueError here.
        ssim (no reference counterpart; DESIGN.md §1 "SSIM loss"): None, or the configuration
        of an SSIM loss term, dict(weight=1.0, data_range=None) (srmi.ssim.SSIMLoss's
        arguments; a missing key takes that default).  The step's loss is then loss_fn (+
        the spectral term) + weight * L_ssim, L_ssim = 1 - the mean of SSIMScore's ssim over
        the used positions of the global batch (data_range None: every target plane's own
        range), and its gradient is added to the upstream gradient after the spectral term's.
        Positions whose window touches a non-finite pixel are not used, so land=True needs
        nothing more.  Unknown keys, a bad weight (finite, >= 0) or range, or an HR tile below
        11 pixels (the window) in either dimension raise ValueError here.
        gradient (no reference counterpart; DESIGN.md §1 "Gradient loss"): None, or the
        configuration of a gradient loss term, dict(weight=1.0, eps=1e-6)
        (srmi.gradient.GradientLoss's arguments; a missing key takes that default).  The
        step's loss is then loss_fn (+ the spectral term) (+ the SSIM term) + weight * L_grad,
        L_grad the mean over the used positions of the global batch of sqrt(Gx[e]^2 + Gy[e]^2 +
        eps), e = sr - target and Gx, Gy the Sobel derivative at unit scale; its gradient is
        added to the upstream gradient after the SSIM term's and before the consistency
        layer's adjoint.  Positions whose 3 x 3 window touches a non-finite pixel are not
        used, so land=True needs nothing more.  A non-dict, unknown keys, a bad weight
        (finite, >= 0) or eps (finite, > 0), or an HR tile below 3 pixels in either dimension
        raise ValueError here.  step() then also returns "pixel_loss" and "gradient_loss".
        consistent (no reference counterpart; DESIGN.md §1 "Consistency in training"): K in
        0 .. 16.  K > 0 makes K steps of back-projection onto the LR input the model's last,
        parameter-free layer (srmi.consistency.ConsistencyLayer): the network's output is
        corrected in place right after the forward, so the pixel loss, the spectral term and
        ``sr`` see the corrected field, and the upstream gradient goes through the layer's
        adjoint before the engine's backward.  The constraint is imposed against the LR batch
        as downsampled; land=True: as it was BEFORE the flood fill, so a cell whose coarse
        value is NaN is left unconstrained.  It needs nchannels_out == nchannels_in without
        a task.target_variables selection, an even scale (>= 4 under a bicubic downsample)
        and bilinear / bicubic modes: ValueError otherwise, before anything is allocated.
        K is no parameter and is not stored in a checkpoint: pass the same K to
        TiledInference / RegionSuperResolver.  consistent=0 is the trainer as it was.
        clip_norm, guard, ema, lr_schedule (no reference counterpart; DESIGN.md §1 "Optimizer
        guards"; srmi.optim holds the checks and closed forms).  All opt-in: at their defaults
        the step enqueues exactly what it did without them.
        guard: before Adam, srmi_grad_norm takes the L2 norm of the whole-batch gradient
        (self.grads after the micro-batch sum and, data parallel, after the all-reduces: every
        rank derives the same numbers from the same bytes, no further collective) into the
        device record self.ctl = (norm, clip coefficient, finite, skipped count), and Adam is
        srmi_adam_step_guarded: a step whose norm is not finite writes nothing -- params, m, v
        and ema stay bit for bit -- and is counted in ctl[3] (skipped_steps()).  A skipped step
        still consumes its step number: self.t advances and the next step's bias corrections
        are those of t + 1, because the host never reads ctl inside step().  step() then also
        returns "grad_norm" (a view of ctl[0:1]) and "step_skipped" (ctl[2:3]: 0.0 = skipped).
        Default None: on iff clip_norm or ema is set; guard=True alone measures and guards
        without clipping (max_norm = inf).
        clip_norm: None or a finite float > 0, torch.nn.utils.clip_grad_norm_'s max_norm: the
        gradient enters Adam as g * min(1, clip_norm / (norm + 1e-6)), the coefficient read from
        the device by the Adam launch.
        ema: None or dict(decay=0.999, warmup=True): self.ema, a flat fp32 copy of the initial
        params, follows ema += (1 - d_t) (params - ema) inside the Adam launch, d_t =
        min(decay, (1 + t) / (10 + t)) at Adam step t under warm-up, else decay
        (ema_state_dict(), eval_params(ema=True)).  Unknown keys or a decay outside [0, 1):
        ValueError.
        lr_schedule: None, dict(kind="constant" | "step" | "cosine", ...) or a callable
        t0 -> lr (srmi.optim.make_lr_schedule): Adam step t runs at schedule(t - 1), a pure
        function of the step count, so a resume with the same arguments is exact and nothing
        of it is stored; the checkpoint's param_groups[0]["lr"] stays the base rate `lr`."""
        # the optimizer guards' arguments: refused before anything is allocated
        self.clip_norm = check_clip_norm(clip_norm)
        self.ema_cfg = check_ema(ema)
        self.guard = check_guard(guard, self.clip_norm, self.ema_cfg)
        self.lr_schedule = make_lr_schedule(lr_schedule, lr)
        if loss_fn not in LOSS_KINDS:  # single_product_loss, dual_trainer.py:210-211
            raise ValueError(f"Unknown single-product loss function {loss_fn}")
        if task is None:
            from . import config as _config
            task = _config._CURRENT.get("task") if _config._CURRENT is not None else None
        # consistent > 0 (the integer alone is checked here, scale and modes below): the layer
        # compares the output with the input channel by channel, so a target_variables subset
        # (fewer output channels) has no meaning -- said before check_fused_task looks for names
        if check_consistent(consistent, 2, "bilinear", "bilinear") and spec.nchannels_out != spec.nchannels_in:
            raise ValueError(f"consistent={consistent} needs a model whose output channels are its input's (no "
                             f"task.target_variables subset): {spec.nchannels_in} in, {spec.nchannels_out} out")
        tindx = check_fused_task(task, spec.nchannels_in, spec.nchannels_out)
        self.ds = data_downsample_factor(task)
        self.land = bool(land)
        if self.land and self.ds > 1:
            raise ValueError(f"land=True with task.data_downsample={self.ds}: the land mask of a pre-downsampled "
                             "HR batch is not defined (train on tiles of the model's own HR size)")
        self.dmode, self.umode = interp_mode(task, True), interp_mode(task, False)
        self.consistent = check_consistent(consistent, spec.scale, self.dmode, self.umode)
        if tindx is not None and interp_loss and spec.nchannels_out != 1:
            # loss(btarget, upsample(binput)) (:315-317) needs equal or broadcastable channels
            raise ValueError(f"interp loss of a {spec.nchannels_out}-channel target against the "
                             f"{spec.nchannels_in}-channel interpolated input does not broadcast (as in the reference)")
        self.loss_fn = loss_fn
        self.loss_kind = LOSS_KINDS[loss_fn]
        # the configured loss terms in their fixed order: the order of step()'s chain
        hr_hw = (lr_hw[0] * spec.scale, lr_hw[1] * spec.scale)
        term_cfgs = [(cls, _term_config(cls, cfg, hr_hw))
                     for cls, cfg in ((SpectralLoss, spectral), (SSIMLoss, ssim), (GradientLoss, gradient))]
        term_cfgs = [(cls, cfg) for cls, cfg in term_cfgs if cfg is not None]
        self.info = info or DistInfo()
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.tindx = None if tindx is None else torch.tensor(tindx, dtype=torch.long, device=self.device)
        self.spec = spec
        self.batch = batch
        if micro is None:
            micro = 2 if (batch % 2 == 0 and batch >= 16) else 1
        if batch % micro:
            raise ValueError(f"batch {batch} not divisible into {micro} micro-batches")
        self.micro = micro
        self.mb = batch // micro
        # CUs each engine's launches are sized for (0 = the whole chip)
        budget = (256 // micro if micro > 1 else 0) if cu_budget is None else int(cu_budget)
        self.engines = [Engine(spec, self.mb, lr_hw, train=True, device=self.device, cu_budget=budget)
                        for _ in range(micro)]
        self.eng = self.engines[0]
        n = self.eng.n_params
        self.params = torch.empty(n, dtype=torch.float32, device=self.device)
        if params is not None:
            self.params.copy_(params)
        else:
            default_init_(self.params, self.eng.table, seed)
        if self.info.enabled:  # identical replicas (rank 0's weights)
            torch.distributed.broadcast(self.params, 0)
        self.grads = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.mgrads = [self.grads] + [torch.zeros(n, dtype=torch.float32, device=self.device)
                                      for _ in range(micro - 1)]
        self.m = torch.zeros_like(self.grads)
        self.v = torch.zeros_like(self.grads)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.t = 0
        # the guards' control record (norm, coefficient, finite, skipped), the norm's partials
        # and the averaged weights; none of them exists with the guards off
        self.ctl = torch.zeros(4, dtype=torch.float32, device=self.device) if self.guard else None
        self.norm_ws = (torch.empty(grad_norm_workspace(n), dtype=torch.uint8, device=self.device)
                        if self.guard else None)
        self.ema = self.params.clone() if self.ema_cfg is not None else None
        self.interp_loss = interp_loss
        C, h, w, s = spec.nchannels_in, lr_hw[0], lr_hw[1], spec.scale
        self.lrbuf = torch.empty((batch, C, h, w), dtype=torch.float32, device=self.device)
        self.sr = torch.empty((batch, spec.nchannels_out, h * s, w * s), dtype=torch.float32, device=self.device)
        self.up = (torch.empty((batch, C, h * s, w * s), dtype=torch.float32, device=self.device)
                   if interp_loss else None)
        # Charbonnier: the elementwise loss gradient is the backward's upstream gradient
        # (land: for the RMSE too -- zero on land, srmi_loss_dy_masked)
        # (a loss term: always -- its gradient is added to the pixel loss's)
        # (a consistency layer: always -- its adjoint runs on it)
        self.dy = (torch.empty_like(self.sr)
                   if self.loss_kind == SRMI_LOSS_MEAN or self.land or term_cfgs or self.consistent else None)
        # the consistency layer and, with land, the LR batch as it was before the flood fill
        self.layer = (ConsistencyLayer((batch, C, h, w), s, self.umode, self.dmode, self.consistent, self.device)
                      if self.consistent else None)
        self.lr_raw = torch.empty_like(self.lrbuf) if self.consistent and self.land else None
        # the selected target channels (index_select) and, for the interp metric, that
        # target broadcast over the input's channels (1-channel target, :316-317)
        self.tgt = torch.empty_like(self.sr) if self.tindx is not None else None
        self.tgt_b = (torch.empty((batch, C, h * s, w * s), dtype=torch.float32, device=self.device)
                      if self.tindx is not None and interp_loss else None)
        # apply_network's data_downsample: the HR batch downsampled by ds first
        self.hrds = (torch.empty((batch, C, h * s, w * s), dtype=torch.float32, device=self.device)
                     if self.ds > 1 else None)
        self.loss4 = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.iloss4 = torch.zeros(4, dtype=torch.float32, device=self.device)
        # the loss sums as per-tile parts (srmi_tile_loss_parts) of the GLOBAL batch, in
        # global tile order: [loss parts | interp parts] of the step's gb tiles.  The
        # step's loss -- and the gradient scale 1/(count L) -- then depends neither on the
        # micro-batch split nor, data parallel, on how the batch is sharded over ranks:
        # every rank writes its tiles' parts into a zeroed array, one SUM all-reduce
        # (x + 0 is exact) hands every rank all of them, and every rank sums them in the
        # order one process would.
        self.gcap = batch * self.info.world
        # land: the counts of the finite elements ride behind them, [loss | interp] again,
        # through the same single all-reduce (whole numbers: x + 0 and their sums are exact)
        self.gparts = torch.zeros((4 if self.land else 2) * self.gcap * TILE_LOSS_SUB, dtype=torch.float32,
                                  device=self.device)
        # the loss terms: each owns a workspace for this rank's tiles (the spectral term's
        # gradient windows, the SSIM term's coefficient maps, the gradient term's partial sums)
        # and the per-plane parts and used counts of the GLOBAL batch, which travel as gparts does
        self.terms = [cls(tuple(self.sr.shape), device=self.device, global_batch=self.gcap, **cfg)
                      for cls, cfg in term_cfgs]
        by_name = {t.name: t for t in self.terms}
        self.spectral, self.ssim, self.gradient = (by_name.get(n) for n in ("spectral", "ssim", "gradient"))
        self.streams = [None] + [engine_stream(self.device) for _ in range(micro - 1)]
        self.dp_staged = not dp_reducer_stream
        self.reducer = GradReducer(self.eng.table, spec.arch, spec.nlayers, self.info, self.device,
                                   stream=self.info.enabled and not self.dp_staged)
        # group events of engines 1.. (engine 0 records into reducer.events)
        self.xevents = [self.reducer.new_events() for _ in range(micro - 1)]
        # staged DP backward: the stages, the buckets final after each, and per engine
        # (but the last, which reduces) an event per stage
        self.nstages = self.eng.stage_count if self.info.enabled and self.dp_staged else 0
        self.stage_buckets = self.reducer.stage_buckets(self.nstages) if self.nstages else []
        self.stage_ev = ([[torch.cuda.Event() for _ in range(self.nstages)] for _ in range(micro - 1)]
                         if self.nstages and self.device.type == "cuda" else [])
        for e in self.engines:
            e.pack(self.params)

    def _ctx(self, k):
        st = self.streams[k]
        return torch.cuda.stream(st) if st is not None else _Null()

    def _loss_parts(self, pred, target, parts, t0, cparts=None):
        """This micro-batch's tiles' loss parts (rows t0.. of the batch-wide parts array);
        land: over the finite elements, their counts into the same rows of cparts."""
        nt = pred.shape[0]
        te = pred[0].numel()
        if cparts is not None:
            call("srmi_tile_loss_parts_masked", ptr(pred), ptr(target), nt, te, self.loss_kind, CHARBONNIER_EPS,
                 ptr(parts[t0 * TILE_LOSS_SUB:]), ptr(cparts[t0 * TILE_LOSS_SUB:]),
                 torch.cuda.current_stream(self.device).cuda_stream)
            return
        call("srmi_tile_loss_parts", ptr(pred), ptr(target), nt, te, self.loss_kind, CHARBONNIER_EPS,
             ptr(parts[t0 * TILE_LOSS_SUB:]), torch.cuda.current_stream(self.device).cuda_stream)

    def _reduce_losses(self, gb, count, icount):
        """loss4 / iloss4 of the whole (global) batch from its gb tiles' parts in tile
        order, finalised (data parallel: after the all-reduce of the parts)."""
        st = torch.cuda.current_stream(self.device).cuda_stream
        n = gb * TILE_LOSS_SUB
        if self.land:  # [loss | interp] parts, then [loss | interp] counts; the count is the device's
            m = 2 if self.interp_loss else 1
            if self.info.enabled:
                allreduce_sum_(self.gparts[:2 * m * n], self.info)
            call("srmi_loss_from_parts_masked", ptr(self.gparts), ptr(self.gparts[m * n:]), gb, self.loss_kind,
                 ptr(self.loss4), st)
            if self.interp_loss:
                call("srmi_loss_from_parts_masked", ptr(self.gparts[n:]), ptr(self.gparts[m * n + n:]), gb,
                     self.loss_kind, ptr(self.iloss4), st)
            return
        if self.info.enabled:
            allreduce_sum_(self.gparts[:2 * n if self.interp_loss else n], self.info)
        call("srmi_loss_from_parts", ptr(self.gparts), gb, float(count), self.loss_kind, ptr(self.loss4), st)
        if self.interp_loss:
            call("srmi_loss_from_parts", ptr(self.gparts[n:]), gb, float(icount), self.loss_kind, ptr(self.iloss4),
                 st)

    def _shard(self, b: int, shard: Optional[Tuple[int, int]]) -> Tuple[int, int]:
        """(t0, gb): this call's tiles are tiles t0 .. t0 + b - 1 of a gb-tile global
        batch.  Default: the whole batch (one process) or, data parallel, equal shards
        in rank order."""
        if shard is None:
            return (self.info.rank * b, self.info.world * b) if self.info.enabled else (0, b)
        t0, gb = int(shard[0]), int(shard[1])
        if not self.info.enabled and (t0, gb) != (0, b):
            raise ValueError(f"shard {shard} of a {b}-tile batch without data parallelism")
        if t0 < 0 or t0 + b > gb or gb < 1 or gb > self.gcap:
            raise ValueError(f"shard {shard} of {b} tiles outside a global batch of 1..{self.gcap} tiles")
        return t0, gb

    def step(self, hr: torch.Tensor, shard: Optional[Tuple[int, int]] = None) -> Dict[str, torch.Tensor]:
        """hr: this rank's HR tiles [b, C, H, W] fp32 on the device (already normalised;
        land=True: NaN on land),
        b <= the trainer's batch (a short last batch of a time slice, as the
        reference's TileBatchIterator yields, sres/data/tiles.py:55-72).

        Data parallel, shard = (t0, gb): hr holds tiles t0 .. t0 + b - 1 of the step's
        gb-tile global batch (srmi.dist.shard_range; a rank of a short last batch may
        hold none, b = 0, and still takes part in every collective and the Adam step);
        the default is equal shards in rank order."""
        b = hr.shape[0]
        if b < (0 if self.info.enabled else 1) or b > self.batch:
            raise ValueError(f"batch {b} outside {0 if self.info.enabled else 1}..{self.batch}")
        t0, gb = self._shard(b, shard)
        s = self.spec.scale
        if self.ds > 1 and b:  # apply_network: downsample(input, scale_factor=ds) first (:561-563)
            got = tuple(interp_size(n, 1.0 / self.ds) for n in hr.shape[2:])
            if got != tuple(self.hrds.shape[2:]):
                raise ValueError(f"data_downsample={self.ds}: HR tiles {tuple(hr.shape[2:])} give {got}, "
                                 f"expected {tuple(self.hrds.shape[2:])}")
            hr = downsample(hr, self.ds, out=self.hrds[:b], mode=self.dmode)
        mb = (b + self.micro - 1) // self.micro
        sls = [slice(min(b, k * mb), min(b, (k + 1) * mb)) for k in range(self.micro)]
        main = torch.cuda.current_stream(self.device)
        if self.tindx is not None and b:  # apply_network's index_select of the target channels
            tgt = torch.index_select(hr, 1, self.tindx, out=self.tgt[:b])
            if self.tgt_b is not None:
                self.tgt_b[:b].copy_(tgt.expand(-1, hr.shape[1], -1, -1))
        else:
            tgt = hr
        # element counts of the global batch: target tiles (Co x HR) and interp tiles (C x HR)
        count = float(gb) * self.sr[0].numel()
        icount = float(gb) * self.lrbuf[0].numel() * s * s
        n = gb * TILE_LOSS_SUB
        lparts, iparts = self.gparts[:n], self.gparts[n:2 * n]
        lcparts = icparts = None
        if self.land:
            # [loss | interp | loss counts | interp counts] of n each; without the interp
            # metric [loss | loss counts]: iparts above then overlaps lcparts and is not used
            m = 2 if self.interp_loss else 1
            lcparts, icparts = self.gparts[m * n:m * n + n], self.gparts[m * n + n:m * n + 2 * n]
        if self.info.enabled:  # the other ranks' tiles' parts stay 0 here
            self.gparts[:(4 if self.land else 2) * n].zero_()
        for term in self.terms:
            term.set_global_batch(gb)
            if self.info.enabled:
                for v in term.views():
                    v.zero_()
        for st in self.streams[1:]:
            st.wait_stream(main)
        # forward + loss partials per micro-batch (an empty micro-batch adds nothing)
        for k, eng in enumerate(self.engines):
            sl = sls[k]
            if sl.stop == sl.start:
                continue
            with self._ctx(k):
                downsample(hr[sl], s, out=self.lrbuf[sl], mode=self.dmode)
                if self.land:  # an LR pixel is NaN iff one of its taps is dry: fill, as inference does
                    lrs = self.lrbuf[sl]
                    if self.lr_raw is not None:
                        self.lr_raw[sl].copy_(lrs)
                    call("srmi_tiles_fill", ptr(lrs), lrs.shape[0] * lrs.shape[1], lrs.shape[2], lrs.shape[3], None,
                         torch.cuda.current_stream(self.device).cuda_stream)
                eng.forward(self.params, self.lrbuf[sl], out=self.sr[sl])
                if self.layer is not None:  # the last layer: sr corrected in place
                    self.layer.forward_(self.sr[sl], (self.lrbuf if self.lr_raw is None else self.lr_raw)[sl],
                                        rows=sl.start)
                if self.dy is not None and not self.land:  # Charbonnier: the elementwise upstream gradient only
                    eng.charbonnier_partial(self.sr[sl], tgt[sl], None, count, CHARBONNIER_EPS, dy=self.dy[sl])
                self._loss_parts(self.sr[sl], tgt[sl], lparts, t0 + sl.start, lcparts)
                for term in self.terms:
                    term.parts(self.sr[sl], tgt[sl], rows=sl.start, global_row=t0 + sl.start)
                if self.interp_loss:  # self.loss(btarget, binterp), dual_trainer.py:316-317
                    up = upsample(self.lrbuf[sl], s, out=self.up[sl], mode=self.umode)
                    itgt = hr[sl] if self.tgt_b is None else self.tgt_b[sl]
                    self._loss_parts(itgt, up, iparts, t0 + sl.start, icparts)
        for st in self.streams[1:]:
            main.wait_stream(st)
        self._reduce_losses(gb, count, icount)
        # each term and its scale from the global batch's parts and counts, chained: a term's
        # total is the pixel loss + the terms before it + its own
        prev = self.loss4[3:4] if self.terms else None
        for term in self.terms:
            if self.info.enabled:
                allreduce_sum_(term.gparts[:2 * gb * term.C], self.info)
            term.finalize(prev)
            prev = term.total
        for st in self.streams[1:]:
            st.wait_stream(main)
        # the upstream gradient from the finalised loss, zero on land; with a loss term or a
        # consistency layer the RMSE's too ((p - t) * loss4[2], what the tail kernels form), then
        # the terms' on top
        explicit = bool(self.terms) or self.layer is not None
        if self.land or (explicit and self.loss_kind == SRMI_LOSS_RMSE):
            for k in range(self.micro):
                sl = sls[k]
                if sl.stop > sl.start:
                    with self._ctx(k):
                        call("srmi_loss_dy_masked", ptr(self.sr[sl]), ptr(tgt[sl]), self.sr[sl].numel(),
                             self.loss_kind, CHARBONNIER_EPS, ptr(self.loss4), ptr(self.dy[sl]),
                             torch.cuda.current_stream(self.device).cuda_stream)
        for term in self.terms:
            for k in range(self.micro):
                sl = sls[k]
                if sl.stop > sl.start:
                    with self._ctx(k):
                        term.add_dy(self.dy[sl], self.sr[sl], tgt[sl], rows=sl.start)
        if self.layer is not None:  # through the layer's adjoint: dy becomes the network output's gradient
            for k in range(self.micro):
                sl = sls[k]
                if sl.stop > sl.start:
                    with self._ctx(k):
                        self.layer.backward_(self.dy[sl], rows=sl.start)
        # backward per micro-batch with the global loss scale.  Data parallel: the
        # engines' gradients are added and all-reduced bucket by bucket as soon as every
        # engine is past the bucket, overlapped with the rest of backward
        # (_backward_dp_staged, or the reducer stream waiting on the engines' residual-group events).
        dp = self.info.enabled and self.reducer.cuda
        if dp and self.dp_staged:
            self._backward_dp_staged(sls, tgt)
            return self._finish_step(main)
        evs = [self.reducer.events] + self.xevents if dp else [None] * self.micro
        for k, eng in enumerate(self.engines):
            sl = sls[k]
            with self._ctx(k):
                if sl.stop == sl.start:  # no tiles: zero gradient (and its group events)
                    self.mgrads[k].zero_()
                    if evs[k] is not None:
                        for ev in evs[k]:
                            ev.record()
                    continue
                if self.dy is not None:
                    eng.backward(self.params, self.lrbuf[sl], self.mgrads[k], dy=self.dy[sl], events=evs[k])
                else:
                    eng.backward(self.params, self.lrbuf[sl], self.mgrads[k], sr=self.sr[sl], hr=tgt[sl],
                                 loss4=self.loss4, events=evs[k])
        for st in self.streams[1:]:
            main.wait_stream(st)
        if dp:
            self.reducer.reduce(self.grads, events_recorded=True, extra=self.mgrads[1:], extra_events=self.xevents)
        else:
            for g in self.mgrads[1:]:
                axpy(self.grads, g, 1.0)  # exact gradient of the whole batch
        return self._finish_step(main)

    def _backward_dp_staged(self, sls, tgt):
        """Data-parallel backward without a reducer stream: with two micro-batch engines
        a rank runs 3 streams (the engines' and RCCL's) instead of 4.  The engines'
        backward is enqueued stage by stage (srmi_backward_stages: tail / upsamplers,
        each residual group, head); behind the stage that finalises a bucket, the LAST
        engine's stream waits for the other engines' events of that stage, adds their
        gradients into engine 0's (the exact whole-batch gradient) and launches the
        bucket's asynchronous all-reduce.  RCCL's stream waits for that point; no engine
        stream waits for RCCL until Adam."""
        red_k = self.micro - 1
        works = []
        for s in range(self.nstages):
            for k, eng in enumerate(self.engines):
                sl = sls[k]
                with self._ctx(k):
                    if sl.stop == sl.start:  # no tiles: a zero gradient
                        if s == 0:
                            self.mgrads[k].zero_()
                    elif self.dy is not None:
                        eng.backward(self.params, self.lrbuf[sl], self.mgrads[k], dy=self.dy[sl], stages=(s, s))
                    else:
                        eng.backward(self.params, self.lrbuf[sl], self.mgrads[k], sr=self.sr[sl], hr=tgt[sl],
                                     loss4=self.loss4, stages=(s, s))
                    if k != red_k:
                        self.stage_ev[k][s].record()
            if self.stage_buckets[s]:
                with self._ctx(red_k):
                    cur = torch.cuda.current_stream(self.device)
                    for k in range(self.micro):
                        if k != red_k:
                            cur.wait_event(self.stage_ev[k][s])
                    self.reducer.reduce_stage(self.stage_buckets[s], self.grads, self.mgrads[1:], works)
        for w in works:
            w.wait()  # the current (main) stream waits for the all-reduces

    def _finish_step(self, main):
        for st in self.streams[1:]:
            main.wait_stream(st)
        self.t += 1
        lr = self.lr if self.lr_schedule is None else float(self.lr_schedule(self.t - 1))
        if self.guard:  # norm -> ctl on the device -> the guarded step reads it there: no host read
            grad_norm(self.grads, self.ctl, math.inf if self.clip_norm is None else self.clip_norm, self.norm_ws)
            adam_step_guarded(self.params, self.grads, self.m, self.v, self.ctl, self.t, lr, self.betas, self.eps,
                              self.wd, ema=self.ema,
                              ema_decay=ema_decay_at(self.ema_cfg, self.t) if self.ema is not None else 0.0)
        else:
            adam_step(self.params, self.grads, self.m, self.v, self.t, lr, self.betas, self.eps, self.wd)
        for k, eng in enumerate(self.engines):
            if k:
                self.streams[k].wait_stream(main)
            with self._ctx(k):
                eng.pack(self.params)
        for st in self.streams[1:]:
            main.wait_stream(st)
        out = {"loss": self.loss4[3:4], "interp_loss": self.iloss4[3:4]}
        if self.terms:  # the last term's total is the step's loss
            out.update(loss=self.terms[-1].total, pixel_loss=self.loss4[3:4])
            out.update({f"{term.name}_loss": term.term4[3:4] for term in self.terms})
        if self.guard:
            out["grad_norm"] = self.ctl[0:1]
            out["step_skipped"] = self.ctl[2:3]
        return out

    def current_lr(self) -> float:
        """The learning rate the next step will use: schedule(t), the base rate without one."""
        return self.lr if self.lr_schedule is None else float(self.lr_schedule(self.t))

    def skipped_steps(self) -> int:
        """Steps skipped so far for a non-finite gradient norm (ctl[3]).  One host
        synchronisation: the caller's to take, outside step().  0 with the guard off."""
        return int(self.ctl[3].item()) if self.guard else 0

    def eval_params(self, ema: bool = False) -> torch.Tensor:
        """The flat device buffer a TiledInference / RegionSuperResolver packs from: the
        averaged weights (ema=True; ValueError on a trainer without them) or the last iterate."""
        if ema and self.ema is None:
            raise ValueError("eval_params(ema=True) on a trainer built without ema=")
        return self.ema if ema else self.params

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """Reference-format state_dict of the averaged weights (CPU copies)."""
        if self.ema is None:
            raise ValueError("ema_state_dict() on a trainer built without ema=")
        return ckpt.model_state_dict(self.ema, self.eng.table)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Reference-format model state_dict (CPU copies)."""
        return ckpt.model_state_dict(self.params, self.eng.table)

    def checkpoint(self, epoch: int = 0, itime: int = 0, loss: float = 0.0) -> Dict:
        """What CheckpointManager.save_checkpoint writes (checkpoints.py:18-26): model
        and torch.optim.Adam state dicts in the reference's layouts.  param_groups[0]["lr"] is
        the BASE rate whatever the schedule.  With the guard on, two more top-level keys, which
        the reference's loader never looks at: srmi_optimizer = dict(skipped, ema_decay,
        ema_warmup) and, with ema, ema_state_dict in model_state_dict's layout."""
        state = ckpt.checkpoint(epoch, itime, self.params, self.eng.table, self.m, self.v, self.t, self.lr,
                                self.betas, self.eps, self.wd, loss)
        if self.guard:
            ckpt.add_optimizer_extras(state, self.eng.table, self.skipped_steps(), self.ema_cfg, self.ema)
        return state

    def load_checkpoint(self, state: Dict) -> None:
        """Resume from a reference-format checkpoint dict (checkpoints.py:35-51,
        update_model=True): weights, Adam moments, step count and hyper-parameters;
        the bf16 filter packs are rebuilt.  The model dict is loaded with FModule's
        strict semantics (common.py:50-71: unexpected or missing keys raise, only a
        re-shaped 'tail' is skipped).  Both dicts are validated into host buffers
        before anything on the device changes, so a failed load leaves the trainer
        as it was -- the averaged weights and the skipped count too: a trainer with ema
        loads ema_state_dict (strict, as the model's) or, from a file without one, starts
        the average at the loaded params; a trainer without ema ignores the key; the count
        comes from srmi_optimizer (0 without it)."""
        host_p = ckpt.load_model_state_dict(self.params, self.eng.table, state["model_state_dict"], strict=True,
                                            apply=False)
        t, hp, mh, vh = ckpt.load_adam_state_dict(self.eng.table, state["optimizer_state_dict"], self.m, self.v,
                                                  apply=False)
        skipped, host_e = ckpt.load_optimizer_extras(self.eng.table, state, host_p, self.ema)
        self.params.copy_(host_p)
        if self.ema is not None:
            self.ema.copy_(host_e)
        if self.guard:
            self.ctl.zero_()
            self.ctl[3] = float(skipped)
        self.m.copy_(mh)
        self.v.copy_(vh)
        self.t = t
        self.lr, self.betas, self.eps, self.wd = hp["lr"], tuple(hp["betas"]), hp["eps"], hp["weight_decay"]
        if self.info.enabled:
            for x in (self.params, self.m, self.v) + ((self.ema,) if self.ema is not None else ()):
                torch.distributed.broadcast(x, 0)
        for e in self.engines:
            e.pack(self.params)
