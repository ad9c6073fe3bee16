"""The consistency correction as the last, parameter-free layer of a model in training and
in tile-wise evaluation (no reference counterpart; DESIGN.md §1 "Consistency in training").

``srmi.superres`` states the correction: K steps of iterative back-projection x <- x + U(lr
- D x), run on LR-size buffers as x_K = x0 + U(R_K), R_K = sum_{k < K} E^k r0 with r0 = M (lr
- D x0) and E = M (I - G), G the clamped D U stencil and M the mask of the active cells (lr
finite, every tap of D finite).  x_K is affine in x0 with Jacobian J = I - U P M D, P = sum_{k
< K} E^k, so a loss gradient g with respect to x_K goes back to x0 as

    q = U^T g;   t_0 = q, t_{k+1} = (I - G^T)(M t_k), Q = sum_{k < K} t_k;   g0 = g - D^T (M Q)

``ConsistencyLayer`` owns the LR-size workspace of both directions and issues the three
launches of each (srmi_consistency_residual / _iterate / _apply and
srmi_consistency_adjoint_gather / _adjoint_iterate / _adjoint_apply), in place, on the current
stream, capturable.  lr takes no gradient.

The layer has no parameters and the checkpoint format does not record K: whoever trains with
``FusedTrainer(consistent=K)`` passes the same K to ``TiledInference(consistent=K)`` (and to
``RegionSuperResolver``, which applies the correction once to the blended region instead of
per tile).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._lib import call, ptr
from .superres import INTERP_MODES, check_consistent


class ConsistencyLayer:
    def __init__(self, shape_lr: Tuple[int, int, int, int], scale: int, umode: str, dmode: str, K: int,
                 device: Optional[torch.device] = None):
        """shape_lr: (N, C, h, w) of the largest LR batch; umode / dmode: 'bilinear' /
        'bicubic', the task's upsample / downsample; K: 1 .. 16 steps (check_consistent's
        refusals; K = 0 is no layer and is refused here)."""
        self.K = check_consistent(K, scale, dmode, umode)
        if self.K < 1:
            raise ValueError("ConsistencyLayer needs K >= 1 (K = 0 is no layer)")
        N, C, h, w = (int(v) for v in shape_lr)
        if min(N, C, h, w) < 1:
            raise ValueError(f"shape_lr {tuple(shape_lr)}: positive (N, C, h, w)")
        self.shape_lr, self.s = (N, C, h, w), int(scale)
        self.um, self.dm = INTERP_MODES[umode], INTERP_MODES[dmode]
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        f32 = dict(dtype=torch.float32, device=self.device)
        self.r0 = torch.zeros((N, C, h, w), **f32)  # M (lr - D x0) of the last forward_
        self.active = torch.zeros((N, C, h, w), dtype=torch.int32, device=self.device)
        self.pp = [torch.zeros((N, C, h, w), **f32) for _ in range(2)]  # ping-pong: r_k, then t_k
        self.R = torch.zeros((N, C, h, w), **f32)  # R_K after forward_, Q after backward_

    def _check(self, x: torch.Tensor, rows: int) -> int:
        N, C, h, w = self.shape_lr
        n = x.shape[0]
        if tuple(x.shape[1:]) != (C, h * self.s, w * self.s) or rows < 0 or rows + n > N:
            raise ValueError(f"HR batch {tuple(x.shape)} at rows {rows} outside the layer's "
                             f"{(N, C, h * self.s, w * self.s)}")
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("the layer works in place on contiguous fp32")
        return n

    def residual_left(self, n: int, rows: int = 0) -> torch.Tensor:
        """E^K r0 = M (lr - D x_K) of the last forward_ on these rows (until backward_, which
        reuses the buffer)."""
        return self.pp[(self.K - 1) % 2][rows:rows + n]

    def forward_(self, x: torch.Tensor, lr: torch.Tensor, rows: int = 0) -> torch.Tensor:
        """x [n, C, h s, w s] <- x + U(R_K) at its finite pixels, lr [n, C, h, w] the LR batch
        (NaN: that cell is inactive).  ``rows``: the workspace rows rows .. rows + n - 1 hold
        this call's state until backward_(dy, rows) -- micro-batches on different streams
        pass their own."""
        n = self._check(x, rows)
        _, C, h, w = self.shape_lr
        if tuple(lr.shape) != (n, C, h, w) or lr.dtype != torch.float32 or not lr.is_contiguous():
            raise ValueError(f"LR batch {tuple(lr.shape)} != {(n, C, h, w)} contiguous fp32")
        if n == 0:
            return x
        st = torch.cuda.current_stream(self.device).cuda_stream
        sl = slice(rows, rows + n)
        act, R = ptr(self.active[sl]), ptr(self.R[sl])
        call("srmi_consistency_residual", ptr(x), ptr(lr), n * C, h, w, self.s, self.dm, ptr(self.r0[sl]), act, st)
        src = self.r0[sl]
        for k in range(self.K):
            dst = self.pp[k % 2][sl]
            call("srmi_consistency_iterate", ptr(src), act, n * C, h, w, self.s, self.um, self.dm, int(k == 0), R,
                 ptr(dst), st)
            src = dst
        call("srmi_consistency_apply", R, n * C, h, w, self.s, self.um, ptr(x), st)
        return x

    def backward_(self, dy: torch.Tensor, rows: int = 0) -> torch.Tensor:
        """dy [n, C, h s, w s], the gradient with respect to forward_'s result, <- J^T dy, the
        gradient with respect to its input, with the active mask forward_ left in these
        rows."""
        n = self._check(dy, rows)
        if n == 0:
            return dy
        _, C, h, w = self.shape_lr
        st = torch.cuda.current_stream(self.device).cuda_stream
        sl = slice(rows, rows + n)
        act, Q = ptr(self.active[sl]), ptr(self.R[sl])
        src = self.pp[0][sl]  # the ping-pong buffers now hold t_k; r0 and active stay
        call("srmi_consistency_adjoint_gather", ptr(dy), n * C, h, w, self.s, self.um, ptr(src), st)
        for k in range(self.K):
            dst = self.pp[(k + 1) % 2][sl]
            call("srmi_consistency_adjoint_iterate", ptr(src), act, n * C, h, w, self.s, self.um, self.dm,
                 int(k == 0), Q, ptr(dst), st)
            src = dst
        call("srmi_consistency_adjoint_apply", Q, act, n * C, h, w, self.s, self.dm, ptr(dy), st)
        return dy
