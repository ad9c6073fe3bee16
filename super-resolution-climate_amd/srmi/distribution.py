"""Distribution score of a super-resolved field: does it have the truth's values?

No reference counterpart -- a deliberate extension, not a parity item.  ``score`` (RMSE)
rewards smooth output, ``srmi.spectra`` says at which wavelengths a field fails and
``srmi.ssim`` where.  Output pulled to the mean also under-fills the tails -- the marine heat
waves, cold filaments and salinity minima a user of a downscaled field looks at first -- and
none of those shows it.  ``DistributionScore`` is the distributional leg of downscaling
evaluation: the histograms of the prediction and of the truth on the truth's range, their
joint histogram, the Perkins skill score (histogram overlap), the Wasserstein-1 distance,
the share of the prediction outside the truth's range, and a set of quantiles whose
difference ``q_bias`` is the tail-compression number.

Definition (``srmi_distribution``, include/srmi.h; tests/distribution_oracle.py restates it)
-------------------------------------------------------------------------------------------
Per channel of a prediction ``a`` and a truth ``b``, [C, H, W]: a pixel is used iff it is
finite in both (NaN is the land mask); ``lo``, ``hi`` are the truth's min and max over the
used pixels unless ``value_range`` is given; the bin of ``x`` is ``1 + min(int((x - lo) *
scale), B - 1)`` with ``scale = fp32(B) / (hi - lo)``, every operation fp32 and rounded
once, entry 0 for ``x < lo`` and entry B + 1 for ``x > hi``; the joint histogram uses the
same formula with J bins and puts a prediction outside the range into the edge bin.  All
sums are integers, so every count is exact and every derived value (fp64, formed on the
device from the integer tables) is the same bits from run to run.

Everything runs on the device in three launches without global atomics or a host read, so
``measure`` can be captured in a HIP graph.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import SRMI_ERR_ARG, call, load, ptr, stream_handle

DEFAULT_PROBS = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999)
MAX_PROBS = 16
# srmi_distribution's flags (SRMI_DISTRIBUTION_*): the measured alternatives of the histogram kernel
MERGE_RUNS, ONE_COPY, COPY_BY_WAVE = 1, 2, 4


def distribution_workspace(C_: int, H: int, W: int, bins: int, joint: int) -> int:
    """srmi_distribution_workspace (host only): the bytes, or ValueError where it returns
    SRMI_ERR_ARG."""
    n = C.c_size_t()
    rc = load().srmi_distribution_workspace(int(C_), int(H), int(W), int(bins), int(joint), C.byref(n))
    if rc == SRMI_ERR_ARG:
        raise ValueError(f"the distribution score needs C, H, W >= 1 with H W < 2^31, bins in 2 .. 4096 and joint in "
                         f"0 .. 64, got {(C_, H, W)}, bins {bins}, joint {joint}")
    if rc:
        raise RuntimeError(f"srmi_distribution_workspace: {rc}")
    return int(n.value)


class DistributionScore:
    def __init__(self, shape: Tuple[int, int, int], bins: int = 256, joint: int = 32,
                 probs: Sequence[float] = DEFAULT_PROBS, value_range: Optional[Tuple[float, float]] = None,
                 device: Optional[torch.device] = None, flags: int = 0):
        """shape: (C, H, W) of the fields; bins: B in 2 .. 4096; joint: J in 0 .. 64 (0: no
        joint histogram); probs: up to 16 probabilities strictly inside (0, 1); value_range:
        (lo, hi) for every channel, finite with hi > lo, or None for each channel's truth's own
        min and max; flags: 0, or the measured alternatives of the kernel (the result does
        not depend on them).  Owns the workspace and the outputs: ``measure`` allocates
        nothing.  Bad arguments raise ValueError before anything is allocated."""
        Cn, H, W = (int(v) for v in shape)
        B, J = int(bins), int(joint)
        nbytes = distribution_workspace(Cn, H, W, B, J)
        pr = tuple(float(p) for p in probs)
        if len(pr) > MAX_PROBS or not all(0.0 < p < 1.0 for p in pr):
            raise ValueError(f"probs {probs!r}: at most {MAX_PROBS} numbers strictly inside (0, 1)")
        if value_range is not None:
            lo, hi = (float(np.float32(v)) for v in value_range)
            if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
                raise ValueError(f"value_range {value_range!r}: two finite fp32 numbers with hi > lo (or None)")
            self._lo_hi = (C.c_float * 2)(lo, hi)
        else:
            self._lo_hi = None
        if int(flags) & ~(MERGE_RUNS | ONE_COPY | COPY_BY_WAVE):
            raise ValueError(f"flags {flags!r}: unknown bits")
        self.C, self.H, self.W, self.bins, self.joint, self.probs, self.flags = Cn, H, W, B, J, pr, int(flags)
        self.value_range = None if value_range is None else (self._lo_hi[0], self._lo_hi[1])
        self._probs = (C.c_double * max(len(pr), 1))(*pr)
        d = torch.device(device) if device is not None else torch.device("cuda")
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        self.device = d
        P = len(pr)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=d)
        self.hist = torch.zeros((Cn, 2, B + 2), dtype=torch.int64, device=d)
        self.joint_hist = torch.zeros((Cn, J, J), dtype=torch.int64, device=d)
        self.range = torch.empty((Cn, 2), dtype=torch.float32, device=d)
        self.count = torch.zeros(Cn, dtype=torch.int64, device=d)
        self.derived = torch.empty((Cn, 4 + 2 * P), dtype=torch.float64, device=d)
        self.q_bias = torch.empty((Cn, P), dtype=torch.float64, device=d)

    def measure(self, pred: torch.Tensor, truth: torch.Tensor) -> Dict[str, torch.Tensor]:
        """pred, truth [C, H, W] fp32 on the device (NaN / Inf allowed: they are the mask) ->
        device tensors, views of this object's buffers, valid until the next call:
        'hist_pred', 'hist_truth' [C, B + 2] int64 (entry 0: below lo, entries 1 .. B: the
        bins, entry B + 1: above hi); 'joint' [C, J, J] int64, [c, ja, jb] with ja the
        prediction's bin; 'lo', 'hi' [C] fp32; 'count' [C] int64, the used pixels; 'pss' (the
        Perkins skill score, 1 = the same histogram), 'w1' (the Wasserstein-1 distance of
        the histograms, a lower bound when the prediction leaves the range), 'under', 'over'
        (the share of the prediction below lo and above hi) [C] fp64; 'q_pred', 'q_truth',
        'q_bias' = q_pred - q_truth [C, nprobs] fp64.  A channel without a used pixel has NaN
        in all of the fp64 values and in 'lo', 'hi'."""
        shape = (self.C, self.H, self.W)
        for name, t in (("pred", pred), ("truth", truth)):
            if (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
                    or t.device != self.device):
                raise ValueError(f"{name}: a contiguous fp32 {shape} tensor on {self.device} is needed, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
        P = len(self.probs)
        call("srmi_distribution", ptr(pred), ptr(truth), self.C, self.H, self.W, self.bins, self.joint, self._lo_hi,
             self._probs if P else None, P, ptr(self.workspace), self.workspace.numel(), ptr(self.hist),
             ptr(self.joint_hist) if self.joint else None, ptr(self.range), ptr(self.count), ptr(self.derived),
             self.flags, stream_handle())
        q_pred, q_truth = self.derived[:, 4:4 + P], self.derived[:, 4 + P:]
        torch.sub(q_pred, q_truth, out=self.q_bias)
        return {"hist_pred": self.hist[:, 0], "hist_truth": self.hist[:, 1], "joint": self.joint_hist,
                "lo": self.range[:, 0], "hi": self.range[:, 1], "count": self.count, "pss": self.derived[:, 0],
                "w1": self.derived[:, 1], "under": self.derived[:, 2], "over": self.derived[:, 3], "q_pred": q_pred,
                "q_truth": q_truth, "q_bias": self.q_bias}


def _np(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def bin_edges(lo, hi, bins: int) -> np.ndarray:
    """The B + 3 edges of the B + 2 histogram entries, fp64 [..., B + 3] for lo, hi of any
    (equal) shape: lo - w, lo, lo + w, ..., hi, hi + w with w = (hi - lo) / B -- under and over
    drawn as bins of one width beside the range, as 'w1' and the quantiles take them."""
    lo, hi = _np(lo).astype(np.float64), _np(hi).astype(np.float64)
    B = int(bins)
    w = (hi - lo) / B
    k = np.arange(-1, B + 2, dtype=np.float64)
    e = lo[..., None] + k * w[..., None]
    e[..., B + 1] = hi  # exactly, whatever lo + B w rounds to
    return e


def contingency(joint, k: int) -> Dict[str, np.ndarray]:
    """The 2 x 2 table of the event "the value lies at or above the lower edge of joint bin
    k", lo + k (hi - lo) / J, from the integer table joint [C, J, J] ([c, ja, jb], ja the
    prediction's bin): 'hits' (both), 'misses' (the truth alone), 'false_alarms' (the
    prediction alone), 'correct_negatives' int64 [C]; 'csi' = hits / (hits + misses + false
    alarms) and 'bias' = (hits + false alarms) / (hits + misses), the frequency bias, fp64
    [C] (NaN where the denominator is 0).  Values outside the range sit in the edge bins."""
    j = _np(joint).astype(np.int64)
    if j.ndim != 3 or j.shape[1] != j.shape[2] or j.shape[1] < 2:
        raise ValueError(f"joint: [C, J, J] with J >= 2 is needed, got {j.shape}")
    k = int(k)
    if not 1 <= k <= j.shape[1] - 1:
        raise ValueError(f"k = {k}: a bin in 1 .. {j.shape[1] - 1} (below bin 1 everything is an event)")
    hits = j[:, k:, k:].sum((1, 2))
    misses = j[:, :k, k:].sum((1, 2))
    fa = j[:, k:, :k].sum((1, 2))
    cn = j[:, :k, :k].sum((1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        csi = hits / (hits + misses + fa).astype(np.float64)
        bias = (hits + fa) / (hits + misses).astype(np.float64)
    return {"hits": hits, "misses": misses, "false_alarms": fa, "correct_negatives": cn, "csi": csi, "bias": bias}
