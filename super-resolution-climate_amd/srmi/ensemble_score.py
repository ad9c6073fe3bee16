"""Verification of an ensemble against a truth: does the spread say where to trust the mean?

No reference counterpart -- a deliberate extension, not a parity item.  Every other score here
verifies one deterministic field.  ``RegionSuperResolver(ensemble=4 | 8)`` ships a per-pixel
'spread'; this is what says whether it means anything: the CRPS of the K members' empirical
distribution (plain, and the fair one of Ferro 2014 that does not reward a small K), the rank
(Talagrand) histogram (flat when the truth is exchangeable with the members, U-shaped when the
ensemble is under-dispersed), the spread-skill ratio (Fortin et al. 2014: 1 when the spread is
as large as the error of the mean) with a reliability table binned by the spread, the Pearson
correlation of spread and |error|, and a per-pixel CRPS map.  It takes any [K, C, H, W] stack:
checkpoints, EMA against raw weights and seeds as well as the self-ensemble's 'members'.

Definition (``srmi_ensemble_score``, include/srmi.h; tests/ensemble_score_oracle.py restates it
in numpy)
------------------------------------------------------------------------------------------------
Per channel a pixel is used iff the truth and all K members are finite.  Per used pixel, in
fp64 with every operation rounded once: ``a = sum_j |m_j - y|``, ``b = sum_{j<l} |m_j - m_l|``,
``crps = a / K - b / K^2``, ``crps_fair = a / K - b / (K (K - 1))``, the mean, the ddof-0
variance ``var``, ``e = mean - y``, ``s = sqrt(var)``, the rank of the truth among the members
(members equal to the truth are counted in 'tied' and do not raise the rank) and the bin of
``(float)s`` among the B - 1 interior ``edges``.  The integer tables are exact; the fp64 sums are
added in a fixed order (the same bits on every run); the derived values are formed on the device
from the tables and sums alone.  Two launches without global atomics or a host read, so
``measure`` can be captured in a HIP graph.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ._lib import SRMI_ERR_ARG, SRMI_ERR_SHAPE, call, load, ptr, stream_handle

MIN_MEMBERS, MAX_MEMBERS, MAX_BINS = 2, 8, 16
# the pixels of a plane a workgroup of the main launch owns (kEnsSpan of csrc/ensemble_score.hip):
# the workspace grows by 9 + 2 B doubles and K + 3 + B uint32 per channel and such span
ENS_SPAN = 4096
# srmi_ensemble_score's launches (SRMI_ENSEMBLE_SCORE_*): 0 runs both; one bit times a launch alone
MAIN, FINISH = 1, 2
ENS_SUMS = ("crps", "crps_fair", "a", "b", "var", "e2", "abs_e", "s", "s_abs_e")  # sums' columns before the bins'
ENS_DERIVED = ("crps", "crps_fair", "rmse_mean", "spread_rms", "ssr", "spread_error_corr", "outliers",
               "outliers_expected", "reliability_index")  # derived's columns before bin_spread[B], bin_rmse[B]


def ensemble_workspace(K: int, C_: int, H: int, W: int, B: int) -> int:
    """srmi_ensemble_score_workspace (host only): the bytes, or ValueError where it refuses."""
    n = C.c_size_t()
    rc = load().srmi_ensemble_score_workspace(int(K), int(C_), int(H), int(W), int(B), C.byref(n))
    if rc in (SRMI_ERR_ARG, SRMI_ERR_SHAPE):
        raise ValueError(f"the ensemble score needs {MIN_MEMBERS} .. {MAX_MEMBERS} members, C, H, W >= 1 with H W < "
                         f"2^31 and 1 .. {MAX_BINS} spread bins, got {(K, C_, H, W)} and {B} bins")
    if rc:
        raise RuntimeError(f"srmi_ensemble_score_workspace: {rc}")
    return int(n.value)


class EnsembleScore:
    def __init__(self, shape: Tuple[int, int, int, int], edges=(), crps_map: bool = False,
                 device: Optional[torch.device] = None):
        """shape: (K, C, H, W) of the member stack, K in 2 .. 8; edges: the interior edges of
        the B spread bins of the reliability table -- a sequence of B - 1 floats (the same for
        every channel; empty: one bin), a [C, B - 1] array, or a [C, B - 1] fp32 tensor on the
        device, which is kept by reference and read at every ``measure`` (fill it on the
        device, e.g. from a quantile, without a host read), B in 1 .. 16, NaN allowed (such an
        edge is never reached); crps_map: also write the per-pixel CRPS.  Owns the workspace
        and the outputs: ``measure`` allocates nothing.  Bad arguments raise ValueError before
        anything is allocated."""
        try:
            K, Cn, H, W = (int(v) for v in shape)
        except (TypeError, ValueError):
            raise ValueError(f"shape {shape!r}: (K, C, H, W) is needed") from None
        d = torch.device(device) if device is not None else torch.device("cuda")
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        host = None
        if isinstance(edges, torch.Tensor):
            if (edges.dim() != 2 or edges.shape[0] != Cn or not 0 <= edges.shape[1] <= MAX_BINS - 1
                    or edges.dtype != torch.float32 or not edges.is_contiguous() or edges.device != d):
                raise ValueError(f"edges: a contiguous fp32 [{Cn}, 0 .. {MAX_BINS - 1}] tensor on {d} is needed, got "
                                 f"{tuple(edges.shape)} {edges.dtype} on {edges.device}")
            B = int(edges.shape[1]) + 1
        else:
            try:
                host = np.asarray(edges, dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError(f"edges {edges!r}: numbers are needed") from None
            if host.ndim == 1:
                host = np.tile(host[None], (max(Cn, 1), 1))
            if host.ndim != 2 or host.shape[0] != Cn or not 0 <= host.shape[1] <= MAX_BINS - 1:
                raise ValueError(f"edges: B - 1 or [{Cn}, B - 1] numbers with B in 1 .. {MAX_BINS} are needed, got shape "
                                 f"{host.shape}")
            B = int(host.shape[1]) + 1
        nbytes = ensemble_workspace(K, Cn, H, W, B)
        self.K, self.C, self.H, self.W, self.B, self.device = K, Cn, H, W, B, d
        self.edges = edges if host is None else torch.tensor(np.ascontiguousarray(host), device=d)
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=d)
        self.counts = torch.zeros((Cn, K + 3 + B), dtype=torch.int64, device=d)
        self.sums = torch.zeros((Cn, len(ENS_SUMS) + 2 * B), dtype=torch.float64, device=d)
        self.derived = torch.empty((Cn, len(ENS_DERIVED) + 2 * B), dtype=torch.float64, device=d)
        self.crps_map = torch.empty((Cn, H, W), dtype=torch.float32, device=d) if crps_map else None

    def measure(self, members: torch.Tensor, truth: torch.Tensor, launches: int = 0) -> Dict[str, torch.Tensor]:
        """members [K, C, H, W], truth [C, H, W] fp32 on the device (NaN / Inf allowed: they are
        the mask) -> device tensors, views of this object's buffers, valid until the next call.
        Tables, int64, exact: 'used' [C], 'rank_hist' [C, K + 1], 'tied' [C], 'bin_count' [C, B].
        'sums' [C, 9 + 2 B] fp64 (ENS_SUMS, then per bin var and e^2), with 'bin_var' and 'bin_e2'
        [C, B] its per-bin columns.  Derived, fp64 [C]: 'crps', 'crps_fair', 'rmse_mean' (of the
        ensemble mean), 'spread_rms', 'ssr' (sqrt((K + 1) / (K - 1) mean var) / rmse_mean: below 1
        the ensemble is under-dispersed), 'spread_error_corr', 'outliers' (the share of the two
        outer ranks) beside 'outliers_expected' = 2 / (K + 1), 'reliability_index' (the summed
        distance of the rank frequencies from flat); [C, B]: 'bin_spread' and 'bin_rmse', the
        reliability table (on the diagonal when the spread is calibrated; NaN in an empty bin).
        'edges' [C, B - 1] fp32, the ones used, and with crps_map=True 'crps_map' [C, H, W] fp32,
        NaN where a pixel is not used.  A channel without a used pixel has NaN in every derived
        value and 0 in every table and sum.  launches: 0, or MAIN | FINISH bits to run one of the
        two launches alone (a diagnostic for timing: FINISH reads what an earlier call left in the
        workspace)."""
        mshape, tshape = (self.K, self.C, self.H, self.W), (self.C, self.H, self.W)
        for name, t, shape in (("members", members, mshape), ("truth", truth, tshape)):
            if (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()
                    or t.device != self.device):
                raise ValueError(f"{name}: a contiguous fp32 {shape} tensor on {self.device} is needed, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
        call("srmi_ensemble_score", ptr(members), ptr(truth), self.K, self.C, self.H, self.W,
             ptr(self.edges) if self.B > 1 else None, self.B, ptr(self.workspace), self.workspace.numel(),
             ptr(self.counts), ptr(self.sums), ptr(self.derived), ptr(self.crps_map), int(launches), stream_handle())
        K, B, ns, nd = self.K, self.B, len(ENS_SUMS), len(ENS_DERIVED)
        res = {"used": self.counts[:, 0], "rank_hist": self.counts[:, 1:K + 2], "tied": self.counts[:, K + 2],
               "bin_count": self.counts[:, K + 3:], "sums": self.sums, "bin_var": self.sums[:, ns::2],
               "bin_e2": self.sums[:, ns + 1::2], "derived": self.derived, "bin_spread": self.derived[:, nd:nd + B],
               "bin_rmse": self.derived[:, nd + B:], "edges": self.edges}
        for i, name in enumerate(ENS_DERIVED):
            res[name] = self.derived[:, i]
        if self.crps_map is not None:
            res["crps_map"] = self.crps_map
        return res
