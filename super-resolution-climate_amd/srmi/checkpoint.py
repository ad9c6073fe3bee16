"""Checkpoints in the reference's format.

CheckpointManager.save_checkpoint (sres/controller/checkpoints.py:18-26) writes
``dict(epoch, itime, model_state_dict, optimizer_state_dict, loss)`` with
``torch.save``; load_checkpoint (:35-51) restores the model and the
``torch.optim.Adam`` state.  The plugin path (srmi.model.*: an nn.Module plus a
real torch Adam) goes through that manager unchanged.  For the fused trainer,
whose parameters and Adam moments live in flat device buffers, these helpers
convert between the flat buffers and the exact torch state-dict layouts, so a
checkpoint written by either side resumes on the other:

* model_state_dict: the reference's keys/shapes (state-dict order);
* optimizer_state_dict: torch.optim.Adam's ``{"state": {i: {"step",
  "exp_avg", "exp_avg_sq"}}, "param_groups": [...]}`` with parameter index i
  in ``model.parameters()`` order (= state-dict order for these networks).
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch


def model_state_dict(flat: torch.Tensor, table) -> Dict[str, torch.Tensor]:
    host = flat.detach().float().cpu()
    return {name: host[off:off + n].view(shape).clone() for name, off, n, shape in table}


def load_model_state_dict(flat: torch.Tensor, table, sd: Dict[str, torch.Tensor], strict: bool = True,
                          apply: bool = True) -> torch.Tensor:
    """A reference state dict -> the flat layout, with FModule.load_state_dict's
    semantics (sres/model/common/common.py:50-71): a key whose shape differs is
    skipped if it is under 'tail' (a re-shaped upsampler) and raises otherwise;
    with strict, unexpected keys not under 'tail' and missing keys raise.  Returns
    the host buffer; apply copies it into `flat`."""
    host = flat.detach().cpu().clone()
    names = {name for name, _, _, _ in table}
    if strict:
        extra = [k for k in sd if k not in names and "tail" not in k]
        if extra:
            raise KeyError(f'unexpected key "{extra[0]}" in state_dict')
        missing = names - set(sd)
        if missing:
            raise KeyError(f'missing keys in state_dict: "{missing}"')
    for name, off, n, shape in table:
        if name not in sd:
            continue
        t = sd[name]
        if tuple(t.shape) != tuple(shape):
            if "tail" in name:
                continue
            raise RuntimeError(f"While copying the parameter named {name}, whose dimensions in the model are "
                               f"{tuple(shape)} and whose dimensions in the checkpoint are {tuple(t.shape)}.")
        host[off:off + n] = t.detach().float().reshape(-1)
    if apply:
        flat.copy_(host)
    return host


def adam_state_dict(table, m: torch.Tensor, v: torch.Tensor, step: int, lr: float, betas=(0.9, 0.999),
                    eps: float = 1e-8, weight_decay: float = 0.0) -> Dict:
    """torch.optim.Adam.state_dict() layout for the flat moments."""
    mh, vh = m.detach().float().cpu(), v.detach().float().cpu()
    state = {}
    if step > 0:
        for i, (_, off, n, shape) in enumerate(table):
            state[i] = {"step": torch.tensor(float(step)), "exp_avg": mh[off:off + n].view(shape).clone(),
                        "exp_avg_sq": vh[off:off + n].view(shape).clone()}
    group = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay, "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "decoupled_weight_decay": False, "params": list(range(len(table)))}
    return {"state": state, "param_groups": [group]}


def load_adam_state_dict(table, sd: Dict, m: torch.Tensor, v: torch.Tensor, apply: bool = True):
    """Flat moments from a torch Adam state dict.  All parameters must share one step
    count (one param group, as dual_trainer.py:126).  apply=True copies the moments
    into m, v and returns (step, param-group hyper-parameters); apply=False leaves
    them and returns (step, hyper-parameters, m_host, v_host)."""
    groups = sd["param_groups"]
    if len(groups) != 1 or len(groups[0]["params"]) != len(table):
        raise ValueError("expected one Adam param group over all model parameters")
    mh = torch.zeros(m.numel(), dtype=torch.float32)
    vh = torch.zeros(v.numel(), dtype=torch.float32)
    steps = set()
    for i, (name, off, n, shape) in enumerate(table):
        st = sd["state"].get(groups[0]["params"][i])
        if st is None:
            steps.add(0)
            continue
        steps.add(int(float(st["step"])))
        for key, dst in (("exp_avg", mh), ("exp_avg_sq", vh)):
            x = st[key]
            if x.numel() != n:
                raise ValueError(f"{name}: Adam {key} has {x.numel()} elements, expected {n}")
            dst[off:off + n] = x.float().reshape(-1)
    if len(steps) != 1:
        raise ValueError(f"parameters at different Adam steps: {sorted(steps)}")
    g = groups[0]
    hp = {k: g[k] for k in ("lr", "betas", "eps", "weight_decay")}
    if not apply:
        return steps.pop(), hp, mh, vh
    m.copy_(mh)
    v.copy_(vh)
    return steps.pop(), hp


def checkpoint(epoch: int, itime: int, flat, table, m, v, step, lr, betas, eps, wd, loss: float) -> Dict:
    """The dict CheckpointManager.save_checkpoint writes (checkpoints.py:20)."""
    return dict(epoch=epoch, itime=itime, model_state_dict=model_state_dict(flat, table),
                optimizer_state_dict=adam_state_dict(table, m, v, step, lr, betas, eps, wd), loss=loss)


def optimizer_record(skipped: int, ema_decay=None, ema_warmup=None) -> Dict:
    """The fused trainer's srmi_optimizer key beside the reference's five: what its optimizer
    guards hold that torch.optim.Adam's state dict has no place for.  Plain Python values
    (torch.load(weights_only=True) reads them).  CheckpointManager.load_checkpoint
    (checkpoints.py:35-51) pops the two dicts it knows and reads the rest with .get, so a
    reference process loads a file with this key, and with ema_state_dict, unchanged."""
    return dict(skipped=int(skipped), ema_decay=None if ema_decay is None else float(ema_decay),
                ema_warmup=None if ema_warmup is None else bool(ema_warmup))


def add_optimizer_extras(state: Dict, table, skipped: int, ema_cfg=None, ema: "torch.Tensor | None" = None) -> Dict:
    """The two keys a guarded trainer adds to checkpoint()'s dict: srmi_optimizer and, with
    averaged weights, ema_state_dict in model_state_dict's layout."""
    cfg = ema_cfg or {}
    state["srmi_optimizer"] = optimizer_record(skipped, cfg.get("decay"), cfg.get("warmup"))
    if ema is not None:
        state["ema_state_dict"] = model_state_dict(ema, table)
    return state


def load_optimizer_extras(table, state: Dict, params_host: torch.Tensor, ema: "torch.Tensor | None"):
    """-> (skipped, ema_host): validated on the host, nothing is applied.  skipped from
    srmi_optimizer (0 for a file without it; ValueError for a record that is no dict or
    whose count is no whole number >= 0).  ema (the trainer's flat buffer, None without
    averaged weights: the file's ema_state_dict is then ignored and ema_host is None): the
    file's ema_state_dict with the model dict's strict semantics, or params_host when the
    file has none."""
    rec = state.get("srmi_optimizer")
    if rec is not None and not isinstance(rec, dict):
        raise ValueError(f"srmi_optimizer: a dict, got {type(rec).__name__}")
    skipped = 0 if rec is None else rec.get("skipped", 0)
    if not isinstance(skipped, int) or isinstance(skipped, bool) or skipped < 0:
        raise ValueError(f"srmi_optimizer: skipped a whole number >= 0, got {skipped!r}")
    if ema is None:
        return skipped, None
    sd = state.get("ema_state_dict")
    if sd is None:
        return skipped, params_host.clone()
    return skipped, load_model_state_dict(ema, table, sd, strict=True, apply=False)
