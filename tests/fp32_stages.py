"""Stage-level intermediates of an RCANOracle (CPU) and of the exact-fp32 engine, for
tests/test_gpu_fp32_stages.py: the maps every RCAB saves in the forward (t = relu(conv1),
u = conv2, the RCAB output) and, after ``out.backward(dy)``, the gradient maps the engine's
backward stages leave behind (dz w.r.t. conv1's pre-ReLU output, du w.r.t. conv2's output,
the gradient w.r.t. each group's input, dRES w.r.t. the upsampler's input).

All maps are returned NHWC ([n, h, w, 64]), the engine's layout.  A fixed upstream dy
replaces the loss, so every image's backward is independent of the batch."""
import copy

import torch
import torch.nn.functional as F

from oracle import rcan_oracle as ro
from srmi.engine import Engine, NetSpec, param_table


def nhwc(x):
    return x.detach().permute(0, 2, 3, 1).contiguous()


# |fl(sum) - sum| <= gamma_K sum |w_i x_i| for a K-term fp32 dot product in ANY order of
# summation (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5); K = 64 x 9
# products and the bias; twice that, for the operands' own fp32 rounding (a few u each)
# passing through the same sum
_K = 64 * 9 + 1
_U = 2.0 ** -24
Z_TOL = 2 * _K * _U / (1 - _K * _U)


def oracle_stages(model, lr, dy, masks=None, loss_fn=None):
    """Forward `model` (an RCANOracle, any dtype) on lr, backward dy.  -> dict:
    ("hb", g, b): b = 0 the input of group g (g = nlayers: of the body tail), b >= 1 the
    output of RCAB b; ("z" | "t" | "u", g, b) (z = conv1's output); ("ztol", g, b): the bound
    Z_TOL (|conv1.w| * |x| + |conv1.b|) on the fp32 rounding error of z, per element;
    ("dz" | "du", g, b); ("gin", g) the gradient w.r.t. group g's input; ("dres",);
    "grads": {parameter name: gradient}.
    masks: {(g, b): bool NCHW} replaces RCAB (g, b)'s ReLU by z * mask, forward and backward.
    loss_fn (dy None): backward of the scalar loss_fn(out) instead, returned as "loss"."""
    dt = next(model.parameters()).dtype
    keep, tol = {}, {}
    hooks = []

    def save(key, grad_key=None):
        def hook(_m, _inp, out):
            keep[key] = out
            if grad_key is not None:
                out.retain_grad()
                keep[grad_key] = out
        return hook

    def save_input(key, grad_key):
        def hook(_m, inp):
            keep[key] = inp[0]
            inp[0].retain_grad()
            keep[grad_key] = inp[0]
        return hook

    def ztol(key):
        def hook(m, inp, _out):
            with torch.no_grad():
                tol[key] = Z_TOL * F.conv2d(inp[0].abs(), m.weight.abs(), m.bias.abs(), padding=1)
        return hook

    def masked(mask):
        def hook(_m, inp, _out):
            return inp[0] * mask.to(inp[0].dtype)
        return hook

    groups = list(model.body)[:-1]
    nl = len(groups)
    for g, grp in enumerate(groups):
        hooks.append(grp.register_forward_pre_hook(save_input(("hb", g, 0), ("gin", g))))
        for b, rcab in enumerate(list(grp.body)[:-1], start=1):
            hooks.append(rcab.body[0].register_forward_hook(save(("z", g, b), ("dz", g, b))))
            hooks.append(rcab.body[0].register_forward_hook(ztol(("ztol", g, b))))
            if masks is not None:
                hooks.append(rcab.body[1].register_forward_hook(masked(masks[(g, b)])))
            hooks.append(rcab.body[1].register_forward_hook(save(("t", g, b))))
            hooks.append(rcab.body[2].register_forward_hook(save(("u", g, b), ("du", g, b))))
            hooks.append(rcab.register_forward_hook(save(("hb", g, b))))
    hooks.append(model.body[nl].register_forward_pre_hook(save_input(("hb", nl, 0), ("_gtail",))))
    hooks.append(model.tail.register_forward_pre_hook(save_input(("_res",), ("dres",))))
    model.zero_grad()
    out = model(lr.to(dt))
    if loss_fn is not None:
        loss = loss_fn(out)
        loss.backward()
    else:
        out.backward(dy.to(dt))
    for h in hooks:
        h.remove()
    res = {}
    for key, v in keep.items():
        if key[0] in ("_gtail", "_res"):
            continue
        res[key] = nhwc(v.grad if key[0] in ("dz", "du", "gin", "dres") else v)
    for key, v in tol.items():
        res[key] = nhwc(v)
    res["grads"] = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    if loss_fn is not None:
        res["loss"] = float(loss.detach())
    model.zero_grad()
    return res


def relu_masks(t_maps):
    """{(g, b): the engine's t, NHWC} -> the masks argument of oracle_stages."""
    return {k: (v > 0).permute(0, 3, 1, 2).cpu() for k, v in t_maps.items()}


def mask_flips(ref, t_maps):
    """The ReLU decisions of t_maps that differ from the fp64 intermediates ref:
    ([(g, b), image, (c, y, x), z, bound] per element, [(g, b)] where one lies outside the
    bound ("ztol") or they are more than 1e-5 of the map)."""
    flips, bad = [], []
    for (g, b), t in sorted(t_maps.items()):
        z, tol = ref[("z", g, b)], ref[("ztol", g, b)]
        differ = (t.cpu() > 0) != (z > 0)
        for n, y, x, c in differ.nonzero().tolist():
            flips.append(((g, b), f"image {n}", (c, y, x), f"z {float(z[n, y, x, c]):+.2e}",
                          f"bound {float(tol[n, y, x, c]):.1e}"))
        if bool((differ & (z.abs() > tol)).any()) or int(differ.sum()) > 1e-5 * differ.numel():
            bad.append((g, b))
    return flips, bad


def make_case(nl, nb, cb, hw, B=2, C=2, seed_w=9, seed_x=13, seed_dy=5):
    """The model, spec, parameters and inputs of one configuration: seed-9 weights,
    synthetic_hr(B, C, 4 h, 13) (square tiles; else the top-left 4h x 4w of the 4 max(h, w)
    square), lr = its fp32 bicubic downsample, dy ~ N(0, 1) / numel (the scale of an RMSE
    gradient at loss 1)."""
    h, w = hw
    model = ro.RCANOracle(nchannels_in=C, nchannels_out=C, nlayers=nl, nblocks=nb, nfeatures=64, cbottleneck=cb)
    ro.init_params_numpy(model, seed_w)
    spec = NetSpec(arch="rcan", nchannels_in=C, nchannels_out=C, nfeatures=64, nlayers=nl, nblocks=nb, cbottleneck=cb,
                   scale=4, dtype="fp32")
    table = param_table(spec)
    sd = dict(model.named_parameters())
    flat = torch.cat([sd[n].detach().reshape(-1).float() for n, _, _, _ in table])
    S = 4 * max(h, w)
    hr = torch.tensor(ro.synthetic_hr(B, C, S, seed_x))[:, :, :4 * h, :4 * w].contiguous()
    lr = ro.downsample(hr, 4).contiguous()
    gen = torch.Generator().manual_seed(seed_dy)
    dy = torch.randn(hr.shape, generator=gen) / hr.numel()
    return dict(model=model, spec=spec, table=table, flat=flat, lr=lr, dy=dy, nl=nl, nb=nb, hw=(h, w), B=B)


def oracle_pair(case):
    """(fp64 intermediates, {key: per-image rel-L2 drift of fp32 torch on the CPU from them})."""
    ref = oracle_stages(copy.deepcopy(case["model"]).double(), case["lr"], case["dy"])
    f32 = oracle_stages(copy.deepcopy(case["model"]).float(), case["lr"], case["dy"])
    drift = {"grads": {name: rel_l2(f32["grads"][name], g) for name, g in ref["grads"].items()}}
    for key, v in ref.items():
        if key == "grads" or key[0] == "ztol":
            continue
        drift[key] = [rel_l2(f32[key][n], v[n]) for n in range(v.shape[0])]
    return ref, drift


def oracle_with_masks(case, t_maps):
    """The fp64 intermediates with every RCAB's ReLU mask taken from t_maps {(g, b): the
    engine's t, NHWC}: where a pre-activation lies inside the fp32 rounding error of zero,
    which side of the ReLU it falls on is the summation order's choice, and the whole
    backward below it follows that choice."""
    return oracle_stages(copy.deepcopy(case["model"]).double(), case["lr"], case["dy"], masks=relu_masks(t_maps))


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


SAVED = (("HB", 0, 0), ("T", 0, 1), ("U", 0, 1), ("REC", 0, 1))  # group 0's first RCAB: the first slot of each array


def engine_stages(case, dev, capacity=None, images=None):
    """Run the exact-fp32 engine on the case (images: a slice of the batch, default all;
    capacity: the engine's, default the number of images): forward, then the backward one
    stage at a time.  -> dict with the oracle_stages keys the engine exposes (with nb > 1 a
    group's stage leaves the dz / du of its first RCAB), plus
    "grads": the flat gradient; "clobbered": [(buffer, stage)] for every SAVED buffer that
    is not bit-identical to its post-forward snapshot after a backward stage;
    "closure": group 0's first RCAB's operands as they are right after group 0's stage
    (hb00, dz, t01, du)."""
    nl, nb, (h, w) = case["nl"], case["nb"], case["hw"]
    sl = images if images is not None else slice(0, case["B"])
    lr = case["lr"][sl].contiguous().to(dev)
    dy = case["dy"][sl].contiguous().to(dev)
    n = lr.shape[0]
    eng = Engine(case["spec"], capacity or n, (h, w), train=True, device=dev)
    flat = case["flat"].to(dev)
    eng.pack(flat)
    eng.forward(flat, lr)
    torch.cuda.synchronize()
    res = {}
    for g in range(nl):
        res[("hb", g, 0)] = eng.buffer("HB", g, 0).cpu()
        for b in range(1, nb + 1):
            res[("hb", g, b)] = eng.buffer("HB", g, b).cpu()
            res[("t", g, b)] = eng.buffer("T", g, b).cpu()
            res[("u", g, b)] = eng.buffer("U", g, b).cpu()
    res[("hb", nl, 0)] = eng.buffer("HB", nl, 0).cpu()
    snap = {k: eng.buffer(*k).clone() for k in SAVED}
    grads = torch.zeros(eng.n_params, device=dev)
    res["clobbered"] = []
    assert eng.stage_count == nl + 2
    for s in range(nl + 2):
        eng.backward(flat, lr, grads, dy=dy, stages=(s, s))
        torch.cuda.synchronize()
        for k, v in snap.items():
            if not torch.equal(eng.buffer(*k), v):
                res["clobbered"].append((k, s))
        if s == 0:
            res[("dres",)] = eng.buffer("DRESF").cpu()
        if 1 <= s <= nl:
            g = nl - s
            res[("dz", g, 1)] = eng.buffer("DZ").cpu()
            res[("du", g, 1)] = eng.buffer("DU").cpu()
            res[("gin", g)] = eng.buffer("GROUP_IN_GRAD", g).cpu()
            if g == 0:
                res["closure"] = dict(hb00=eng.buffer("HB", 0, 0).cpu(), dz=res[("dz", 0, 1)],
                                      t01=eng.buffer("T", 0, 1).cpu(), du=res[("du", 0, 1)])
    res["grads"] = grads.cpu()
    return res
