"""Per-launch closure of what the bf16 engine's backward runs OUTSIDE the residual groups, for
tests/test_gpu_bf16_outer.py and tests/test_bf16_outer_checks.py: stage 0 (the tail conv's dgrad
and filter gradient, the upsamplers' and the body tail's backward) and the last stage (the head's
filter gradient), and EDSR's one-stage backward, which no trace reaches.

The checks are pure functions of a STATE: a dict of CPU tensors holding every operand and every
output of every launch plus the fp32 master parameters (engine_state fills it from an engine
through Engine.buffer, reference_state from an fp64 restatement rounded where the engine stores),
and return a bf16_stages.Report; they need no GPU.  Every launch's output is recomputed in fp64
from the operands the state holds for it, so nothing compounds and the bars are a priori
(bf16_stages' Report, acc, bf, bf16_ulp and bars).  In the bf16 mode every reference uses the
filter rounded to bf16, as the packs are -- except the tail conv's dgrad, which reads the fp32
master weights as they are (small.hip tail_dgrad_kernel).

Keys of a state: "meta" (make_case's arguments and nups), "table", "params", "lr" [n, C, h, w];
the upstream gradient as "dy" [n, Co, H, W], or "sr", "hr" and "loss4" (the RMSE form: the tail
kernels form (sr - hr) * loss4[2] on the fly; the reference forms it in fp64 from the same three);
("PS", k), "RESB", ("HB", nl, 0), ("DPS", k), "DRESF", "DRESB", ("BODY_GRAD", 0 | 1), "HEAD_GRAD";
"grads0": the flat gradient after stage 0 (tail, upsamplers, body tail), "grads": after the last
stage.  EDSR adds "X0F", ("HB", i, 0), ("T", i), "DZ".  Maps are NHWC in their own type.

Classes (the issue's table):
a  tail dgrad: DPS[nups - 1] = bf16(convT(dy, fp32 tail filter)); Report.bf16_map with the
   accumulation bound acc(9 Co + 2) (|w| * |dy|) where dy is formed on the fly (its two roundings
   ride in it), acc(9 Co) where dy is explicit.
b  tail filter gradient + its slab reduction: tail.weight / tail.bias from dy and PS[nups - 1].
c  upsampler k, last to first: filter and bias gradient from (RESB | PS[k - 1],
   pixel_unshuffle(DPS[k])); its dgrad DPS[k - 1] (bf16_map, K = 256 x 9), for k = 0 DRESF (fp32,
   acc(256 x 9)) and DRESB, a rounding of the STORED DRESF: half a bf16 ulp of it.
d  body tail: filter and bias gradient from (HB(nl, 0), DRESB); BODY_GRAD 0 (fp32, acc(577)),
   BODY_GRAD 1 a rounding of the stored fp32 map.
e  head filter gradient + reduction from (lr, HEAD_GRAD).
f  EDSR.  nlayers == 1, the ResBlock's backward: conv2's filter gradient = res_scale x
   wgrad(T(0), BODY_GRAD 1); DZ = bf16(res_scale relu'(T) convT(BODY_GRAD 1)); conv1's filter
   gradient from (HB(0, 0), DZ); HEAD_GRAD = convT(DZ) + BODY_GRAD 0 + DRESF.  At nlayers >= 2
   every block writes one of the two gradient buffers (fp32 + bf16) from the other and the two
   swap, and DZ is rewritten by every block.  What survives to the end of the one-stage
   backward: DPS, DRESF, DRESB (stage-0 maps nothing overwrites), HEAD_GRAD, block 0's DZ
   beside its saved HB(0, 0), and, in the buffer HEAD_GRAD is not in, the gradient w.r.t. block
   0's output -- which no accessor reaches on an EDSR engine (GROUP_IN_GRAD is RCAN's, BODY_GRAD
   names one fixed buffer: at nlayers 2 the one HEAD_GRAD is in).  That missing operand is what
   limits class f at nlayers >= 2 to block 0's conv1 filter gradient (block 0's conv2, DZ and
   HEAD_GRAD would need it), and class d to the body tail's filter gradient (BODY_GRAD no
   longer holds the body tail's dgrad).
g  EDSR at nlayers == 1, the forward from saved maps (bf16_forward's class g bars): HB(0, 0) ==
   bf16(X0F), T, HB(1, 0) = bf16(res_scale (conv2 + b) + X0F), RESB, PS[k], sr.

Bars of the fp32 outputs: elementwise acc(K) sum |terms| (the any-order bound, K the number of
terms: n H W pixels for a filter gradient, + 2 where dy is formed on the fly), and per tensor,
weight and bias alike, rel-L2 <= 1e-5 (F32_L2, test_wgrad's bar; torch's own fp32 conv2d_weight
sits at 0.9e-6 to 1.8e-6 of fp64 for the tail and 2e-7 to 4e-7 for the head at these shapes,
torch's fp32 sum of the same dy at 3e-8 to 3.4e-7 for tail.bias and of the same head gradient at
8e-8 to 1.4e-7 for head.bias, over the nine cases).  The rel-L2 is the sharp bar of the
biases: their sums cancel to a few per cent of sum |terms|, where the elementwise bound alone
(acc(K) up to 8.8e-3) would let a bias be 10 % off.  No element is excluded; maps are reported
per image.
"""
import torch
import torch.nn.functional as F

from bf16_stages import F32_L2, K_CONV, Report, acc, bf, bf16_ulp, dgrad, nchw, nhwc
from oracle import rcan_oracle as ro
from srmi.engine import NetSpec, param_table

CLASSES = "abcdefg"
K_UP = 256 * 9

#        arch    (h, w)   scale cin cout n cap cu  dy form     nl nb res_scale
CONFIGS = [
    ("rcan", (4, 48), 4, 1, 1, 1, 1, 0, "rmse", 2, 1, 1.0),
    ("rcan", (8, 48), 2, 2, 2, 3, 3, 0, "explicit", 2, 1, 1.0),
    ("rcan", (8, 144), 2, 1, 1, 1, 1, 0, "rmse", 2, 1, 1.0),
    ("rcan", (8, 32), 4, 3, 3, 2, 3, 0, "rmse", 2, 1, 1.0),
    ("rcan", (4, 32), 8, 4, 4, 1, 1, 0, "explicit", 2, 1, 1.0),
    ("rcan", (24, 96), 4, 2, 2, 1, 1, 0, "explicit", 2, 1, 1.0),
    ("rcan", (48, 48), 4, 2, 1, 2, 2, 128, "rmse", 2, 1, 1.0),
    ("edsr", (4, 32), 8, 4, 4, 2, 2, 0, "explicit", 1, 0, 0.5),
    ("edsr", (8, 48), 4, 1, 1, 1, 1, 0, "rmse", 2, 0, 1.0),
]
CB = 2  # the RCAN cases' CA reduction


def case_id(c):
    return f"{c[0]}-{c[1][0]}x{c[1][1]}-x{c[2]}-c{c[3]}to{c[4]}-n{c[5]}of{c[6]}-cu{c[7]}-{c[8]}" + (
        f"-nl{c[9]}-rs{c[11]}" if c[0] == "edsr" else "")


def launch_paths(c):
    """The branches a case reaches, from its shapes alone (small.hip: tail_dgrad_t picks TWT 64 at
    HR widths that are a multiple of 64, else 32; tail_wgrad_lds_kernel<CC> walks 64-pixel
    segments, the last one partial where the width is no multiple of 64; head_wgrad_kernel's C)."""
    arch, (h, w), scale, cin, cout, n, cap, cu, dy_form = c[:9]
    W = w * scale
    assert W % 32 == 0
    return dict(twt=64 if W % 64 == 0 else 32, partial_segment=W % 64 != 0, cc=cout, head_c=cin,
                nups=scale.bit_length() - 1, dy_form=dy_form, below_capacity=n < cap, cu=cu)


def make_case(arch, hw, scale, cin, cout, n, cap, cu, dy_form, nl, nb, res_scale):
    """Seed-9 weights, synthetic_hr tiles (the top-left of the scale max(h, w) square), lr their
    bicubic downsample, and an explicit dy ~ N(0, 1) / numel (fp32_stages.make_case's)."""
    h, w = hw
    nups = scale.bit_length() - 1
    kw = dict(nchannels_in=cin, nchannels_out=cout, nlayers=nl, nfeatures=64, downscale_factors=[2] * nups)
    if arch == "rcan":
        model = ro.RCANOracle(nblocks=nb, cbottleneck=CB, **kw)
    else:
        model = ro.EDSROracle(res_scale=res_scale, **kw)
    ro.init_params_numpy(model, 9)
    spec = NetSpec(arch=arch, nchannels_in=cin, nchannels_out=cout, nfeatures=64, nlayers=nl, nblocks=nb,
                   cbottleneck=CB, scale=scale, res_scale=res_scale, dtype="bf16")
    table = param_table(spec)
    sd = dict(model.named_parameters())
    flat = torch.cat([sd[name].detach().reshape(-1).float() for name, _, _, _ in table])
    S = scale * max(h, w)
    full = torch.tensor(ro.synthetic_hr(n, max(cin, cout), S, 13))[:, :, :scale * h, :scale * w]
    hr = full[:, :cout].contiguous()
    lr = ro.downsample(full[:, :cin].contiguous(), scale).contiguous()
    gen = torch.Generator().manual_seed(5)
    dy = torch.randn(hr.shape, generator=gen) / hr.numel()
    meta = dict(arch=arch, h=h, w=w, scale=scale, cin=cin, cout=cout, n=n, cap=cap, cu=cu, dy_form=dy_form, nl=nl,
                nb=nb, res_scale=float(res_scale), nups=nups)
    return dict(meta=meta, model=model, spec=spec, table=table, flat=flat, lr=lr, hr=hr, dy=dy)


# ------------------------------------------------------------------ helpers
def _P(st):
    tab = {name: (off, cnt, shape) for name, off, cnt, shape in st["table"]}
    prm = st["params"].double()

    def P(name):
        off, cnt, shape = tab[name]
        return prm[off:off + cnt].view(shape)

    def G(name, key="grads"):
        off, cnt, shape = tab[name]
        return st[key].double()[off:off + cnt].view(shape)

    return P, G


def upstream(st):
    """dy [n, Co, H, W] in fp64: explicit, or (sr - hr) * loss4[2] from the fp32 sr, hr, loss4[2]."""
    if "dy" in st:
        return st["dy"].double()
    return (st["sr"].double() - st["hr"].double()) * float(st["loss4"][2])


def conv(x, w, b=None):
    """conv2d(., w, padding=1) + b: x NHWC fp64 -> NHWC."""
    return nhwc(F.conv2d(nchw(x), w, b, padding=1))


def wgrad(x, dyc, cout):
    """The filter gradient of conv2d(x, ., padding=1): x NHWC, dyc NCHW, both fp64."""
    xc = nchw(x)
    return torch.nn.grad.conv2d_weight(xc, (cout, xc.shape[1], 3, 3), dyc, padding=1)


def _filter_gradient(rep, cls, what, gb, got_w, got_b, x, dyc, k, scale=1.0):
    """got_w / got_b against scale x the fp64 filter / bias gradient of (x NHWC, dyc NCHW): acc(k)
    sum |terms| elementwise, the weight also at 1e-5 rel-L2."""
    cout = dyc.shape[1]
    ref = scale * wgrad(x, dyc, cout)
    mag = abs(scale) * wgrad(x.abs(), dyc.abs(), cout)
    rep.elem(cls, what + ".weight", gb, got_w, ref, acc(k) * mag, l2bar=F32_L2, per_image=False)
    rep.elem(cls, what + ".bias", gb, got_b, scale * dyc.sum((0, 2, 3)), acc(k) * abs(scale) * dyc.abs().sum((0, 2, 3)),
             l2bar=F32_L2, per_image=False)


def _rounding_of_stored(rep, cls, what, gb, got, stored):
    """A bf16 copy of a stored fp32 map: within half a bf16 ulp of the stored value."""
    s = stored.double()
    rep.elem(cls, what, gb, got, s, bf16_ulp(s) / 2)


# ------------------------------------------------------------------ the checks
def check_tail(st, rep):
    """Classes a and b."""
    m = st["meta"]
    P, G = _P(st)
    k, co = m["nups"] - 1, m["cout"]
    dy = upstream(st)
    dyh = nhwc(dy)
    wt = P("tail.1.weight")  # the fp32 master, as it is
    formed = 0 if "dy" in st else 2  # the subtraction's and the scaling's rounding, where dy is formed on the fly
    rep.bf16_map("a", f"DPS[{k}] (tail dgrad)", (k, 0), st[("DPS", k)], dgrad(dyh, wt),
                 acc(9 * co + formed) * dgrad(dyh.abs(), wt.abs()))
    kk = dy.shape[0] * dy.shape[2] * dy.shape[3] + formed
    _filter_gradient(rep, "b", "tail", (k, 0), G("tail.1.weight", "grads0"), G("tail.1.bias", "grads0"),
                     st[("PS", k)].double(), dy, kk)


def check_upsamplers(st, rep):
    """Class c."""
    m = st["meta"]
    P, G = _P(st)
    for k in range(m["nups"] - 1, -1, -1):
        xin = (st["RESB"] if k == 0 else st[("PS", k - 1)]).double()
        dyc = F.pixel_unshuffle(nchw(st[("DPS", k)]), 2)  # torch's channel 4 c + q: phase q of channel c
        name = f"tail.0.{2 * k}"
        _filter_gradient(rep, "c", f"ups[{k}]", (k, 0), G(name + ".weight", "grads0"), G(name + ".bias", "grads0"),
                         xin, dyc, xin.shape[0] * xin.shape[1] * xin.shape[2])
        wk = bf(P(name + ".weight"))
        ref = nhwc(F.conv_transpose2d(dyc, wk, padding=1))
        mag = nhwc(F.conv_transpose2d(dyc.abs(), wk.abs(), padding=1))
        if k > 0:
            rep.bf16_map("c", f"DPS[{k - 1}] (ups[{k}] dgrad)", (k, 0), st[("DPS", k - 1)], ref, acc(K_UP) * mag)
        else:
            rep.elem("c", "DRESF (ups[0] dgrad)", (0, 0), st["DRESF"], ref, acc(K_UP) * mag, l2bar=F32_L2)
            _rounding_of_stored(rep, "c", "DRESB vs the stored DRESF", (0, 0), st["DRESB"], st["DRESF"])


def check_body_tail(st, rep):
    """Class d."""
    m = st["meta"]
    P, G = _P(st)
    nl = m["nl"]
    x, dyv = st[("HB", nl, 0)].double(), st["DRESB"].double()
    name = f"body.{nl}"
    _filter_gradient(rep, "d", "body tail", (nl, 0), G(name + ".weight", "grads0"), G(name + ".bias", "grads0"), x,
                     nchw(dyv), x.shape[0] * x.shape[1] * x.shape[2])
    if m["arch"] == "edsr" and nl != 1:
        return  # (BODY_GRAD holds another block's map by the end of the one-stage backward)
    wb = bf(P(name + ".weight"))
    rep.elem("d", "BODY_GRAD 0 (body tail dgrad, fp32)", (nl, 0), st[("BODY_GRAD", 0)], dgrad(dyv, wb),
             acc(K_CONV) * dgrad(dyv.abs(), wb.abs()), l2bar=F32_L2)
    _rounding_of_stored(rep, "d", "BODY_GRAD 1 vs the stored fp32 map", (nl, 0), st[("BODY_GRAD", 1)],
                        st[("BODY_GRAD", 0)])


def check_head(st, rep):
    """Class e."""
    P, G = _P(st)
    g = st["HEAD_GRAD"].double()
    lrd = st["lr"].double()
    gc = nchw(g)
    k = g.shape[0] * g.shape[1] * g.shape[2]
    shape = (64, lrd.shape[1], 3, 3)
    ref = torch.nn.grad.conv2d_weight(lrd, shape, gc, padding=1)
    mag = torch.nn.grad.conv2d_weight(lrd.abs(), shape, gc.abs(), padding=1)
    rep.elem("e", "head.weight", (0, 0), G("head.0.weight"), ref, acc(k) * mag, l2bar=F32_L2, per_image=False)
    rep.elem("e", "head.bias", (0, 0), G("head.0.bias"), gc.sum((0, 2, 3)), acc(k) * gc.abs().sum((0, 2, 3)),
             l2bar=F32_L2, per_image=False)


def check_edsr_blocks(st, rep):
    """Class f."""
    m = st["meta"]
    P, G = _P(st)
    dz = st["DZ"].double()
    hb0 = st[("HB", 0, 0)].double()
    k = dz.shape[0] * dz.shape[1] * dz.shape[2]
    if m["nl"] == 1:
        rs = m["res_scale"]
        g0, g1, t = st[("BODY_GRAD", 0)].double(), st[("BODY_GRAD", 1)].double(), st[("T", 0)].double()
        _filter_gradient(rep, "f", "block 0 conv2", (0, 1), G("body.0.body.2.weight"), G("body.0.body.2.bias"), t,
                         nchw(g1), k + 1, scale=rs)
        w2 = bf(P("body.0.body.2.weight"))
        mask = (t > 0).double()
        rep.bf16_map("f", "DZ", (0, 1), st["DZ"], rs * mask * dgrad(g1, w2),
                     mask * acc(K_CONV + 1) * abs(rs) * dgrad(g1.abs(), w2.abs()))
    _filter_gradient(rep, "f", "block 0 conv1", (0, 1), G("body.0.body.0.weight"), G("body.0.body.0.bias"), hb0,
                     nchw(dz), k)
    if m["nl"] == 1:
        w1 = bf(P("body.0.body.0.weight"))
        dres = st["DRESF"].double()
        rep.elem("f", "HEAD_GRAD (conv1 dgrad + BODY_GRAD 0 + DRESF)", (0, 1), st["HEAD_GRAD"],
                 dgrad(dz, w1) + g0 + dres, acc(K_CONV + 2) * (dgrad(dz.abs(), w1.abs()) + g0.abs() + dres.abs()),
                 l2bar=F32_L2)


def check_edsr_forward(st, rep):
    """Class g (EDSR, nlayers == 1)."""
    m = st["meta"]
    P, _ = _P(st)
    assert m["arch"] == "edsr" and m["nl"] == 1
    rs = m["res_scale"]
    x0 = st["X0F"].double()
    hb0, t, hb1 = st[("HB", 0, 0)], st[("T", 0)], st[("HB", 1, 0)]
    rep.add("g", "hb(0, 0) == bf16(X0F)", (0, 0), "all", 0.0 if torch.equal(st["X0F"].bfloat16(), hb0) else 1.0, 0.0)
    w1, b1 = bf(P("body.0.body.0.weight")), P("body.0.body.0.bias")
    rep.bf16_map("g", "t", (0, 1), t, conv(hb0.double(), w1, b1).clamp_min(0),
                 acc(K_CONV) * conv(hb0.double().abs(), w1.abs(), b1.abs()))
    w2, b2 = bf(P("body.0.body.2.weight")), P("body.0.body.2.bias")
    td = t.double()
    rep.bf16_map("g", "hb(1, 0)", (1, 0), hb1, rs * conv(td, w2, b2) + x0,
                 acc(K_CONV + 2) * (abs(rs) * conv(td.abs(), w2.abs(), b2.abs()) + x0.abs()))
    wb, bb = bf(P("body.1.weight")), P("body.1.bias")
    hd = hb1.double()
    rep.bf16_map("g", "RESb", (1, 0), st["RESB"], conv(hd, wb, bb) + x0,
                 acc(K_CONV + 1) * (conv(hd.abs(), wb.abs(), bb.abs()) + x0.abs()))
    cur = st["RESB"].double()
    for k in range(m["nups"]):
        wu, bu = bf(P(f"tail.0.{2 * k}.weight")), P(f"tail.0.{2 * k}.bias")
        ref = nhwc(F.pixel_shuffle(F.conv2d(nchw(cur), wu, bu, padding=1), 2))
        mag = nhwc(F.pixel_shuffle(F.conv2d(nchw(cur.abs()), wu.abs(), bu.abs(), padding=1), 2))
        rep.bf16_map("g", f"PS[{k}]", (1, k + 1), st[("PS", k)], ref, acc(K_CONV) * mag)
        cur = st[("PS", k)].double()
    wl, bl = bf(P("tail.1.weight")), P("tail.1.bias")
    rep.elem("g", "sr", (1, m["nups"] + 1), st["sr"], F.conv2d(nchw(cur), wl, bl, padding=1),
             acc(K_CONV) * F.conv2d(nchw(cur.abs()), wl.abs(), bl.abs(), padding=1), l2bar=F32_L2)


def check_all(st):
    """Every check the state's architecture has.  -> Report."""
    m = st["meta"]
    rep = Report()
    check_tail(st, rep)
    check_upsamplers(st, rep)
    check_body_tail(st, rep)
    check_head(st, rep)
    if m["arch"] == "edsr":
        check_edsr_blocks(st, rep)
        if m["nl"] == 1:
            check_edsr_forward(st, rep)
    return rep


def report_lines(rep, classes):
    """The worst figure of every kind per class, and every bias rel-L2 (the weights' would hide it)."""
    out = []
    for cls in classes:
        for kind, (ratio, row) in sorted(rep.worst(cls).items()):
            out.append(f"  ({cls}) worst {kind}: {row[4]:.3e} (bar {row[5]:.3e}) {row[1]} {row[2]} {row[3]}")
        for r in rep.rows:
            if r[0] == cls and r[1].endswith(".bias rel-L2"):
                out.append(f"  ({cls}) {r[1]}: {r[4]:.3e} (bar {r[5]:.3e}) {r[2]}")
    return out


def classes_of(case):
    m = case["meta"]
    return "abcde" + ("f" if m["arch"] == "edsr" else "") + ("g" if m["arch"] == "edsr" and m["nl"] == 1 else "")


# ------------------------------------------------------------------ the reference side
MUTATIONS = {
    1: "the tail dgrad ignores the last HR column's contribution",
    2: "the tail filter gradient drops the last pixel of the partial 32-pixel segment",
    3: "the tail dgrad uses the bf16-rounded filter instead of the fp32 master",
    4: "dy is formed with a scale off by 2^-10",
    5: "one upsampler filter gradient has two pixel-shuffle phases swapped",
    6: "DRESB is truncated instead of rounded",
    7: "the head gradient misses one 2-row band of one image",
    8: "the head bias gradient sums n - 1 images",
    9: "EDSR conv2's filter gradient is not multiplied by res_scale",
    10: "the tail bias gradient is 1 % off (its slab slot is written apart from the filter's)",
}


def _rbf(x):
    return x.float().bfloat16()


def _trunc_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits."""
    bits = x32.contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).bfloat16()


def reference_state(case, mut=0):
    """The state as an fp64 restatement of the engine leaves it: every launch in fp64 from the
    stored operands, stored as the engine stores (bf16 to nearest even for maps, fp32 for
    gradients and fp32 maps).  mut: one of MUTATIONS, applied to that launch alone -- what it
    writes is consumed downstream as it is, as on an engine."""
    m = case["meta"]
    n, nl, nups, co, rs = m["n"], m["nl"], m["nups"], m["cout"], m["res_scale"]
    st = dict(meta=m, table=case["table"], params=case["flat"], lr=case["lr"])
    P, _ = _P(st)
    grads = torch.zeros_like(case["flat"])
    tab = {name: (off, cnt) for name, off, cnt, _ in case["table"]}

    def put(name, v):
        off, cnt = tab[name]
        grads[off:off + cnt] = v.reshape(-1).float()

    # ---- forward
    x0f = nhwc(F.conv2d(case["lr"].double(), P("head.0.weight"), P("head.0.bias"), padding=1)).float()
    x0 = x0f.double()
    st["X0F"] = x0f
    if m["arch"] == "rcan":
        groups = torch.nn.Sequential(*list(case["model"].body)[:nl]).double()
        x0t = nchw(x0).requires_grad_(True)
        hbt = groups(x0t)
        hbl = _rbf(nhwc(hbt.detach()))
    else:
        cur32 = x0f
        for i in range(nl):
            hb = _rbf(cur32)
            st[("HB", i, 0)] = hb
            pre = f"body.{i}.body"
            t = _rbf(conv(hb.double(), bf(P(pre + ".0.weight")), P(pre + ".0.bias")).clamp_min(0))
            st[("T", i)] = t
            cur32 = (rs * conv(t.double(), bf(P(pre + ".2.weight")), P(pre + ".2.bias")) + cur32.double()).float()
        hbl = _rbf(cur32)
    st[("HB", nl, 0)] = hbl
    st["RESB"] = _rbf(conv(hbl.double(), bf(P(f"body.{nl}.weight")), P(f"body.{nl}.bias")) + x0)
    cur = st["RESB"].double()
    for k in range(nups):
        wu, bu = bf(P(f"tail.0.{2 * k}.weight")), P(f"tail.0.{2 * k}.bias")
        st[("PS", k)] = _rbf(nhwc(F.pixel_shuffle(F.conv2d(nchw(cur), wu, bu, padding=1), 2)))
        cur = st[("PS", k)].double()
    st["sr"] = F.conv2d(nchw(cur), bf(P("tail.1.weight")), P("tail.1.bias"), padding=1).float()
    # ---- the upstream gradient
    if m["dy_form"] == "rmse":
        hr = case["hr"]
        d = st["sr"].double() - hr.double()
        cnt = float(hr.numel())
        S = float((d * d).sum())
        L = (S / cnt) ** 0.5
        st["hr"] = hr
        st["loss4"] = torch.tensor([S, cnt, 1.0 / (cnt * L), L], dtype=torch.float32)
    else:
        st["dy"] = case["dy"]
    dy = upstream(st)
    if mut == 4:
        dy = dy * (1 + 2.0 ** -10)
    # ---- a, b: the tail conv
    dy_a = dy.clone()
    if mut == 1:
        dy_a[..., -1] = 0
    wt = P("tail.1.weight")
    st[("DPS", nups - 1)] = _rbf(dgrad(nhwc(dy_a), bf(wt) if mut == 3 else wt))
    dy_b = dy.clone()
    if mut == 2:
        assert dy.shape[3] % 64 == 32
        dy_b[..., -1] = 0
    put("tail.1.weight", wgrad(st[("PS", nups - 1)].double(), dy_b, co))
    put("tail.1.bias", dy_b.sum((0, 2, 3)) * (1.01 if mut == 10 else 1.0))
    # ---- c: the upsamplers
    for k in range(nups - 1, -1, -1):
        xin = (st["RESB"] if k == 0 else st[("PS", k - 1)]).double()
        dyc = F.pixel_unshuffle(nchw(st[("DPS", k)]), 2)
        gw = wgrad(xin, dyc, 256)
        if mut == 5 and k == 0:
            gw = gw.view(64, 4, 64, 3, 3)[:, [0, 2, 1, 3]].reshape(256, 64, 3, 3)
        put(f"tail.0.{2 * k}.weight", gw)
        put(f"tail.0.{2 * k}.bias", dyc.sum((0, 2, 3)))
        dx = nhwc(F.conv_transpose2d(dyc, bf(P(f"tail.0.{2 * k}.weight")), padding=1))
        if k > 0:
            st[("DPS", k - 1)] = _rbf(dx)
        else:
            st["DRESF"] = dx.float()
            st["DRESB"] = _trunc_bf16(st["DRESF"]) if mut == 6 else st["DRESF"].bfloat16()
    # ---- d: the body tail
    dres_b = st["DRESB"].double()
    put(f"body.{nl}.weight", wgrad(hbl.double(), nchw(dres_b), 64))
    put(f"body.{nl}.bias", dres_b.sum((0, 1, 2)))
    g0 = dgrad(dres_b, bf(P(f"body.{nl}.weight"))).float()
    st[("BODY_GRAD", 0)], st[("BODY_GRAD", 1)] = g0, g0.bfloat16()
    st["grads0"] = grads.clone()
    # ---- the body's backward down to the head's output gradient
    if m["arch"] == "rcan":
        hbt.backward(nchw(g0))
        hg = (nhwc(x0t.grad) + st["DRESF"].double()).float()
    else:
        gf = g0
        for i in range(nl - 1, -1, -1):
            pre = f"body.{i}.body"
            gb16 = gf.bfloat16().double()
            t = st[("T", i)].double()
            put(pre + ".2.weight", (1.0 if mut == 9 else rs) * wgrad(t, nchw(gb16), 64))
            put(pre + ".2.bias", rs * gb16.sum((0, 1, 2)))
            dz = _rbf(rs * (t > 0).double() * dgrad(gb16, bf(P(pre + ".2.weight"))))
            put(pre + ".0.weight", wgrad(st[("HB", i, 0)].double(), nchw(dz.double()), 64))
            put(pre + ".0.bias", dz.double().sum((0, 1, 2)))
            gf = (dgrad(dz.double(), bf(P(pre + ".0.weight"))) + gf.double() +
                  (st["DRESF"].double() if i == 0 else 0)).float()
        st["DZ"] = dz
        hg = gf
        if nl != 1:  # (what the accessor returns then: the buffer's last writer, the head's input gradient)
            st[("BODY_GRAD", 0)], st[("BODY_GRAD", 1)] = hg, hg.bfloat16()
    st["HEAD_GRAD"] = hg
    # ---- e: the head
    g = nchw(hg.double())
    gw_ = g.clone()
    if mut == 7:
        gw_[n - 1, :, 2:4, :] = 0
    put("head.0.weight", torch.nn.grad.conv2d_weight(case["lr"].double(), (64, m["cin"], 3, 3), gw_, padding=1))
    put("head.0.bias", (gw_[:n - 1] if mut == 8 else gw_).sum((0, 2, 3)))
    st["grads"] = grads
    return st


# ------------------------------------------------------------------ the engine side
def engine_state(case, dev, staged=True):
    """Run the engine on the case and read the state out of it.  RCAN, staged: forward, (RMSE:
    rmse_partial, rmse_finalize into loss4,) stage 0, clone what it left, stages 1 .. nl, clone
    HEAD_GRAD, the head's stage.  EDSR has one stage: run it, then read (staged is ignored).
    staged=False: one backward call; only "grads" and "sr" are returned."""
    from srmi.engine import Engine
    m = case["meta"]
    n, nl, nups = m["n"], m["nl"], m["nups"]
    rcan = m["arch"] == "rcan"
    lr, flat = case["lr"].to(dev), case["flat"].to(dev)
    eng = Engine(case["spec"], m["cap"], (m["h"], m["w"]), train=True, device=dev, cu_budget=m["cu"])
    eng.pack(flat)
    sr = eng.forward(flat, lr)
    st = dict(meta=m, table=case["table"], params=case["flat"], lr=case["lr"])
    if m["dy_form"] == "rmse":
        hr = case["hr"].to(dev)
        loss4 = torch.zeros(4, dtype=torch.float32, device=dev)
        eng.rmse_partial(sr, hr, loss4, float(hr.numel()))
        eng.rmse_finalize(loss4)
        kw = dict(sr=sr, hr=hr, loss4=loss4)
        st["hr"] = case["hr"]
    else:
        kw = dict(dy=case["dy"].to(dev))
        st["dy"] = case["dy"]
    grads = torch.zeros(eng.n_params, device=dev)

    def buf(*key):
        return eng.buffer(*key).cpu().clone()

    def stage0_maps():
        for k in range(nups):
            st[("DPS", k)] = buf("DPS", k)
            st[("PS", k)] = buf("PS", k)
        for key in ("DRESB", "DRESF", "RESB", "X0F"):
            st[key] = buf(key)
        st[("HB", nl, 0)] = buf("HB", nl, 0)

    if not rcan or not staged:
        eng.backward(flat, lr, grads, **kw)
        torch.cuda.synchronize()
        if rcan:
            return dict(grads=grads.cpu(), sr=sr.cpu())
        assert eng.stage_count == 1
        stage0_maps()
        st[("BODY_GRAD", 0)], st[("BODY_GRAD", 1)] = buf("BODY_GRAD", 0, 0), buf("BODY_GRAD", 0, 1)
        st["HEAD_GRAD"] = buf("HEAD_GRAD")
        st["DZ"] = buf("DZ")
        for i in range(nl):
            st[("HB", i, 0)] = buf("HB", i, 0)
            st[("T", i)] = buf("T", i, 1)
        st["grads0"] = st["grads"] = grads.cpu()
    else:
        assert eng.stage_count == nl + 2
        eng.backward(flat, lr, grads, stages=(0, 0), **kw)
        torch.cuda.synchronize()
        stage0_maps()
        st[("BODY_GRAD", 0)], st[("BODY_GRAD", 1)] = buf("BODY_GRAD", 0, 0), buf("BODY_GRAD", 0, 1)
        st["grads0"] = grads.cpu().clone()
        eng.backward(flat, lr, grads, stages=(1, nl), **kw)
        torch.cuda.synchronize()
        st["HEAD_GRAD"] = buf("HEAD_GRAD")
        same = torch.equal(eng.buffer("HEAD_GRAD"), eng.buffer("GROUP_IN_GRAD", 0))
        eng.backward(flat, lr, grads, stages=(nl + 1, nl + 1), **kw)
        torch.cuda.synchronize()
        st["head_grad_is_group_in_grad"] = same
        st["grads"] = grads.cpu()
    st["sr"] = sr.cpu()
    if m["dy_form"] == "rmse":
        st["loss4"] = kw["loss4"].cpu()
    return st
