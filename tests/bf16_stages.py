"""Per-launch closure of the bf16 engine's RCAB backward, for tests/test_gpu_bf16_stages.py.

Every launch of a residual group's backward stage is recomputed in fp64 on the CPU from the
operands the engine itself consumed -- its saved forward maps (Engine.buffer), the in-group
state the backward trace copied out between the launches (Engine.trace / trace_view), and the
master weights rounded to bf16 as the filter packs are -- so the only admissible difference is
that launch's own output rounding and its fp32 accumulation.  Errors do not compound and the
ReLU decisions are the engine's own (its t), so the bars are a priori:

* bf16 maps: |got - ref| <= 2^-7 |ref| (one bf16 ulp: round-to-nearest's half ulp, and a sum
  that lands on the other side of a rounding boundary) + acc(K) (|w| * |x| + |addends|), with
  acc(K) = 2 gamma_K, gamma_K = K u / (1 - K u), u = 2^-24: the any-order bound of a K-term fp32
  sum (Higham, eq. 3.5) built as fp32_stages.Z_TOL is, K = 577 + the addends; and the
  project's bf16 bar of 4e-3 rel-L2 per image.  No element is excluded.  That bound lets any
  element be a whole ulp off, so the maps are also held to what round-to-nearest of an fp32
  sum can give: |got - unrounded ref| <= half the bf16 ulp of got + the same accumulation bound.
* the CA sums are checked per strip record (4 rows x one 48- or 32-column block, K = its
  pixels) against the sums of the STORED bf16 stream, not only as image totals.
* fp32 outputs: acc(K) sum |terms|, K the number of terms; relative to sum |terms|, never to
  the (possibly cancelling) result.
* filter gradients from bf16 partial slabs (one per image, row chunk and 48-column block;
  pack2 in csrc/common.hpp is __builtin_convertvector, round to nearest even): elementwise the
  sum over the partials of half a bf16 ulp of the partial as the fp32 sum gives it (2^-8 (|P| +
  its fp32 bound)) + the fp32 bound; rel-L2 <= 2 x sqrt(sum_p sum_e ulp(P_pe)^2 / 12) / ||ref||
  + 1e-5 (the variance of round-to-nearest, partials taken as independent).  fp32 slabs (the
  group tail's, and every launch at tiles that are no multiple of 48 wide): the fp32 bound and
  1e-5 rel-L2 (test_wgrad's bar).
* where the fused conv2 backward forms du = bf16(g s + dm / HW) itself (it is then never in
  memory) the reference forms it in fp64; an element whose exact value lies within the fp32
  error (3 u (|g s| + |dm / HW|)) of a bf16 rounding boundary may come out one ulp away in the
  engine, so those elements' ulp, passed through |w| (dgrad) or |t| (filter gradient), is
  added to the bound.  Everywhere else du is the engine's own traced map.
"""
import dataclasses
import math

import torch
import torch.nn.functional as F

import fp32_stages as fs
from srmi.engine import Engine

U32 = 2.0 ** -24
BF_ULP = 2.0 ** -7      # one bf16 ulp of x is at most 2^-7 |x|
BF16_L2 = 4e-3          # TOL["bf16"] of test_gpu_kernels.py
F32_L2 = 1e-5           # TOL["fp32"], test_wgrad's bar
K_CONV = 64 * 9 + 1     # fp32_stages._K


def acc(k):
    """Twice the any-order bound gamma_K of a K-term fp32 sum (as fp32_stages.Z_TOL)."""
    return 2 * k * U32 / (1 - k * U32)


def bf(x):
    return x.float().bfloat16().double()


def nchw(x):
    return x.double().permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def dgrad(dy, w):
    """The input gradient of conv2d(., w, padding=1): dy NHWC fp64 -> NHWC."""
    return nhwc(F.conv_transpose2d(nchw(dy), w, padding=1))


def bf16_ulp(x):
    """The spacing of bf16 numbers at |x| (x fp64, nonzero where it matters)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


def du_from_g(g, s, dm, hw):
    """du = bf16(g s + dm / HW) in fp64 from the engine's stream and records.  -> (du, risk):
    risk = the bf16 ulp of the elements whose exact value lies within 3 u (|g s| + |dm / HW|)
    of a rounding boundary (the engine's fp32 fma of the fp32 dm / HW may round those to the
    neighbouring bf16 number), 0 elsewhere."""
    a = g.double() * s[:, None, None, :]
    c = (dm / hw)[:, None, None, :].expand_as(a)
    x = a + c
    r = bf(x)
    ulp = bf16_ulp(r)
    d = (x - r).abs()
    pow2_below = (r.abs() == torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.floor(torch.log2(
        r.abs().clamp_min(2.0 ** -126))))) & (x.abs() < r.abs())
    to_boundary = torch.where(pow2_below, ulp / 4 - d, ulp / 2 - d)
    risk = torch.where(to_boundary <= 3 * U32 * (a.abs() + c.abs()), ulp, torch.zeros_like(ulp))
    return r, risk


def chunks(n, h, w, rs):
    """The partial slabs of a 48-wide filter-gradient launch: (image, rows, columns)."""
    hr = h // rs
    return [(i, k * hr, (k + 1) * hr, x0, x0 + 48) for i in range(n) for k in range(rs) for x0 in range(0, w, 48)]


def wgrad_partials(x, dy, parts):
    """x, dy NHWC fp64 -> [len(parts), 64, 64, 3, 3]: each part's share of the filter gradient."""
    xp = F.pad(nchw(x), (1, 1, 1, 1))
    dyc = nchw(dy)
    out = []
    for i, y0, y1, x0, x1 in parts:
        out.append(torch.nn.grad.conv2d_weight(xp[i:i + 1, :, y0:y1 + 2, x0:x1 + 2], (64, 64, 3, 3),
                                               dyc[i:i + 1, :, y0:y1, x0:x1], padding=0))
    return torch.stack(out)


class Report:
    """The outcome of every check of one case: rows (class, what, (g, b), image, figure, bar,
    ok).  `figure` is the worst |got - ref| / bound of an elementwise check (bar 1) or a
    rel-L2 (its bar)."""

    def __init__(self):
        self.rows = []

    def add(self, cls, what, gb, image, figure, bar):
        self.rows.append((cls, what, gb, image, float(figure), float(bar), bool(figure <= bar)))

    def elem(self, cls, what, gb, got, ref, tol, l2bar=None, per_image=True):
        """Elementwise |got - ref| <= tol (every element) and, l2bar, rel-L2 <= l2bar; per image
        (dim 0) or over the whole tensor."""
        got, ref = got.double(), ref.double()
        tol = tol + 1e-300
        sl = [(f"image {n}", slice(n, n + 1)) for n in range(ref.shape[0])] if per_image else [("all", slice(None))]
        for name, s in sl:
            self.add(cls, what + " elementwise/bound", gb, name, ((got[s] - ref[s]).abs() / tol[s]).max(), 1.0)
            if l2bar is not None:
                self.add(cls, what + " rel-L2", gb, name, fs.rel_l2(got[s], ref[s]), l2bar)

    def bf16_map(self, cls, what, gb, got, ref, accb):
        """A bf16 map against its unrounded fp64 reference `ref`: one bf16 ulp of ref + accb
        against the rounded reference and 4e-3 rel-L2, and round-to-nearest's half ulp + accb."""
        self.elem(cls, what, gb, got, bf(ref), BF_ULP * ref.abs() + accb, l2bar=BF16_L2)
        self.elem(cls, what + " (to nearest)", gb, got, ref, bf16_ulp(got.double()) / 2 + accb)

    def failures(self, cls):
        return [r[:6] for r in self.rows if r[0] == cls and not r[6]]

    def worst(self, cls):
        """{kind of figure: (worst figure / bar, row)} of a class."""
        out = {}
        for r in self.rows:
            if r[0] != cls:
                continue
            kind = "rel-L2" if r[1].endswith("rel-L2") else "elementwise/bound"
            ratio = r[4] / r[5] if r[5] else (math.inf if r[4] else 0.0)  # (bar 0: a bit-identity check)
            if kind not in out or ratio > out[kind][0]:
                out[kind] = (ratio, r[:6])
        return out


def make_case(hw, cb, B, cu_budget=0, flags=0, nl=2, nb=3):
    case = fs.make_case(nl, nb, cb, hw, B=B, C=1)
    case["spec"] = dataclasses.replace(case["spec"], dtype="bf16", flags=flags)
    case["cu_budget"] = cu_budget
    case["cb"] = cb
    return case


def _records(eng, g, b, n, cr):
    """(m, z1, s) of REC(g, b) and (dz2, dz1, conv2 bias gradient, dm) of BREC(g, b), each [n, .]."""
    per = 128 + cr
    rec = eng.buffer("REC", g, b).reshape(-1)[:n * per].view(n, per).double().cpu()
    raw = eng.buffer("BREC", g, b).reshape(-1).double().cpu()
    br = raw[:n * per].view(n, per)
    dm = raw[n * per:n * per + n * 64].view(n, 64)
    return (rec[:, :64], rec[:, 64:64 + cr], rec[:, 64 + cr:]), (br[:, :64], br[:, 64:64 + cr], br[:, 64 + cr:], dm)


def run_case(case, dev):
    """Forward, then the backward one stage at a time with the trace on; every check of the
    module docstring.  -> (Report, info)."""
    nl, nb, (h, w), n = case["nl"], case["nb"], case["hw"], case["B"]
    assert nl >= 2  # (the fp32 group output gradient is read through the alternating buffers)
    HW = h * w
    cr = 64 // case["cb"]
    lr, dy, flat = case["lr"].to(dev), case["dy"].to(dev), case["flat"].to(dev)
    eng = Engine(case["spec"], n, (h, w), train=True, device=dev, cu_budget=case["cu_budget"])
    eng.pack(flat)
    eng.forward(flat, lr)
    eng.trace(True)
    torch.cuda.synchronize()
    rs1, rs2, mode = eng.probe(5), eng.probe(6), None
    saved = [("HB", nl, 0)] + [("HB", g, b) for g in range(nl) for b in range(nb + 1)]
    saved += [(k, g, b) for k in ("T", "U", "REC") for g in range(nl) for b in range(1, nb + 1)]
    snap = {k: eng.buffer(*k).clone() for k in saved}
    grads = torch.zeros(eng.n_params, device=dev)
    clobbered, gout, gin = [], {}, {}
    for s in range(nl + 2):
        if 1 <= s <= nl:
            # the fp32 gradient w.r.t. group g's output, before g's stage: group g + 1's input
            # gradient, or for the last group the body tail's dgrad, which lies in the buffer
            # group g - 1's input gradient goes to later (the two fp32 streams alternate)
            g = nl - s
            gout[g] = eng.buffer("GROUP_IN_GRAD", g + 1 if g + 1 < nl else g - 1).double().cpu()
        eng.backward(flat, lr, grads, dy=dy, stages=(s, s))
        torch.cuda.synchronize()
        if mode is None:
            mode = eng.probe(7)
        clobbered += [(k, f"stage {s}") for k, v in snap.items() if not torch.equal(eng.buffer(*k), v)]
        if 1 <= s <= nl:
            gin[nl - s] = eng.buffer("GROUP_IN_GRAD", nl - s).cpu()
    fused, slab16, du_fused = bool(mode & 1), bool(mode & 2), bool(mode & 4)
    dresf = eng.buffer("DRESF").double().cpu()
    grads = grads.double().cpu()
    tab = {name: (off, cnt, shape) for name, off, cnt, shape in case["table"]}
    prm = case["flat"].double()

    def P(name):
        off, cnt, shape = tab[name]
        return prm[off:off + cnt].view(shape)

    def G(name):
        off, cnt, shape = tab[name]
        return grads[off:off + cnt].view(shape)

    def tr(name, g, b=0):
        return eng.trace_view(name, g, b).double().cpu()

    def buf(name, g, b):
        return eng.buffer(name, g, b).double().cpu()

    rep = Report()
    info = dict(rs1=rs1, rs2=rs2, fused=fused, slab16=slab16, du_fused=du_fused, clobbered=clobbered)
    ones = torch.ones(n, dtype=torch.float64)

    def filter_gradient(cls, what, gb, name, x, dyv, rs, bf16_slabs, extra=None):
        """The filter gradient `name` against the fp64 partials of (x, dyv) (module docstring);
        extra: an additional elementwise allowance."""
        got = G(name)
        if bf16_slabs:
            parts = chunks(n, h, w, rs)
            Pp = wgrad_partials(x, dyv, parts)
            k = (h // rs) * 48 + len(parts)
            Ap = acc(k) * wgrad_partials(x.abs(), dyv.abs(), parts)
            ref = Pp.sum(0)
            tol = (2.0 ** -8 * (Pp.abs() + Ap) + Ap).sum(0)
            model = math.sqrt(float((bf16_ulp(Pp) ** 2 / 12).sum())) / float(ref.norm())
            l2 = 2 * model + 1e-5
        else:
            ref = torch.nn.grad.conv2d_weight(nchw(x), (64, 64, 3, 3), nchw(dyv), padding=1)
            tol = acc(n * HW) * torch.nn.grad.conv2d_weight(nchw(x.abs()), (64, 64, 3, 3), nchw(dyv.abs()), padding=1)
            l2 = F32_L2
        if extra is not None:
            tol = tol + extra
        rep.elem(cls, what, gb, got, ref, tol, l2bar=l2, per_image=False)

    def ca_sums(cls, gb, pacc, stream, u):
        """pacc [n, nstrips, 128] against the sums of the STORED stream and stream * u."""
        tw = 48 if w % 48 == 0 else 32

        def strips(x):  # [n, h, w, 64] -> [n, (h / 4) (w / tw), 64]: strip record k nsx + j
            return x.view(n, h // 4, 4, w // tw, tw, 64).sum((2, 4)).reshape(n, -1, 64)

        for what, col, terms in (("sum g", slice(0, 64), stream), ("sum g u", slice(64, 128), stream * u)):
            rep.elem(cls, f"pacc {what}", gb, pacc[:, :, col].sum(1), terms.sum((1, 2)),
                     acc(HW) * terms.abs().sum((1, 2)))
            rep.elem(cls, f"pacc {what} per strip", gb, pacc[:, :, col], strips(terms), acc(4 * tw) * strips(terms.abs()))

    for g in range(nl):
        pre = f"body.{g}.body"
        grb = tr("GRB", g)
        # the bf16 copy of the group output gradient is the rounding of the fp32 one
        rep.add("e", "GRB == bf16(group output gradient)", (g, nb + 1), "all",
                0.0 if torch.equal(bf(gout[g]), grb) else 1.0, 0.0)
        # ---- a. the group tail: epilogue 12 beside its filter gradient (fp32 slabs)
        wt = bf(P(f"{pre}.{nb}.weight"))
        s0 = tr("STREAM", g, nb)
        ref = dgrad(grb, wt)
        rep.bf16_map("a", "stream after the group tail", (g, nb + 1), s0, ref,
                     acc(K_CONV) * dgrad(grb.abs(), wt.abs()))
        ca_sums("a", (g, nb + 1), tr("PACC", g, nb), s0, buf("U", g, nb))
        filter_gradient("a", "group tail gw", (g, nb + 1), f"{pre}.{nb}.weight", buf("HB", g, nb), grb, rs1, False)
        rep.elem("a", "group tail gb", (g, nb + 1), G(f"{pre}.{nb}.bias"), grb.sum((0, 1, 2)),
                 acc(n * HW) * grb.abs().sum((0, 1, 2)), per_image=False)
        for b in range(nb, 0, -1):
            rp = f"{pre}.{b - 1}.body"
            gs = tr("STREAM", g, b)      # the gradient w.r.t. RCAB b's output: its backward's input
            pacc = tr("PACC", g, b)
            (m, z1, sv), (dz2, dz1, db2, dm) = _records(eng, g, b, n, cr)
            w1, w2 = P(f"{rp}.3.conv_du.0.weight").view(cr, 64), P(f"{rp}.3.conv_du.2.weight").view(64, cr)
            ns = pacc.shape[1]
            # ---- b. the CALayer backward's MLP inside F2, from pacc, REC and the fp32 w1, w2
            Gs, ds = pacc[:, :, :64].sum(1), pacc[:, :, 64:].sum(1)
            Ga, dsa = pacc[:, :, :64].abs().sum(1), pacc[:, :, 64:].abs().sum(1)
            dz2r = ds * sv * (1 - sv)
            t2 = acc(ns + 3) * dsa * (sv * (1 - sv)).abs()
            on = (z1 > 0).double()
            dz1r = on * (dz2r @ w2)
            t1 = on * (acc(64) * (dz2r.abs() @ w2.abs()) + t2 @ w2.abs())
            dmr = dz1r @ w1
            tm = acc(cr) * (dz1r.abs() @ w1.abs()) + t1 @ w1.abs()
            db2r = sv * Gs + dmr
            tb = acc(ns + 3) * (sv.abs() * Ga + dmr.abs()) + tm
            for what, got, ref, tol in (("dz2", dz2, dz2r, t2), ("dz1", dz1, dz1r, t1), ("dm", dm, dmr, tm),
                                        ("conv2 bias-gradient segment", db2, db2r, tb)):
                rep.elem("b", f"BREC {what}", (g, b), got, ref, tol)
            # ---- c. F2's dgrad role: du from the stream, then the ReLU-mask dgrad of conv2
            t, wc2 = buf("T", g, b), bf(P(f"{rp}.2.weight"))
            du_ref, risk = du_from_g(gs, sv, dm, HW)
            if du_fused:
                du, spill_c = du_ref, dgrad(risk, wc2.abs())
                spill_d = torch.nn.grad.conv2d_weight(nchw(t.abs()), (64, 64, 3, 3), nchw(risk), padding=1)
            else:  # the engine wrote du: hold it to the reference, then close over the engine's own
                du, spill_c, spill_d = tr("DU", g, b), 0.0, None
                x = gs * sv[:, None, None, :] + (dm / HW)[:, None, None, :]
                rep.bf16_map("c", "du", (g, b), du, x, acc(3) * (
                    (gs * sv[:, None, None, :]).abs() + (dm / HW).abs()[:, None, None, :]))
            mask = (t > 0).double()
            ref = dgrad(du, wc2) * mask
            dz = tr("DZ", g, b)
            rep.bf16_map("c", "dz", (g, b), dz, ref, mask * (acc(K_CONV) * dgrad(du.abs(), wc2.abs()) + spill_c))
            # ---- d. F2's filter role: the only observation of the du that role forms
            filter_gradient("d", "conv2 gw", (g, b), f"{rp}.2.weight", t, du, rs2, slab16, extra=spill_d)
            # the engine takes conv2's bias gradient from the records: s sum g + dm, which is
            # sum_p (g s + dm / HW) before du's rounding; against the sum of the ROUNDED du the
            # roundings themselves (half an ulp each) are part of the bound
            x = gs * sv[:, None, None, :] + (dm / HW)[:, None, None, :]
            tgb = ones @ (acc(HW + 3) * (sv.abs() * gs.abs().sum((1, 2)) + dm.abs())) + acc(n) * db2.abs().sum(0)
            rep.elem("d", "conv2 gb vs sum of unrounded du", (g, b), G(f"{rp}.2.bias"), x.sum((0, 1, 2)), tgb,
                     per_image=False)
            rep.elem("d", "conv2 gb vs sum of du", (g, b), G(f"{rp}.2.bias"), du.sum((0, 1, 2)),
                     tgb + 2.0 ** -8 * x.abs().sum((0, 1, 2)), per_image=False)
            # ---- e. F1: conv1's dgrad into the stream (epilogue 11) or the group input gradient (13)
            wc1 = bf(P(f"{rp}.0.weight"))
            so = tr("STREAM", g, b - 1)
            if b > 1:
                ref = dgrad(dz, wc1) + gs
                rep.bf16_map("e", "stream after F1", (g, b), so, ref,
                             acc(K_CONV + 1) * (dgrad(dz.abs(), wc1.abs()) + gs.abs()))
                ca_sums("e", (g, b), tr("PACC", g, b - 1), so, buf("U", g, b - 1))
            else:
                adds = [gs, gout[g]] + ([dresf] if g == 0 else [])
                ref = dgrad(dz, wc1) + sum(adds)
                rep.elem("e", "group input gradient (fp32)", (g, b), gin[g], ref, acc(K_CONV + len(adds)) * (
                    dgrad(dz.abs(), wc1.abs()) + sum(a.abs() for a in adds)), l2bar=F32_L2)
                rep.add("e", "stream == bf16(group input gradient)", (g, b), "all",
                        0.0 if torch.equal(bf(gin[g]), so) else 1.0, 0.0)
            filter_gradient("e", "conv1 gw", (g, b), f"{rp}.0.weight", buf("HB", g, b - 1), dz, rs1, slab16)
            rep.elem("e", "conv1 gb", (g, b), G(f"{rp}.0.bias"), dz.sum((0, 1, 2)),
                     acc(n * HW) * dz.abs().sum((0, 1, 2)), per_image=False)
            # ---- f. the CA parameter gradients of this RCAB's slot, from REC / BREC over the images
            hid = z1.clamp_min(0)
            for key, got, ref, mag in (
                    ("0.weight", G(f"{rp}.3.conv_du.0.weight").view(cr, 64), dz1.t() @ m, dz1.abs().t() @ m.abs()),
                    ("0.bias", G(f"{rp}.3.conv_du.0.bias"), dz1.sum(0), dz1.abs().sum(0)),
                    ("2.weight", G(f"{rp}.3.conv_du.2.weight").view(64, cr), dz2.t() @ hid, dz2.abs().t() @ hid),
                    ("2.bias", G(f"{rp}.3.conv_du.2.bias"), dz2.sum(0), dz2.abs().sum(0)),
                    ("conv2 bias", G(f"{rp}.2.bias"), db2.sum(0), db2.abs().sum(0))):
                rep.elem("f", f"conv_du.{key}" if key[0] in "02" else key, (g, b), got, ref, acc(n + 1) * mag,
                         per_image=False)
    eng.trace(False)
    return rep, info
