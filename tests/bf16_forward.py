"""Per-launch closure of the bf16 engine's forward (training and inference), for
tests/test_gpu_bf16_forward.py.

Every launch's output is recomputed in fp64 on the CPU from the operands the engine itself
consumed -- its stored maps (Engine.buffer), the state the forward trace copied out between the
launches (Engine.fwd_trace / fwd_trace_view: the pair's lo8 bytes, the CA strip records, the fp32
group outputs, and an inference engine's rotating hb / t / record slots) and the master weights
rounded to bf16 where the filter pack is bf16 -- so nothing compounds and the bars are a priori,
as in bf16_stages (whose Report, acc, bf, bf16_ulp and bars this module uses):

* bf16 maps (t, u, RESb, PS[k]): Report.bf16_map with the accumulation bound acc(577 + addends)
  (|w| * |x| + |b| + |addends|).  Every kernel rounds fp32 to bf16 to nearest even (common.hpp
  f2bf and pack2, both v_cvt_pk_bf16_f32; small.hip head_fwd_kernel uses f2bf), so the bf16
  copies of fp32 maps (hb(0, 0) of X0F, hb(g + 1, 0) of the group output) are held bit for bit
  to torch's round-to-nearest-even of the engine's own fp32 map.
* fp32 outputs (X0F, the group outputs, sr): acc(K) sum |terms|.  The head reads its fp32
  weights as they are (K = 9 C + 1); the tail conv rounds its fp32 weights to bf16 (small.hip
  tail_fwd_mfma_kernel: f2bf(w[i])) and keeps its bias fp32.
* the CA strip records, per record (4 rows x one 48- or 32-column block): sums of the STORED
  bf16 t at acc(4 x 48) sum |t| where conv1 writes them (the CA inside conv2, the one-launch
  inference RCAB); sums of conv2's fp32 output against the fp64 conv at acc(577 + 4 tw) where
  conv2 writes them (the CA-pass forms).
* the CA record m | z1 | s: m per image and channel against b2 + mean(conv2_fp64(stored t)) at
  acc(577 + HW) mean(|w| * |t| + |b2|); z1 and s against the fp64 MLP of the ENGINE's m with the
  bounds carried through |W1| and |W2| (the ReLU is 1-Lipschitz, so the bottleneck's decision
  may be the engine's: where it differs from fp64's, |z1| must lie within z1's bound).  The
  sigmoid 1 / (1 + expf(-a)): expf is the ROCm device library's, documented at 1 ulp (HIP
  programming guide, "HIP math API", single precision: expf, maximum ULP error 1; the Makefile
  passes no fast-math flag, and hipcc's fp32 division is correctly rounded by default), so
  e = expf(-a) carries 2^-23 relative, the add and the division half an ulp each: s is within
  2^-22 s of sigmoid of the fp32 argument (SIG_REL), whose own bound enters through
  sigmoid' = s (1 - s) (+ its bound, for the curvature).
* the residual pair: decode(hb, lo) against h_in + s_engine u, h_in the fp32 group input or the
  decoded pair of the RCAB before, u the stored bf16 u: the fp32 rounding of the multiply-add
  (acc(2) (|s u| + |h_in|): fused or not) plus the codec's 128 fp32 steps (2^-16 |A|, 2^-142
  in the denormals), and, bit for bit, hi == (A' + 0x8000) >> 16 of the decoded bits A'.
  Inference stores no u: the reference forms x = conv2_fp64(t) + b2 and r = bf16(x).  The
  engine's u = bf16(fl(x)) with |fl(x) - x| within the accumulation bound, so it is r or, where
  x lies within that bound of the rounding boundary towards it, a bf16 neighbour of r (the
  du_from_g treatment).  Such an element is not given its ulp x s as allowance: it must match r
  or an ADMISSIBLE neighbour at that candidate's own unwidened bound -- never wider than the
  allowance, and as sharp as training on every element.  That matters because the share of
  elements with an admissible neighbour is about one half, not the 1e-3 an allowance would need
  to stay harmless: the any-order bound of a 577-term sum that cancels is about 0.4 of half a
  bf16 ulp of the result (median); the fp64 oracle alone, with no engine, shows the same share
  on the CPU.  Class "r" therefore asserts what the condition is for -- at most 1e-3 of a map
  is held to a widened bound (none is) -- and run_case reports the shares of elements with an
  admissible neighbour and of those that took one.
"""
import torch
import torch.nn.functional as F

from bf16_stages import F32_L2, K_CONV, Report, acc, bf, bf16_ulp, nchw, nhwc
from srmi.engine import Engine

SIG_REL = 2.0 ** -22    # expf 1 ulp + the add's and the division's half ulps (module docstring)
RISK_SHARE = 1e-3       # the share of a map that may be held to a widened bound in inference
FORMS = {0: "CA pass", 1: "CA inside conv2", 2: "one-launch RCAB"}


def conv(x, w, b=None):
    """conv2d(., w, padding=1) + b: x NHWC fp64 -> NHWC."""
    return nhwc(F.conv2d(nchw(x), w, b, padding=1))


def conv_abs(x, w, b=None):
    return conv(x.abs(), w.abs(), None if b is None else b.abs())


def hi_bits(hi):
    """The 16 bits of a bf16 tensor as int64."""
    return hi.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def decode_bits(hi, lo):
    """The fp32 bit pattern A' of the residual pair (test_gpu_kernels.lo8_decode's formula,
    csrc/common.hpp pair_decode4): ((hi << 16) | 0x80) + (sext8(lo) << 8), as int64 in [0, 2^32)."""
    q = lo.contiguous().view(torch.int8).to(torch.int64)
    return (((hi_bits(hi) << 16) | 0x80) + (q << 8)) & 0xFFFFFFFF


def bits_to_f64(bits):
    return torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32).double()


def strips(x, tw):
    """[n, h, w, 64] -> [n, (h / 4) (w / tw), 64]: strip record k nsx + j."""
    n, h, w, _ = x.shape
    return x.view(n, h // 4, 4, w // tw, tw, 64).sum((2, 4)).reshape(n, -1, 64)


def u_from_t(x, accb):
    """The bf16 numbers the engine's u = bf16(fl(x)) can be, given the exact conv2 output x and
    the bound accb on |fl(x) - x|, among r = bf16(x) and its two neighbours: [(candidate,
    admissible)] with r first (always admissible).  A neighbour is admissible where x lies within
    accb of the rounding boundary between r and it."""
    r = bf(x)
    ulp = bf16_ulp(r)
    ra, sg = r.abs(), torch.sign(r)
    pow2 = ra == torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.floor(torch.log2(ra.clamp_min(2.0 ** -126))))
    down = torch.where(pow2, ulp / 2, ulp)     # towards zero of a power of two the spacing halves
    off = x.abs() - ra                         # > 0: x lies on the far side of r
    nz = r != 0
    out = [(r, torch.ones_like(nz))]
    eps = ulp * 2.0 ** -30                     # (a tie at the boundary itself, to fp64 rounding)
    out.append((sg * (ra + ulp), nz & (ulp / 2 - off <= accb + eps)))
    out.append((sg * (ra - down), nz & (down / 2 + off <= accb + eps)))
    return out


def run_case(case, dev, train=True, capacity=None):
    """One forward with the forward trace on; every check of the module docstring.
    -> (Report, info)."""
    nl, nb, (h, w), n = case["nl"], case["nb"], case["hw"], case["B"]
    HW = h * w
    cr = 64 // case["cb"]
    tw = 48 if w % 48 == 0 else 32
    lr, flat = case["lr"].to(dev), case["flat"].to(dev)
    eng = Engine(case["spec"], capacity or n, (h, w), train=train, device=dev, cu_budget=case["cu_budget"])
    eng.pack(flat)
    eng.fwd_trace(True)
    sr = eng.forward(flat, lr)
    torch.cuda.synchronize()
    form = eng.probe(8)
    tab = {name: (off, cnt, shape) for name, off, cnt, shape in case["table"]}
    prm = case["flat"].double()

    def P(name):
        off, cnt, shape = tab[name]
        return prm[off:off + cnt].view(shape)

    def tv(name, g, b=0):
        return eng.fwd_trace_view(name, g, b).cpu()

    def saved(name, g, b):   # a train engine keeps these maps; an inference engine's slots rotate
        return (eng.buffer(name, g, b) if train else eng.fwd_trace_view(name, g, b)).cpu()

    rep = Report()
    info = dict(form=form, n=n, capacity=capacity or n)
    lrd = case["lr"].double()
    x0f = eng.buffer("X0F").cpu()
    # ---- a. the head (fp32 weights as they are)
    wh, bh = P("head.0.weight"), P("head.0.bias")
    ref = nhwc(F.conv2d(lrd, wh, bh, padding=1))
    mag = nhwc(F.conv2d(lrd.abs(), wh.abs(), bh.abs(), padding=1))
    rep.elem("a", "X0F", (0, 0), x0f, ref, acc(9 * lrd.shape[1] + 1) * mag, l2bar=F32_L2)
    hb00 = saved("HB", 0, 0)
    rep.add("a", "hb(0, 0) == bf16(X0F)", (0, 0), "all", 0.0 if torch.equal(x0f.bfloat16(), hb00) else 1.0, 0.0)

    rin = x0f.double()
    for g in range(nl):
        pre = f"body.{g}.body"
        h_prev_bits = None
        for b in range(1, nb + 1):
            rp = f"{pre}.{b - 1}.body"
            hin_b = saved("HB", g, b - 1)
            t = saved("T", g, b)
            td = t.double()
            # ---- b. conv1: t = bf16(relu(conv(hb) + b1)); its strip sums where conv1 writes them
            w1c, b1c = bf(P(f"{rp}.0.weight")), P(f"{rp}.0.bias")
            ref = conv(hin_b.double(), w1c, b1c).clamp_min(0)
            rep.bf16_map("b", "t", (g, b), t, ref, acc(K_CONV) * conv_abs(hin_b.double(), w1c, b1c))
            ppool = tv("PPOOL", g, b).double()
            if form != 0:
                rep.elem("b", "strip sums of the stored t", (g, b), ppool, strips(td, tw), acc(4 * tw) * strips(td.abs(), tw))
            # ---- c. the CA scale: m from the stored t, the MLP from the engine's m
            w2c, b2c = bf(P(f"{rp}.2.weight")), P(f"{rp}.2.bias")
            x = conv(td, w2c, b2c)                  # conv2's exact output
            xa = conv_abs(td, w2c, b2c)
            # (the records are written densely: m | z1 | s of image i at i (128 + CR))
            rec = saved("REC", g, b).reshape(-1)[:n * (128 + cr)].view(n, 128 + cr).double()
            m, z1, s = rec[:, :64], rec[:, 64:64 + cr], rec[:, 64 + cr:]
            if form == 0:
                rep.elem("c", "strip sums of conv2's fp32 output", (g, b), ppool, strips(x, tw),
                         acc(K_CONV + 4 * tw) * strips(xa, tw))
            rep.elem("c", "m", (g, b), m, x.mean((1, 2)), acc(K_CONV + HW) * xa.mean((1, 2)))
            W1, B1 = P(f"{rp}.3.conv_du.0.weight").view(cr, 64), P(f"{rp}.3.conv_du.0.bias")
            W2, B2 = P(f"{rp}.3.conv_du.2.weight").view(64, cr), P(f"{rp}.3.conv_du.2.bias")
            z1r = m @ W1.t() + B1
            tz = acc(65) * (m.abs() @ W1.abs().t() + B1.abs())
            rep.elem("c", "z1", (g, b), z1, z1r, tz)
            flip = (z1 > 0) != (z1r > 0)
            rep.add("c", "|z1| / bound where the ReLU decision differs from fp64's", (g, b), "all",
                    float((z1r.abs() / tz)[flip].max()) if bool(flip.any()) else 0.0, 1.0)
            hid = z1r.clamp_min(0)
            a = hid @ W2.t() + B2
            ta = acc(cr + 1) * (hid @ W2.abs().t() + B2.abs()) + tz @ W2.abs().t()
            sr_ = torch.sigmoid(a)
            rep.elem("c", "s", (g, b), s, sr_, (sr_ * (1 - sr_) + ta) * ta + SIG_REL * sr_)
            # ---- d. conv2 (training: u is stored)
            accu = acc(K_CONV) * xa
            if train:
                u = eng.buffer("U", g, b).cpu()
                rep.bf16_map("d", "u", (g, b), u, x, accu)
                cands = [(u.double(), None)]
            else:
                cands = u_from_t(x, accu)
            # ---- e. the pair: decode(hb, lo) = h_in + s u; hi = the decoded value's bf16 half away
            hb_b, lo = saved("HB", g, b), tv("LO", g, b)
            bits = decode_bits(hb_b, lo)
            got = bits_to_f64(bits)
            hin = rin if b == 1 else bits_to_f64(h_prev_bits)
            sv = s[:, None, None, :]

            def pair_tol(ud):   # the multiply-add's fp32 rounding + the codec's 128 fp32 steps
                ref = hin + sv * ud
                tfp = acc(2) * ((sv * ud).abs() + hin.abs())
                return ref, tfp + (1 + 2.0 ** -15) * 2.0 ** -16 * (ref.abs() + tfp) + 2.0 ** -142

            ref, tol = pair_tol(cands[0][0])
            err = (got - ref).abs()
            tol_r, took = tol, torch.zeros_like(err, dtype=torch.bool)
            for ud, ok in cands[1:]:   # inference: the admissible neighbour that fits best, at ITS bound
                ref_c, tol_c = pair_tol(ud)
                err_c = (got - ref_c).abs()
                better = ok & (err_c / tol_c < err / tol)
                err, tol, took = torch.where(better, err_c, err), torch.where(better, tol_c, tol), took | better
            if not train:
                several = cands[1][1] | cands[2][1]
                # the allowance this check gives: none.  A neighbour is held to ITS OWN bound, which
                # differs from r's by one bf16 step of u times s times the bound's own 2^-16 + acc(2)
                widened = tol > tol_r + (acc(2) + 2.0 ** -15) * sv.abs() * bf16_ulp(cands[0][0])
                for i in range(n):
                    rep.add("r", "share of elements given a widened bound", (g, b), f"image {i}",
                            float(widened[i].double().mean()), RISK_SHARE)
                info.setdefault("several_roundings_possible", []).append(float(several.double().mean()))
                info.setdefault("neighbour_taken", []).append(float(took.double().mean()))
            rep.elem("e", "pair", (g, b), err, torch.zeros_like(err), tol)
            rep.add("e", "hi == (A' + 0x8000) >> 16", (g, b), "all",
                    0.0 if torch.equal(((bits + 0x8000) & 0xFFFFFFFF) >> 16, hi_bits(hb_b)) else 1.0, 0.0)
            h_prev_bits = bits
        # ---- f. the group tail: the fp32 group output and its bf16 copy
        wt, bt = bf(P(f"{pre}.{nb}.weight")), P(f"{pre}.{nb}.bias")
        hl = saved("HB", g, nb).double()
        rf = tv("RF", g)
        ref = conv(hl, wt, bt) + rin
        rep.elem("f", "group output (fp32)", (g, nb + 1), rf, ref, acc(K_CONV + 1) * (conv_abs(hl, wt, bt) + rin.abs()),
                 l2bar=F32_L2)
        rep.add("f", "hb(g + 1, 0) == bf16(group output)", (g, nb + 1), "all",
                0.0 if torch.equal(rf.bfloat16(), saved("HB", g + 1, 0)) else 1.0, 0.0)
        rin = rf.double()
    # ---- g. the body tail, the upsamplers, the tail conv
    wb_, bb_ = bf(P(f"body.{nl}.weight")), P(f"body.{nl}.bias")
    hl = saved("HB", nl, 0).double()
    resb = eng.buffer("RESB").cpu()
    x0d = x0f.double()
    rep.bf16_map("g", "RESb", (nl, 0), resb, conv(hl, wb_, bb_) + x0d,
                 acc(K_CONV + 1) * (conv_abs(hl, wb_, bb_) + x0d.abs()))
    cur = resb.double()
    nups = sum(1 for name in tab if name.startswith("tail.0.") and name.endswith(".weight"))
    for k in range(nups):
        wu, bu = bf(P(f"tail.0.{2 * k}.weight")), P(f"tail.0.{2 * k}.bias")
        ps = eng.buffer("PS", k).cpu()
        ref = nhwc(F.pixel_shuffle(F.conv2d(nchw(cur), wu, bu, padding=1), 2))
        mag = nhwc(F.pixel_shuffle(F.conv2d(nchw(cur.abs()), wu.abs(), bu.abs(), padding=1), 2))
        rep.bf16_map("g", f"PS[{k}]", (nl, k + 1), ps, ref, acc(K_CONV) * mag)
        cur = ps.double()
    wl, bl = bf(P("tail.1.weight")), P("tail.1.bias")
    ref = F.conv2d(nchw(cur), wl, bl, padding=1)
    mag = F.conv2d(nchw(cur.abs()), wl.abs(), bl.abs(), padding=1)
    rep.elem("g", "sr", (nl, nups + 1), sr.cpu(), ref, acc(K_CONV) * mag, l2bar=F32_L2)
    eng.fwd_trace(False)
    return rep, info


def trace_changes_nothing(case, dev, train):
    """Forward with the forward trace off, on, and off again on one engine: [(what, run)] for
    every output or persisting map that is not bit-identical to the first run's, and whether the
    trace buffer was written while on and left alone while off."""
    nl, nb, hw, n = case["nl"], case["nb"], case["hw"], case["B"]
    lr, flat = case["lr"].to(dev), case["flat"].to(dev)
    eng = Engine(case["spec"], n, hw, train=train, device=dev, cu_budget=case["cu_budget"])
    eng.pack(flat)
    keys = [("X0F", 0, 0), ("RESB", 0, 0), ("PS", 0, 0), ("PS", 1, 0)]
    if train:
        keys += [("HB", nl, 0)] + [("HB", g, b) for g in range(nl) for b in range(nb + 1)]
        keys += [(k, g, b) for k in ("T", "U", "REC") for g in range(nl) for b in range(1, nb + 1)]
    runs, buf, written = [], None, None
    for on in (False, True, False):
        if on:
            buf = eng.fwd_trace(True)
        elif runs:
            eng.fwd_trace(False)
            buf.zero_()
        out = eng.forward(flat, lr)
        torch.cuda.synchronize()
        runs.append({("sr", 0, 0): out.clone(), **{k: eng.buffer(*k).clone() for k in keys}})
        if on:
            written = bool(buf.any())
    differ = [(k, i) for i, r in enumerate(runs[1:], start=1) for k, v in r.items() if not torch.equal(v, runs[0][k])]
    return differ, written, not bool(buf.any())
