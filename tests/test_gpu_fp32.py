"""The exact-fp32 engine mode (SRMI_DTYPE_F32, v_mfma_f32_16x16x4_f32) against the
reference's own fp32/fp64 arithmetic: north-star "outputs match the reference
PyTorch model on identical inputs within 1e-5 relative fp32" and BASELINE config
4 (EDSR x8, fp32).

Tolerances (measured on the reference): its fp32 forward drifts
5.5e-7 rel-L2 from fp64 and its loss 1.5e-8, so outputs are held to 1e-5 rel-L2
and losses to 1e-5 rel; its fp32 parameter gradients drift up to 3.3e-4 rel-L2 per
tensor from fp64, so gradients are held to 1e-3 rel-L2 per tensor."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_oracle import exact_fp32  # noqa: E402
from oracle import rcan_oracle as ro  # noqa: E402
from srmi.engine import Engine, NetSpec, downsample, param_table  # noqa: E402
from srmi.trainer import FusedTrainer  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def rel_l2(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _flat(model, table):
    sd = dict(model.named_parameters())
    return torch.cat([sd[n].detach().reshape(-1).float() for n, _, _, _ in table])


def _spec(arch, C, nl, nb=0, scale=4, cb=2):
    return NetSpec(arch=arch, nchannels_in=C, nchannels_out=C, nfeatures=64, nlayers=nl, nblocks=nb, cbottleneck=cb,
                   scale=scale, dtype="fp32")


FIRST_C1 = ("body.0.body.0.body.0.weight", "body.0.body.0.body.0.bias")


def _rcan_step_vs_oracle(cb, nl, nb):
    """One exact-fp32 RCAN train step (seed-9 weights, synthetic_hr(2, 2, 192, 13)) against
    the fp64 oracle on the same weights and tiles, and against the fp64 oracle run with the
    engine's own ReLU masks.  -> ({name: (error vs fp64, fp32 CPU drift, error vs the
    mask-aligned fp64)}, the ReLU decisions that differ from fp64's, those outside the fp32
    rounding bound); the loss is held to 1e-5 here."""
    import copy
    import fp32_stages as fs
    d = dev()
    C, B = 2, 2
    model = ro.RCANOracle(nchannels_in=C, nchannels_out=C, nlayers=nl, nblocks=nb, nfeatures=64, cbottleneck=cb)
    ro.init_params_numpy(model, 9)
    spec = _spec("rcan", C, nl, nb, 4, cb=cb)
    table = param_table(spec)
    tr = FusedTrainer(spec, B, (48, 48), device=d, params=_flat(model, table).to(d))
    hr = ro.synthetic_hr(B, C, 192, 13)
    h32 = torch.tensor(hr)
    h = torch.tensor(hr, dtype=torch.float64)
    g32 = fs.oracle_stages(copy.deepcopy(model).float(), ro.downsample(h32, 4), None,
                           loss_fn=lambda out: ro.l2loss(out, h32))["grads"]
    m64 = model.double()
    ref = fs.oracle_stages(m64, ro.downsample(h, 4), None, loss_fn=lambda out: ro.l2loss(out, h))
    res = tr.step(torch.tensor(hr, device=d))
    torch.cuda.synchronize()
    assert abs(float(res["loss"]) - ref["loss"]) / ref["loss"] < 1e-5
    t_maps = {(g, b): tr.eng.buffer("T", g, b).cpu() for g in range(nl) for b in range(1, nb + 1)}
    flips, outside = fs.mask_flips(ref, t_maps)
    al = fs.oracle_stages(m64, ro.downsample(h, 4), None, masks=fs.relu_masks(t_maps),
                          loss_fn=lambda out: ro.l2loss(out, h))["grads"]
    grads = tr.grads.cpu()
    errs = {name: (rel_l2(grads[off:off + n].view(shape), ref["grads"][name]), rel_l2(g32[name], ref["grads"][name]),
                   rel_l2(grads[off:off + n].view(shape), al[name])) for name, off, n, shape in table}
    top = sorted(errs.items(), key=lambda kv: -kv[1][0])[:4]
    print(f"\ncb {cb}, {nl} x {nb}: ReLU decisions that differ from fp64: {flips}")
    print("worst vs fp64 (engine, fp32 CPU drift, engine vs mask-aligned fp64): "
          f"{[(nm, f'{e:.2e}', f'{dr:.2e}', f'{ea:.2e}') for nm, (e, dr, ea) in top]}")
    return errs, flips, outside


@pytest.mark.parametrize("cb", [2, 8, 16])
def test_fp32_rcan_other_bottlenecks_vs_oracle(cb):
    """The exact-fp32 RCAN engine at CA bottlenecks 2, 8 and 16 (CR = 32, 8, 4) and three
    RCABs per group against the fp64 oracle on the same weights and tiles: loss to 1e-5,
    every gradient tensor to 1e-3 rel-L2 (the CA parameter gradients of RCABs 2..nb read the
    engine's per-RCAB record slots).

    The first RCAB's conv1 weight and bias gradients sit at 1.5e-3 .. 2.7e-3 with these
    weights and tiles and keep a 5e-3 bound against the PLAIN fp64 oracle: conv1's
    pre-activation z[image 1, c 52, y 21, x 23] is +3.9e-8 in fp64 (+3.0e-8 in fp32 torch
    on the CPU), inside the fp32 rounding error of zero, the engine's fp32 sum lands at or
    below zero, and that one ReLU decision removes one element of dz whose share of ||dz||
    is exactly the measured offset (tests/test_gpu_fp32_stages.py localises
    it).  Against the fp64 oracle run with the engine's own ReLU masks -- which may differ
    from fp64's only inside the a-priori fp32 rounding bound of the sum, and in at most
    1e-5 of a map -- EVERY tensor is held to 5e-5 (the level of every healthy fp32 gradient
    tensor of this model; ten times the tensor's fp32-CPU drift where that is more), with
    no exception."""
    errs, flips, outside = _rcan_step_vs_oracle(cb, 2, 3)
    assert not outside, (outside, flips)
    for name, (err, drift, err_al) in errs.items():
        assert err < (5e-3 if name in FIRST_C1 else 1e-3), (name, err, drift)
        assert err_al < max(5e-5, 10 * drift), (name, err_al, drift)


def test_fp32_rcan_deeper_groups_vs_oracle():
    """The same at 2 groups x 8 RCABs, B = 2, cb 16: the per-RCAB slots, slab sets and the
    group-end reduction at a depth the goldens' small models do not reach."""
    errs, flips, outside = _rcan_step_vs_oracle(16, 2, 8)
    assert not outside, (outside, flips)
    for name, (err, drift, err_al) in errs.items():
        assert err < (5e-3 if name in FIRST_C1 else 1e-3), (name, err, drift)
        assert err_al < max(5e-5, 10 * drift), (name, err_al, drift)


@pytest.mark.parametrize("arch,C,nl,nb,scale,S,B,gname", [
    ("rcan", 1, 2, 2, 4, 192, 2, "rcan_small_c1_f64.npz"),
    ("rcan", 2, 2, 2, 4, 192, 2, "rcan_small_c2_f64.npz"),
    ("edsr", 4, 2, 0, 8, 256, 1, "edsr_small_c4_f64.npz"),
])
def test_fp32_small_model_step_vs_golden(arch, C, nl, nb, scale, S, B, gname):
    d = dev()
    gd = np.load(os.path.join(GOLDEN, gname))
    kw = dict(nchannels_in=C, nchannels_out=C, nlayers=nl, nfeatures=64)
    model = (ro.RCANOracle(nblocks=nb, cbottleneck=2, **kw) if arch == "rcan"
             else ro.EDSROracle(downscale_factors=[2, 2, 2], **kw))
    ro.init_params_numpy(model, int(gd["seed_w"]))
    spec = _spec(arch, C, nl, nb, scale)
    table = param_table(spec)
    tr = FusedTrainer(spec, B, (S // scale, S // scale), lr=float(gd["lr"]), device=d,
                      params=_flat(model, table).to(d))
    model = model.double()
    hr = ro.synthetic_hr(B, C, S, int(gd["seed_x"]))
    model.zero_grad()
    h = torch.tensor(hr, dtype=torch.float64)
    loss_ref = ro.l2loss(model(ro.downsample(h, scale)), h)
    loss_ref.backward()
    res = tr.step(torch.tensor(hr, device=d))
    torch.cuda.synchronize()
    assert abs(float(res["loss"]) - float(gd["loss0"])) / float(gd["loss0"]) < 1e-5
    assert abs(float(res["interp_loss"]) - float(gd["iloss0"])) / float(gd["iloss0"]) < 1e-5
    assert rel_l2(tr.sr[:B].cpu()[:, :, ::4, ::4], gd["out_sub"]) < 1e-5
    grads = tr.grads.cpu()
    g = dict(model.named_parameters())
    worst = max(rel_l2(grads[off:off + n].view(shape), g[name].grad) for name, off, n, shape in table)
    print(f"\n{gname}: fp32 engine worst per-tensor grad rel-L2 {worst:.2e}")
    assert worst < 1e-3
    if arch == "rcan":
        # the same against fp64 with the engine's own ReLU masks (_rcan_step_vs_oracle): what is
        # left of `worst` once the ReLU decisions fp32 cannot make the way fp64 does are shared
        import fp32_stages as fs
        t_maps = {(gi, b): tr.eng.buffer("T", gi, b).cpu() for gi in range(nl) for b in range(1, nb + 1)}
        lr64 = ro.downsample(h, scale)
        flips, outside = fs.mask_flips(fs.oracle_stages(model, lr64, None, loss_fn=lambda out: ro.l2loss(out, h)), t_maps)
        al = fs.oracle_stages(model, lr64, None, masks=fs.relu_masks(t_maps), loss_fn=lambda out: ro.l2loss(out, h))["grads"]
        worst_al = max(rel_l2(grads[off:off + n].view(shape), al[name]) for name, off, n, shape in table)
        print(f"{gname}: ReLU decisions that differ from fp64 {flips}; worst vs the mask-aligned fp64 {worst_al:.2e}")
        assert not outside, (outside, flips)
        assert worst_al < 5e-5
    np.testing.assert_allclose(np.array([float(grads[o:o + n].norm()) for _, o, n, _ in table]), gd["grad_l2"],
                               rtol=1e-3)
    res = tr.step(torch.tensor(hr, device=d))
    torch.cuda.synchronize()
    assert abs(float(res["loss"]) - float(gd["loss1"])) / float(gd["loss1"]) < 1e-5


def test_fp32_full_rcan_vs_golden():
    """rcan-10-20-64, 2-var, one tile, exact fp32: output and loss vs the fp64 golden
    of the reference, and the golden's gradient samples."""
    d = dev()
    gd = np.load(os.path.join(GOLDEN, "rcan_full_c2_f64.npz"))
    m = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=10, nblocks=20, nfeatures=64, cbottleneck=2)
    ro.init_params_numpy(m, int(gd["seed_w"]))
    spec = _spec("rcan", 2, 10, 20)
    table = param_table(spec)
    flat = _flat(m, table).to(d)
    hr = torch.tensor(ro.synthetic_hr(1, 2, 192, int(gd["seed_x"])), device=d)
    eng = Engine(spec, 1, (48, 48), train=False, device=d)
    eng.pack(flat)
    out = eng.forward(flat, downsample(hr, 4))
    torch.cuda.synchronize()
    r_out = rel_l2(out.cpu()[:, :, ::4, ::4], gd["out_sub"])
    loss = float(((out.double() - hr.double()) ** 2).mean().sqrt())
    print(f"\nfull rcan fp32: output rel-L2 {r_out:.2e}, loss rel {abs(loss - float(gd['loss0'])) / float(gd['loss0']):.2e}")
    assert r_out < 1e-5
    assert abs(loss - float(gd["loss0"])) / float(gd["loss0"]) < 1e-5
    tr = FusedTrainer(spec, 1, (48, 48), lr=float(gd["lr"]), device=d, params=flat)
    tr.step(hr)
    torch.cuda.synchronize()
    g = tr.grads.double().cpu().numpy()
    eng_s, per, k = [], [], 0
    ref = gd["grad_sample"]
    for name, off, n, shape in table:
        idx = np.unique(np.linspace(0, n - 1, min(n, 48)).astype(np.int64))
        a = g[off + idx]
        b = ref[k:k + idx.size]
        per.append(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
        eng_s.append(a)
        k += idx.size
    r_all = np.linalg.norm(np.concatenate(eng_s) - ref) / np.linalg.norm(ref)
    print(f"full rcan fp32: grad samples rel-L2 {r_all:.2e}, per-tensor max {max(per):.2e}")
    assert r_all < 1e-3
    assert np.median(per) < 1e-3 and max(per) < 1e-2
    # max(per) (2.4e-3 measured) is a handful of ReLU decisions, too: among the 200 RCABs' 29 M
    # pre-activations 8 lie within 1.5e-6 of zero and fall on the other side in the engine's
    # fp32 sums (a conv1 gradient each, 1.7e-3 the worst); with those shared, every one of the
    # 1630 tensors -- whole, not sampled -- is within 5e-5 of fp64 (1.0e-6 measured)
    import fp32_stages as fs
    t_maps = {(gi, b): tr.eng.buffer("T", gi, b).cpu() for gi in range(10) for b in range(1, 21)}
    m = m.double()
    h = hr.double().cpu()
    lr64 = ro.downsample(h, 4)
    flips, outside = fs.mask_flips(fs.oracle_stages(m, lr64, None, loss_fn=lambda out: ro.l2loss(out, h)), t_maps)
    al = fs.oracle_stages(m, lr64, None, masks=fs.relu_masks(t_maps), loss_fn=lambda out: ro.l2loss(out, h))["grads"]
    gt = tr.grads.cpu()
    worst_al = max(rel_l2(gt[off:off + n].view(shape), al[name]) for name, off, n, shape in table)
    print(f"full rcan fp32: {len(flips)} ReLU decisions differ from fp64 {flips}; worst tensor vs the mask-aligned "
          f"fp64 {worst_al:.2e}")
    assert not outside, (outside, flips)
    assert worst_al < 5e-5


@pytest.mark.timeout(600)
@pytest.mark.parametrize("B", [4, 64])
def test_c4_edsr_x8_fp32_full_config_vs_oracle(B):
    """BASELINE config 4 itself: EDSR, 16 ResBlocks, 64 features, x8 (32 -> 256),
    4 channels, fp32 -- one train step against the oracle in fp32 on the GPU.
    B=64 is bench.py's edsr_x8 line exactly: FusedTrainer's default split into
    micro=2 engines of 32 tiles, each sizing its launches for cu_budget=128."""
    d = dev()
    spec = _spec("edsr", 4, 16, 0, 8)
    table = param_table(spec)
    hr = torch.tensor(ro.synthetic_hr(B, 4, 256, 77), device=d)
    with exact_fp32():
        m = ro.EDSROracle(nchannels_in=4, nchannels_out=4, nlayers=16, nfeatures=64, downscale_factors=[2, 2, 2])
        ro.init_params_numpy(m, 3)
        m = m.to(d)
        flat = _flat(m, table)
        lr_in = ro.downsample(hr, 8)
        out_ref = m(lr_in)
        loss_ref = ro.l2loss(out_ref, hr)
        loss_ref.backward()
        g = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
        out_ref = out_ref.detach()
        del m, lr_in  # the oracle's autograd graph (B=64: ~15 GB) is freed before the engines are built
    tr = FusedTrainer(spec, B, (32, 32), lr=1e-4, device=d, params=flat)
    if B == 64:
        assert tr.micro == 2 and all(e._cfg.cu_budget == 128 for e in tr.engines)
    res = tr.step(hr)
    torch.cuda.synchronize()
    assert abs(float(res["loss"]) - float(loss_ref)) / float(loss_ref) < 1e-5
    assert rel_l2(tr.sr, out_ref) < 1e-5
    worst = max(rel_l2(tr.grads[off:off + n].view(shape), g[name]) for name, off, n, shape in table)
    print(f"\nC4 EDSR x8 fp32 B={B} micro={tr.micro}: loss {float(res['loss']):.7f} vs {float(loss_ref):.7f}, "
          f"worst grad rel-L2 {worst:.2e}")
    assert worst < 1e-3


def test_fp32_micro_batch_step_matches_single_engine():
    """The fp32 engine mode under FusedTrainer(micro=2) equals one engine: loss
    partials and gradients summed exactly (up to fp32 summation order)."""
    d = dev()
    spec = _spec("edsr", 4, 2, 0, 8)
    table = param_table(spec)
    from srmi.trainer import default_init_
    flat = torch.empty(sum(t[2] for t in table), device=d)
    default_init_(flat, table, seed=6)
    hr = torch.tensor(ro.synthetic_hr(16, 4, 256, 19)).to(d)
    res = []
    for micro in (1, 2):
        tr = FusedTrainer(spec, 16, (32, 32), device=d, params=flat, micro=micro)
        out = tr.step(hr)
        torch.cuda.synchronize()
        res.append((float(out["loss"]), float(out["interp_loss"]), tr.grads.clone(), tr.sr.clone()))
        del tr
    (l1, i1, g1, s1), (l2, i2, g2, s2) = res
    assert torch.equal(s1, s2)  # the forward is per tile: identical
    assert abs(l1 - l2) <= 1e-6 * abs(l1)
    assert abs(i1 - i2) <= 1e-6 * abs(i1)
    assert rel_l2(g2, g1) < 1e-6
