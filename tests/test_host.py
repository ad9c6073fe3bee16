"""Host-side tests (no GPU): the C-ABI library loads and exports every declared
symbol, the native parameter plan equals the reference state_dict, config
plumbing, the plugin module's construction contract, and the data-parallel
loss/gradient semantics over world_size-2 gloo."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from oracle import rcan_oracle as ro


def test_library_exports_every_header_symbol():
    from srmi import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "srmi.h")).read()
    names = sorted(set(re.findall(r"\b(srmi_[a-z0-9_]+)\s*\(", hdr)))
    assert names, "no prototypes parsed"
    for n in names:
        assert hasattr(lib, n), n
        assert n in _lib.EXPORTED, f"{n} declared in srmi.h but not bound in _lib"
    assert lib.srmi_version() >= 100


def test_engine_buffer_addresses_lie_in_the_workspace_and_do_not_overlap():
    """srmi_engine_buffer on an engine carved over a host buffer (nothing is launched):
    every map it reports lies inside the workspace, no two overlap, GROUP_IN_GRAD
    alternates between two buffers from the last group down, and what the engine does
    not have is SRMI_ERR_ARG."""
    import ctypes as C
    from srmi import _lib
    from srmi.engine import NetSpec
    lib = _lib.load()
    nl, nb, N, h, w = 3, 2, 2, 8, 32

    def make(spec, train):
        cfg = spec.cstruct(N, h, w)
        nbytes = C.c_size_t()
        assert lib.srmi_workspace_size(C.byref(cfg), train, C.byref(nbytes)) == 0
        ws = (C.c_char * (nbytes.value + 256))()
        eng = C.c_void_p()
        assert lib.srmi_engine_create(C.byref(cfg), ws, len(ws), train, C.byref(eng)) == 0
        return eng, ws

    def buf(eng, name, g=0, b=0):
        p, n, eb = C.c_void_p(), C.c_size_t(), C.c_int()
        rc = lib.srmi_engine_buffer(eng, _lib.BUFFERS[name], g, b, C.byref(p), C.byref(n), C.byref(eb))
        return rc, p.value, n.value * eb.value, eb.value

    for dtype, esz in (("fp32", 4), ("bf16", 2)):
        spec = NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nlayers=nl, nblocks=nb, scale=4, dtype=dtype)
        eng, ws = make(spec, 1)
        base = C.addressof(ws)
        want = [("X0F", 0, 0), ("DU", 0, 0), ("DZ", 0, 0), ("DRESF", 0, 0), ("HB", nl, 0),
                ("GROUP_IN_GRAD", nl - 1, 0), ("GROUP_IN_GRAD", nl - 2, 0)]
        want += [("HB", g, b) for g in range(nl) for b in range(nb + 1)]
        want += [(k, g, b) for k in ("T", "U", "REC", "BREC") for g in range(nl) for b in range(1, nb + 1)]
        spans = []
        for name, g, b in want:
            rc, p, nbytes, eb = buf(eng, name, g, b)
            assert rc == 0, (name, g, b)
            assert eb == (4 if name in ("X0F", "DRESF", "GROUP_IN_GRAD", "REC", "BREC") else esz), name
            assert nbytes == (N * {"REC": 160, "BREC": 224}[name] * 4 if name in ("REC", "BREC") else N * h * w * 64 * eb)
            assert base <= p and p + nbytes <= base + len(ws), (name, g, b)
            spans.append((p, p + nbytes, (name, g, b)))
        spans.sort()
        for (a0, a1, ka), (b0, b1, kb) in zip(spans, spans[1:]):
            assert a1 <= b0, (ka, kb)
        assert buf(eng, "GROUP_IN_GRAD", 0)[1] == buf(eng, "GROUP_IN_GRAD", 2)[1] != buf(eng, "GROUP_IN_GRAD", 1)[1]
        for name, g, b in (("HB", nl + 1, 0), ("HB", nl, 1), ("HB", 0, nb + 1), ("T", 0, 0), ("U", 0, nb + 1),
                           ("REC", nl, 1), ("BREC", -1, 1), ("GROUP_IN_GRAD", nl, 0)):
            assert buf(eng, name, g, b)[0] == -10001, (name, g, b)
        p, n, eb = C.c_void_p(), C.c_size_t(), C.c_int()
        assert lib.srmi_engine_buffer(eng, 99, 0, 0, C.byref(p), C.byref(n), C.byref(eb)) == -10001
        assert lib.srmi_engine_buffer(None, 0, 0, 0, C.byref(p), C.byref(n), C.byref(eb)) == -10001
        lib.srmi_engine_destroy(eng)
        inf, ws = make(spec, 0)  # an inference engine keeps no per-block maps and has no backward
        assert buf(inf, "X0F")[0] == 0
        for name in ("HB", "T", "U", "REC", "BREC", "DU", "DZ", "DRESF", "GROUP_IN_GRAD"):
            assert buf(inf, name, 0, 1 if name in ("T", "U", "REC", "BREC") else 0)[0] == -10001, name
        lib.srmi_engine_destroy(inf)
    edsr, ws = make(NetSpec(arch="edsr", nchannels_in=2, nchannels_out=2, nlayers=nl, scale=4, dtype="fp32"), 1)
    assert buf(edsr, "HB", nl, 0)[0] == 0 and buf(edsr, "T", nl - 1, 1)[0] == 0 and buf(edsr, "DZ")[0] == 0
    for name, g, b in (("U", 0, 1), ("REC", 0, 1), ("BREC", 0, 1), ("DU", 0, 0), ("GROUP_IN_GRAD", 0, 0), ("HB", 0, 1),
                       ("T", nl, 1)):
        assert buf(edsr, name, g, b)[0] == -10001, (name, g, b)
    lib.srmi_engine_destroy(edsr)


def test_trace_slots_tile_the_trace_buffer_without_overlap():
    """srmi_engine_trace_size / _trace / _trace_slot on engines carved over host buffers
    (nothing is launched): every slot lies inside the reported size, no two overlap, a short
    or misaligned buffer and engines with no RCAN backward are refused, NULL turns it off."""
    import ctypes as C
    from srmi import _lib
    from srmi.engine import NetSpec
    lib = _lib.load()
    nl, nb, N, h, w = 2, 3, 3, 8, 48

    def make(spec, train):
        cfg = spec.cstruct(N, h, w)
        nbytes = C.c_size_t()
        assert lib.srmi_workspace_size(C.byref(cfg), train, C.byref(nbytes)) == 0
        ws = (C.c_char * (nbytes.value + 256))()
        eng = C.c_void_p()
        assert lib.srmi_engine_create(C.byref(cfg), ws, len(ws), train, C.byref(eng)) == 0
        return eng, ws

    def slot(eng, name, g, b):
        off, n, eb = C.c_size_t(), C.c_size_t(), C.c_int()
        rc = lib.srmi_engine_trace_slot(eng, _lib.TRACE_SLOTS[name], g, b, C.byref(off), C.byref(n), C.byref(eb))
        return rc, off.value, n.value * eb.value, eb.value

    nstrips = lib.srmi_conv3x3_nstrips(h, w)
    for dtype, esz in (("fp32", 4), ("bf16", 2)):
        spec = NetSpec(arch="rcan", nchannels_in=1, nchannels_out=1, nlayers=nl, nblocks=nb, scale=4, dtype=dtype)
        eng, ws = make(spec, 1)
        total = C.c_size_t()
        assert lib.srmi_engine_trace_size(eng, C.byref(total)) == 0
        want = [("GRB", g, 0) for g in range(nl)] + [("STREAM", g, b) for g in range(nl) for b in range(nb + 1)]
        want += [(k, g, b) for k in ("PACC", "DZ", "DU") for g in range(nl) for b in range(1, nb + 1)]
        spans = []
        for name, g, b in want:
            rc, off, nbytes, eb = slot(eng, name, g, b)
            assert rc == 0, (name, g, b)
            assert eb == (4 if name == "PACC" else esz)
            assert nbytes == (N * nstrips * 128 * 4 if name == "PACC" else N * h * w * 64 * esz)
            assert off % 256 == 0 and off + nbytes <= total.value, (name, g, b)
            spans.append((off, off + nbytes, (name, g, b)))
        spans.sort()
        for (a0, a1, ka), (b0, b1, kb) in zip(spans, spans[1:]):
            assert a1 <= b0, (ka, kb)
        for name, g, b in (("GRB", 0, 1), ("GRB", nl, 0), ("STREAM", 0, nb + 1), ("STREAM", -1, 0), ("PACC", 0, 0),
                           ("DZ", 0, nb + 1), ("DU", 0, 0)):
            assert slot(eng, name, g, b)[0] == -10001, (name, g, b)
        off, n, eb = C.c_size_t(), C.c_size_t(), C.c_int()
        assert lib.srmi_engine_trace_slot(eng, 9, 0, 0, C.byref(off), C.byref(n), C.byref(eb)) == -10001
        raw = (C.c_char * (total.value + 512))()
        base = (C.addressof(raw) + 255) & ~255
        assert lib.srmi_engine_trace(eng, C.c_void_p(base), total.value) == 0
        assert lib.srmi_engine_trace(eng, C.c_void_p(base), total.value - 1) == -10003
        assert lib.srmi_engine_trace(eng, C.c_void_p(base + 2), total.value) == -10003
        assert lib.srmi_engine_trace(eng, None, 0) == 0
        assert lib.srmi_engine_trace(None, None, 0) == -10001
        lib.srmi_engine_destroy(eng)
        inf, ws = make(spec, 0)
        assert lib.srmi_engine_trace_size(inf, C.byref(total)) == -10001
        assert lib.srmi_engine_trace(inf, None, 0) == -10001
        lib.srmi_engine_destroy(inf)
    edsr, ws = make(NetSpec(arch="edsr", nchannels_in=1, nchannels_out=1, nlayers=nl, scale=4, dtype="fp32"), 1)
    assert lib.srmi_engine_trace_size(edsr, C.byref(total)) == -10001
    lib.srmi_engine_destroy(edsr)


def test_forward_trace_slots_and_new_buffers():
    """srmi_engine_fwd_trace_size / _fwd_trace / _fwd_trace_slot and SRMI_BUF_RESB / _PS on
    engines carved over host buffers (nothing is launched): every slot is 256-byte aligned, of
    its documented size, inside the reported size and disjoint from the others; an inference
    engine has the HB / T / REC slots a train engine refuses; a short or misaligned buffer, the
    exact-fp32 engine and EDSR are refused, NULL turns it off; RESB and PS(k) lie in the
    workspace beside the other maps, in inference engines too."""
    import ctypes as C
    from srmi import _lib
    from srmi.engine import NetSpec
    lib = _lib.load()
    nl, nb, N, h, w = 2, 3, 3, 8, 48

    def make(spec, train):
        cfg = spec.cstruct(N, h, w)
        nbytes = C.c_size_t()
        assert lib.srmi_workspace_size(C.byref(cfg), train, C.byref(nbytes)) == 0
        ws = (C.c_char * (nbytes.value + 256))()
        eng = C.c_void_p()
        assert lib.srmi_engine_create(C.byref(cfg), ws, len(ws), train, C.byref(eng)) == 0
        return eng, ws

    def slot(eng, name, g, b):
        off, n, eb = C.c_size_t(), C.c_size_t(), C.c_int()
        rc = lib.srmi_engine_fwd_trace_slot(eng, _lib.FWD_TRACE_SLOTS[name], g, b, C.byref(off), C.byref(n),
                                            C.byref(eb))
        return rc, off.value, n.value * eb.value, eb.value

    def buf(eng, name, g=0, b=0):
        p, n, eb = C.c_void_p(), C.c_size_t(), C.c_int()
        rc = lib.srmi_engine_buffer(eng, _lib.BUFFERS[name], g, b, C.byref(p), C.byref(n), C.byref(eb))
        return rc, p.value, n.value * eb.value, eb.value

    for name in ("srmi_engine_fwd_trace_size", "srmi_engine_fwd_trace", "srmi_engine_fwd_trace_slot"):
        assert hasattr(lib, name) and name in _lib.EXPORTED
    assert _lib.BUFFERS["GROUP_IN_GRAD"] == 9 and _lib.BUFFERS["RESB"] == 10 and _lib.BUFFERS["PS"] == 11
    assert _lib.TRACE_SLOTS == {"GRB": 0, "STREAM": 1, "PACC": 2, "DZ": 3, "DU": 4}
    nstrips = lib.srmi_conv3x3_nstrips(h, w)
    px = N * h * w * 64
    size = {"LO": (px, 1), "PPOOL": (N * nstrips * 64 * 4, 4), "RF": (px * 4, 4), "HB": (px * 2, 2), "T": (px * 2, 2),
            "REC": (N * 160 * 4, 4)}
    spec = NetSpec(arch="rcan", nchannels_in=1, nchannels_out=1, nlayers=nl, nblocks=nb, scale=4, dtype="bf16")
    common = [(k, g, b) for k in ("LO", "PPOOL") for g in range(nl) for b in range(1, nb + 1)]
    common += [("RF", g, 0) for g in range(nl)]
    infer_only = [("HB", g, b) for g in range(nl) for b in range(nb + 1)] + [("HB", nl, 0)]
    infer_only += [(k, g, b) for k in ("T", "REC") for g in range(nl) for b in range(1, nb + 1)]
    totals = {}
    for train in (1, 0):
        eng, ws = make(spec, train)
        total = C.c_size_t()
        assert lib.srmi_engine_fwd_trace_size(eng, C.byref(total)) == 0
        totals[train] = total.value
        spans = []
        for name, g, b in common + ([] if train else infer_only):
            rc, off, nbytes, eb = slot(eng, name, g, b)
            assert rc == 0, (name, g, b)
            assert (nbytes, eb) == size[name], (name, g, b)
            assert off % 256 == 0 and off + nbytes <= total.value, (name, g, b)
            spans.append((off, off + nbytes, (name, g, b)))
        spans.sort()
        for (a0, a1, ka), (b0, b1, kb) in zip(spans, spans[1:]):
            assert a1 <= b0, (ka, kb)
        bad = [("LO", 0, 0), ("LO", 0, nb + 1), ("LO", nl, 1), ("LO", -1, 1), ("PPOOL", 0, 0), ("RF", 0, 1),
               ("RF", nl, 0), ("HB", nl, 1), ("HB", nl + 1, 0), ("HB", 0, nb + 1), ("T", 0, 0), ("REC", 0, nb + 1)]
        for name, g, b in bad + (infer_only if train else []):
            assert slot(eng, name, g, b)[0] == -10001, (train, name, g, b)
        off, n, eb = C.c_size_t(), C.c_size_t(), C.c_int()
        assert lib.srmi_engine_fwd_trace_slot(eng, 9, 0, 1, C.byref(off), C.byref(n), C.byref(eb)) == -10001
        assert lib.srmi_engine_fwd_trace_slot(eng, 0, 0, 1, None, C.byref(n), C.byref(eb)) == -10001
        raw = (C.c_char * (total.value + 512))()
        base = (C.addressof(raw) + 255) & ~255
        assert lib.srmi_engine_fwd_trace(eng, C.c_void_p(base), total.value) == 0
        assert lib.srmi_engine_fwd_trace(eng, C.c_void_p(base), total.value - 1) == -10003
        assert lib.srmi_engine_fwd_trace(eng, C.c_void_p(base + 2), total.value) == -10003
        assert lib.srmi_engine_fwd_trace(eng, None, 0) == 0
        assert lib.srmi_engine_fwd_trace_size(eng, None) == -10001
        # RESB and PS(k): in the workspace, disjoint from each other and from the other maps
        wbase = C.addressof(ws)
        maps = [("X0F", 0, 0, px * 4), ("RESB", 0, 0, px * 2), ("PS", 0, 0, px * 4 * 2), ("PS", 1, 0, px * 16 * 2)]
        if train:
            maps += [("HB", nl, 0, px * 2), ("T", nl - 1, nb, px * 2), ("U", nl - 1, nb, px * 2)]
        spans = []
        for name, g, b, want in maps:
            rc, p, nbytes, eb = buf(eng, name, g, b)
            assert rc == 0 and nbytes == want, (name, g)
            assert wbase <= p and p + nbytes <= wbase + len(ws), (name, g)
            spans.append((p, p + nbytes, (name, g)))
        spans.sort()
        for (a0, a1, ka), (b0, b1, kb) in zip(spans, spans[1:]):
            assert a1 <= b0, (ka, kb)
        assert buf(eng, "PS", 2)[0] == -10001 and buf(eng, "PS", -1)[0] == -10001
        assert lib.srmi_engine_probe(eng, 8, 1, None) == (1 if train else 2)
        lib.srmi_engine_destroy(eng)
    assert totals[0] > totals[1]
    assert lib.srmi_engine_fwd_trace_size(None, C.byref(total)) == -10001
    assert lib.srmi_engine_fwd_trace(None, None, 0) == -10001
    for other in (NetSpec(arch="rcan", nchannels_in=1, nchannels_out=1, nlayers=nl, nblocks=nb, scale=4, dtype="fp32"),
                  NetSpec(arch="edsr", nchannels_in=1, nchannels_out=1, nlayers=nl, scale=4, dtype="bf16")):
        eng, ws = make(other, 1)
        assert lib.srmi_engine_fwd_trace_size(eng, C.byref(total)) == -10001
        assert lib.srmi_engine_fwd_trace(eng, None, 0) == -10001
        assert slot(eng, "LO", 0, 1)[0] == -10001
        assert buf(eng, "RESB")[0] == 0 and buf(eng, "PS", 1)[0] == 0
        lib.srmi_engine_destroy(eng)


@pytest.mark.parametrize("C", [1, 2])
def test_native_param_plan_matches_reference_state_dict(C):
    from srmi.engine import NetSpec, param_table
    meta = json.load(open(os.path.join(GOLDEN, "keys.json")))
    spec = NetSpec(arch="rcan", nchannels_in=C, nchannels_out=C, nlayers=10, nblocks=20)
    tab = param_table(spec)
    m = ro.RCANOracle(nchannels_in=C, nchannels_out=C, nlayers=10, nblocks=20)
    exp = [(k, tuple(v.shape)) for k, v in m.named_parameters()]
    assert [(t[0], t[3]) for t in tab] == exp
    if C == 2:
        assert [[t[0], list(t[3])] for t in tab] == meta["keys"]["rcan-10-20-64_c2"]
    offs = [t[1] for t in tab]
    assert offs == sorted(offs) and offs[0] == 0
    assert sum(t[2] for t in tab) == (16313602 if C == 2 else 16312449)


def test_native_param_plan_edsr_x8():
    from srmi.engine import NetSpec, param_table
    meta = json.load(open(os.path.join(GOLDEN, "keys.json")))
    spec = NetSpec(arch="edsr", nchannels_in=4, nchannels_out=4, nlayers=2, scale=8)
    tab = param_table(spec)
    assert [[t[0], list(t[3])] for t in tab] == meta["keys"]["edsr_small_c4"]


def test_workspace_sizes_are_sane():
    import ctypes as C
    from srmi import _lib
    from srmi.engine import NetSpec
    spec = NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nlayers=10, nblocks=20)
    cfg = spec.cstruct(64, 48, 48)
    tb, ib = C.c_size_t(), C.c_size_t()
    _lib.call("srmi_workspace_size", C.byref(cfg), 1, C.byref(tb))
    _lib.call("srmi_workspace_size", C.byref(cfg), 0, C.byref(ib))
    map_b = 64 * 48 * 48 * 64 * 2
    # train saves hb/t/u for every RCAB (~611 bf16 maps); inference keeps a ring
    assert 600 * map_b < tb.value < 20e9
    assert ib.value < 2e9
    bad = spec.cstruct(64, 47, 48)
    with pytest.raises(_lib.SrmiError):
        _lib.call("srmi_workspace_size", C.byref(bad), 1, C.byref(tb))
    # CA bottlenecks: CR = 64 / cbottleneck must be 4 .. 32 and a multiple of 4
    for cb in (4, 8, 16):
        ok = NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, cbottleneck=cb)
        _lib.call("srmi_workspace_size", C.byref(ok.cstruct(8, 48, 48)), 1, C.byref(tb))
    for cb in (1, 32, 64):
        bad = NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=2, cbottleneck=cb)
        with pytest.raises(_lib.SrmiError):
            _lib.call("srmi_workspace_size", C.byref(bad.cstruct(8, 48, 48)), 1, C.byref(tb))


def test_engine_refuses_maps_past_the_32bit_buffer_range():
    """Maps are stored through buffer resources with 32-bit byte ranges: EDSR x8
    fp32 at 256 tiles makes the last pixel-shuffle map exactly 2^32 bytes and must be
    refused (SRMI_ERR_SHAPE), not run with silently dropped stores; 255 tiles fit."""
    import ctypes as C
    from srmi import _lib
    from srmi.engine import NetSpec
    spec = NetSpec(arch="edsr", nchannels_in=4, nchannels_out=4, nlayers=16, scale=8, dtype="fp32")
    b = C.c_size_t()
    ok = spec.cstruct(255, 32, 32)
    _lib.call("srmi_workspace_size", C.byref(ok), 1, C.byref(b))
    assert (255 * 32 * 32 * 64 << 6) * 4 < 2 ** 32
    big = spec.cstruct(256, 32, 32)
    with pytest.raises(_lib.SrmiError):
        _lib.call("srmi_workspace_size", C.byref(big), 1, C.byref(b))
    bf = NetSpec(arch="edsr", nchannels_in=4, nchannels_out=4, nlayers=16, scale=8)
    _lib.call("srmi_workspace_size", C.byref(bf.cstruct(256, 32, 32)), 1, C.byref(b))  # bf16: 2^31


def test_config_context_and_init_parms():
    from srmi.config import ConfigContext, cfg, init_parms
    with ConfigContext("sres", dict(model="rcan-10-20-64", task="SSS_SST-tiles-48"), **{"task.lr": 1e-4}):
        c = cfg()
        assert c.model.nblocks == 20 and c.model.cbottleneck == 2 and c.task.lr == 1e-4
        assert list(c.task.target_variables) == ["SSS", "SST"]
        p = init_parms("rcan", dict(nchannels_in=2, nchannels_out=2, device="cpu"))
        assert p["scale"] == 4 and p["nlayers"] == 10 and p["nblocks"] == 20 and p["device"] == "cpu"
    p = init_parms("rcan", dict(nchannels_in=1), model_cfg={"nlayers": 3})
    assert p["nlayers"] == 3 and p["nblocks"] == 20 and p["nfeatures"] == 64


def test_plugin_contract_on_cpu():
    from srmi import _lib
    from srmi.config import ConfigContext
    from srmi.model.rcan.network import get_model
    with ConfigContext("sres", dict(model="rcan-10-20-64"), **{"model.nlayers": 2, "model.nblocks": 3}):
        net = get_model(nchannels_in=2, nchannels_out=2, device="cpu")
    o = ro.RCANOracle(nchannels_in=2, nchannels_out=2, nlayers=2, nblocks=3)
    assert [(k, v.shape) for k, v in net.state_dict().items()] == [(k, v.shape) for k, v in o.state_dict().items()]
    # every parameter is a view of one flat buffer
    flat = net._flat
    for (name, off, n, shape), p in zip(net._table, net.parameters()):
        assert p.data_ptr() == flat.data_ptr() + 4 * off
    # tolerant load_state_dict (common.py:50-71): wrong-shaped tail is skipped, others raise
    sd = o.state_dict()
    net.load_state_dict(sd)
    assert torch.equal(net.state_dict()["head.0.weight"], sd["head.0.weight"])
    bad = dict(sd)
    bad["tail.1.weight"] = torch.zeros(3, 64, 3, 3)
    net.load_state_dict(bad)
    bad["head.0.weight"] = torch.zeros(5, 7)
    with pytest.raises(RuntimeError):
        net.load_state_dict(bad)
    # product path refuses CPU tensors: no silent fallback
    with pytest.raises(_lib.SrmiError):
        net(torch.zeros(1, 2, 48, 48))
    assert net.nblocks == 3 and net.scale == 4  # FModule attribute access


def test_grad_buckets_partition_every_parameter_once():
    from srmi.dist import DistInfo, GradReducer, grad_buckets
    from srmi.engine import NetSpec, param_table
    for spec in (NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nlayers=10, nblocks=20),
                 NetSpec(arch="edsr", nchannels_in=4, nchannels_out=4, nlayers=16, scale=8)):
        tab = param_table(spec)
        n = sum(t[2] for t in tab)
        mask = np.zeros(n, dtype=np.int32)
        for b in grad_buckets(tab, spec.arch, spec.nlayers):
            for off, k in b.ranges:
                mask[off:off + k] += 1
        assert np.all(mask == 1)
        r = GradReducer(tab, spec.arch, spec.nlayers, DistInfo(), torch.device("cpu"))
        assert r.covered() == n
    # rcan: one bucket per residual group in backward order, head last; the bucket of
    # body.{g} waits on group event g, which srmi_backward records after group g
    tab = param_table(NetSpec(arch="rcan", nlayers=3, nblocks=2))
    b = grad_buckets(tab, "rcan", 3)
    assert [x.event_index for x in b] == [2, 1, 0, None]
    names = {off: nm for nm, off, _, _ in tab}
    for bk in b[:-1]:
        groups = {int(names[off].split(".")[1]) for off, _ in bk.ranges
                  if names[off].startswith("body.") and names[off].split(".")[2] == "body"}
        assert groups == {bk.event_index}
    # the staged schedule (srmi_backward_stages: 0 tail/upsamplers/body tail, 1..nl
    # groups nl-1..0, nl+1 head): group g's bucket after stage nl - g, the head's last
    r = GradReducer(tab, "rcan", 3, DistInfo(), torch.device("cpu"), stream=False)
    sb = r.stage_buckets(3 + 2)
    assert [[x.event_index for x in st] for st in sb] == [[], [2], [1], [0], [None]]
    tab_e = param_table(NetSpec(arch="edsr", nchannels_in=4, nchannels_out=4, nlayers=16, scale=8))
    sb = GradReducer(tab_e, "edsr", 16, DistInfo(), torch.device("cpu"), stream=False).stage_buckets(1)
    assert len(sb) == 1 and len(sb[0]) == 2


def _dp_rank(rank, world, port, q, micro=1, staged=False):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import sys
    sys.path.insert(0, os.path.join(ROOT, "super-resolution-climate_amd"))
    sys.path.insert(0, ROOT)
    from srmi.dist import GradReducer, global_rmse_scale, init_from_env, shard_range
    from srmi.engine import NetSpec
    from srmi.model.common import _python_table
    from oracle import rcan_oracle as ro
    torch.set_num_threads(2)
    info = init_from_env("gloo")
    spec = NetSpec(arch="rcan", nchannels_in=1, nchannels_out=1, nlayers=1, nblocks=1)
    table = _python_table(spec)
    model = ro.RCANOracle(nchannels_in=1, nchannels_out=1, nlayers=1, nblocks=1).double()
    ro.init_params_numpy(model, 0)
    hr_all = torch.tensor(ro.synthetic_hr(4, 1, 192, 3), dtype=torch.float64)
    a, b = shard_range(4, info)
    hr = hr_all[a:b]
    out = model(ro.downsample(hr, 4))
    S = ((out - hr) ** 2).sum().detach().reshape(1)
    count = float(hr_all.numel())
    L, scale = global_rmse_scale(S, count, info)
    dy = (out - hr).detach() * scale          # dL/dy with the GLOBAL count and L
    sd = dict(model.named_parameters())
    mg = []
    per = hr.shape[0] // micro
    for k in range(micro):  # micro-batch engines: separate gradients, summed by the reducer
        model.zero_grad()
        o = model(ro.downsample(hr[k * per:(k + 1) * per], 4))
        o.backward(dy[k * per:(k + 1) * per])
        mg.append(torch.cat([sd[n].grad.reshape(-1) for n, _, _, _ in table]))
    red = GradReducer(table, "rcan", 1, info, torch.device("cpu"), stream=not staged)
    if staged:  # the trainer's default schedule: each bucket behind its backward stage
        works = []
        for bk in red.stage_buckets(1 + 2):
            red.reduce_stage(bk, mg[0], mg[1:], works)
        for w in works:
            w.wait()
    else:
        red.reduce(mg[0], extra=mg[1:])
    grads = mg[0]
    q.put((rank, float(L), grads.numpy()))
    dist.destroy_process_group()


@pytest.mark.parametrize("micro,staged", [(1, False), (2, False), (1, True), (2, True)])
def test_data_parallel_semantics_gloo_world2(micro, staged):
    """2 ranks x 2 tiles == 1 process x 4 tiles: global RMSE and summed grads
    (micro=2: each rank's 2 tiles as 2 micro-batch gradients, summed per bucket
    by the reducer before its all-reduce; staged: bucket by bucket in backward-stage
    order, as FusedTrainer's default DP schedule issues them)."""
    import multiprocessing as mp
    import random
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + random.randint(0, 2000)
    ps = [ctx.Process(target=_dp_rank, args=(r, 2, port, q, micro, staged)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=300) for _ in ps], key=lambda t: t[0])
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    model = ro.RCANOracle(nchannels_in=1, nchannels_out=1, nlayers=1, nblocks=1).double()
    ro.init_params_numpy(model, 0)
    hr = torch.tensor(ro.synthetic_hr(4, 1, 192, 3), dtype=torch.float64)
    loss = ro.l2loss(model(ro.downsample(hr, 4)), hr)
    loss.backward()
    ref = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).numpy()
    for rank, L, g in res:
        assert abs(L - float(loss)) < 1e-12
        np.testing.assert_allclose(g, ref, rtol=1e-9, atol=1e-12)


def test_conv_abi_rejects_missing_operands():
    """Op-level convs refuse (SRMI_ERR_ARG) instead of dereferencing a NULL operand.
    The checks run before any launch, so this needs no GPU."""
    import ctypes as C
    from srmi import _lib
    lib = _lib.load()
    dummy = C.c_void_p(16)  # never dereferenced: every case below fails validation first
    # epi 4 (dgrad * relu mask) without the mask, epi 2 (residual) without r1,
    # epi 1 (pool) without the partial-sum buffer, epi 3 (pixel shuffle) without yb
    for epi in (4, 2, 1, 3):
        for dtype in (0, 1):
            args = [dummy, dummy, None, 1, 4, 48, 64, 256 if epi == 3 else 64, 0, epi, None, None, None, None, None,
                    None, None, 1.0, dtype, None]
            assert lib.srmi_conv3x3(*args) == -10001, (epi, dtype, "expected SRMI_ERR_ARG")
    # an unknown dtype is refused too
    args = [dummy, dummy, dummy, 1, 4, 48, 64, 64, 0, 0, dummy, None, None, None, None, None, None, 1.0, 7, None]
    assert lib.srmi_conv3x3(*args) == -10001
    # a PixelShuffle pack needs Cout = 256 (its channel permutation spans 4 x 64 outputs):
    # Cout/Cin swapped is refused (SRMI_ERR_SHAPE) instead of reading past the filter
    for dtype in (0, 1):
        assert lib.srmi_pack_conv(dummy, dummy, 64, 256, 1, dummy, dummy, dummy, dtype, None) == -10002


def test_stateless_abi_return_codes():
    """The stateless entry points (defined beside their kernels) refuse bad arguments with
    the documented code, and where two checks reject the same call, with the first one's.
    Every case fails validation before any HIP call, so this needs no GPU."""
    import ctypes as C
    from srmi import _lib
    lib = _lib.load()
    ARG, SHAPE = -10001, -10002
    d = C.c_void_p(16)  # never dereferenced: every case below fails validation first
    nbytes = C.c_size_t()
    nan = float("nan")
    cases = [
        # small.hip: the loss sums
        ("tile_loss_parts pred NULL", lib.srmi_tile_loss_parts, (None, d, 1, 64, 0, 0.0, d, None), ARG),
        ("tile_loss_parts kind 2", lib.srmi_tile_loss_parts, (d, d, 1, 64, 2, 0.0, d, None), ARG),
        ("loss_from_parts kind -2", lib.srmi_loss_from_parts, (d, 1, 64.0, -2, d, None), ARG),
        ("loss_combine nparts 0", lib.srmi_loss_combine, (d, d, 0, 0, None), ARG),
        # small.hip: the optimizer
        ("adam_step step 0", lib.srmi_adam_step, (d, d, d, d, 4, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, None), ARG),
        ("adam_step_guarded ctl NULL", lib.srmi_adam_step_guarded,
         (d, d, d, d, None, 4, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, None, None), ARG),
        ("adam_step_guarded ema_decay 1", lib.srmi_adam_step_guarded,
         (d, d, d, d, d, 4, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, d, None), ARG),
        ("grad_norm_workspace n 0", lib.srmi_grad_norm_workspace, (0, C.byref(nbytes)), ARG),
        ("grad_norm_workspace bytes NULL", lib.srmi_grad_norm_workspace, (4, None), ARG),
        ("grad_norm max_norm 0", lib.srmi_grad_norm, (d, 4, 0.0, d, 1 << 20, d, None), ARG),
        ("grad_norm max_norm NaN", lib.srmi_grad_norm, (d, 4, nan, d, 1 << 20, d, None), ARG),
        ("grad_norm workspace misaligned", lib.srmi_grad_norm, (d, 4, 1.0, C.c_void_p(20), 1 << 20, d, None), ARG),
        # small.hip and tiles.hip: pointer and dtype checks that stood in the forwarders
        ("region_to_tiles mean NULL", lib.srmi_region_to_tiles, (d, 1, 48, 48, 48, 48, d, None, d, None, None), ARG),
        ("tiles_to_region std NULL", lib.srmi_tiles_to_region, (d, d, None, None, 1, 48, 48, 1, 1, d, None), ARG),
        ("axpy x NULL", lib.srmi_axpy, (d, None, 1.0, 4, None), ARG),
        ("llc_index_map_workspace bytes NULL", lib.srmi_llc_index_map_workspace, (13, None), ARG),
        ("pack_conv dtype 7", lib.srmi_pack_conv, (d, d, 64, 64, 0, d, d, d, 7, None), ARG),
        # the order of checks: the shape before the pointers
        ("tiles_nonfinite C 0, region NULL", lib.srmi_tiles_nonfinite, (None, 0, 48, 48, 48, 48, d, None), SHAPE),
        ("tiles_nonfinite region NULL", lib.srmi_tiles_nonfinite, (None, 1, 48, 48, 48, 48, d, None), ARG),
        ("upsample scale 0", lib.srmi_upsample, (d, 1, 1, 48, 48, 0, d, None), SHAPE),
        # tiles.hip: the tile count of an overlapped axis
        ("overlap_count stride 0", lib.srmi_overlap_count, (10, 4, 0), ARG),
        ("overlap_count one tile", lib.srmi_overlap_count, (48, 48, 48), 1),
        ("overlap_count shifted last tile", lib.srmi_overlap_count, (100, 48, 26), 3),
        # the score and loss files
        ("ssim_workspace H 10", lib.srmi_ssim_workspace, (1, 10, 48, C.byref(nbytes)), ARG),
        ("ssim_workspace bytes NULL", lib.srmi_ssim_workspace, (1, 48, 48, None), ARG),
        ("ssim_loss_from_parts nplanes 0", lib.srmi_ssim_loss_from_parts, (d, d, 0, 1.0, d, d, d, None), ARG),
        ("spectra_workspace bytes NULL", lib.srmi_spectra_workspace, (1, 64, 64, 32, 16, None), ARG),
        ("spectral_loss_from_parts P 8", lib.srmi_spectral_loss_from_parts, (d, d, 1, 8, 1.0, d, d, d, None), ARG),
        ("quantile_map_fit nbins 1", lib.srmi_quantile_map_fit, (d, d, 1, 1, None, 0, d, d, d, None), ARG),
    ]
    for name, fn, args, want in cases:
        assert fn(*args) == want, name


def _force_dp_rank(port, q):
    import os as _os
    import sys as _sys
    _sys.path[:0] = [_os.path.join(ROOT, "super-resolution-climate_amd"), ROOT]
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        _os.environ.pop(k, None)
    _os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from srmi.dist import allreduce_sum_, init_from_env
    info = init_from_env("gloo", force=True)
    t = torch.tensor([3.0])
    allreduce_sum_(t, info)
    q.put((info.enabled, info.world, dist.get_world_size(), float(t)))
    dist.destroy_process_group()


def test_force_dp_single_rank_gloo():
    """bench.py --force-dp: the data-parallel path (process group, collectives) at
    world size 1, used to measure its on-GPU cost without a second GPU."""
    import multiprocessing as mp
    import random
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_force_dp_rank, args=(29500 + random.randint(2001, 4000), q))
    p.start()
    enabled, world, pg_world, v = q.get(timeout=120)
    p.join(timeout=60)
    assert p.exitcode == 0
    assert enabled and world == 1 and pg_world == 1 and v == 3.0


def _rr_rank(rank, world, port, q):
    import sys
    sys.path[:0] = [os.path.join(ROOT, "super-resolution-climate_amd"), ROOT]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from srmi.dist import init_from_env
    from srmi.inference import gather_round_robin
    init_from_env("gloo")
    n = 11
    mine = torch.arange(rank, n, world, dtype=torch.float32)[:, None] * torch.tensor([[1.0, -1.0]])
    out = gather_round_robin(mine, n, world)
    q.put((rank, out.numpy()))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_round_robin_tile_gather_world_gloo(world):
    """Multi-rank tiled inference deals the grid tiles round-robin (rank r: tiles
    r, r + W, ...) and all-gathers them back into grid order (srmi.inference,
    SURVEY.md §8(e)); 11 tiles leave the ranks with unequal counts."""
    import multiprocessing as mp
    import random
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35000 + random.randint(0, 2000)
    ps = [ctx.Process(target=_rr_rank, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=120) for _ in ps]
    for p in ps:
        p.join(timeout=30)
        assert p.exitcode == 0
    exp = np.arange(11, dtype=np.float32)[:, None] * np.array([[1.0, -1.0]], dtype=np.float32)
    for _, out in res:
        np.testing.assert_array_equal(out, exp)


def test_netspec_batch_norm_rcan_ignored_edsr_refused():
    """RCAN's RCABs hard-code bn=False (sres/model/rcan/network.py:70), so the key is
    ignored, as the reference does; EDSR passes it to its ResBlocks (edsr/network.py:15)."""
    from srmi import _lib
    from srmi.engine import NetSpec
    parms = dict(nchannels_in=2, nchannels_out=2, nfeatures=64, nlayers=10, nblocks=20, scale=4, batch_norm=True)
    assert NetSpec.from_parms("rcan", parms) == NetSpec.from_parms("rcan", dict(parms, batch_norm=False))
    with pytest.raises(_lib.SrmiError, match="batch_norm"):
        NetSpec.from_parms("edsr", dict(parms, nblocks=0, scale=8))


def test_flag_constants_match_header():
    """The Python names of srmi_model_config.flags bits are the header's values, and the
    engine refuses the retired bits (0 and 3) and any unknown bit."""
    import ctypes as C
    from srmi import _lib
    from srmi.engine import NetSpec
    hdr = open(os.path.join(ROOT, "include", "srmi.h")).read()
    defs = dict((k, int(v)) for k, v in re.findall(r"#define (SRMI_FLAG_[A-Z_]+) (\d+)", hdr))
    assert set(defs) == {"SRMI_FLAG_NO_RCAB_INFER", "SRMI_FLAG_CA_PASS", "SRMI_FLAG_DU_PASS"}
    for k, v in defs.items():
        assert getattr(_lib, k) == v, k
    tb = C.c_size_t()
    for bad in (1, 8, 32):
        cfg = NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nlayers=1, nblocks=2, flags=bad).cstruct(4, 48, 48)
        with pytest.raises(_lib.SrmiError):
            _lib.call("srmi_workspace_size", C.byref(cfg), 1, C.byref(tb))
    cfg = NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nlayers=1, nblocks=2,
                  flags=sum(defs.values())).cstruct(4, 48, 48)
    _lib.call("srmi_workspace_size", C.byref(cfg), 1, C.byref(tb))
