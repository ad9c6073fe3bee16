"""The W % 48 == 0 filter gradient (wgrad48_kernel) with a run-time wave index.

Its body is compiled once per role (waves 0-3: four N tiles, the DMA and the bias
gradient; waves 4-7: five N tiles), and a wave finds its first N tile, its taps, its
tile rotation, its DMA groups, its vmcnt counts and its slab addresses from its index
at run time.  A wrong table entry corrupts exactly that wave's own 4 or 5 (tap, 16
input channel) tiles -- 1/9 or 5/36 of the filter, which the whole-filter rel-L2 bar
also catches, but anonymously -- so besides the bars of test_gpu_kernels.py::test_wgrad
(rel-L2 < 1e-5 of the fp64 gradient of the same bf16 operands, bias rtol 1e-4 / atol
1e-3) every (tap, input tile) block is held to the same 1e-5 on its own.

Shapes: rows per chunk 4, 6, 8, 20, 24 at W = 48 (2 row pairs: fewer than the three in
flight; 3: exactly those, and an odd count; 4: the 8-slot dY ring full; 10, 12: the dY
ring and the 10-slot input ring wrap), two chunks an image so the first and the last
row band both occur; W = 96 and 144 for the left, right and
interior column blocks; one and three images; the PixelShuffle form (256 output
channels read through the unshuffle, four output-channel blocks).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

from srmi import _lib  # noqa: E402
from srmi._lib import call, ptr  # noqa: E402

TOL = 1e-5


def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda", 0)


def S():
    return torch.cuda.current_stream().cuda_stream


def nchw(t):
    return t.permute(0, 3, 1, 2)


def rel_l2(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def check(gw, gb, ref_w, ref_b):
    gw = gw.double().cpu()
    whole = rel_l2(gw, ref_w)
    tiles = {(ky, kx, it): rel_l2(gw[:, 16 * it:16 * it + 16, ky, kx], ref_w[:, 16 * it:16 * it + 16, ky, kx])
             for ky in range(3) for kx in range(3) for it in range(4)}
    worst = max(tiles, key=tiles.get)
    print(f"rel-L2 whole {whole:.3e}; worst (ky, kx, input tile) {worst} {tiles[worst]:.3e}")
    assert whole < TOL
    bad = {k: v for k, v in tiles.items() if not v < TOL}
    assert not bad, f"(ky, kx, input tile) blocks over {TOL}: {bad}"
    np.testing.assert_allclose(gb.double().cpu().numpy(), ref_b.numpy(), rtol=1e-4, atol=1e-3)


def run(x, dy, N, H, W, Cout, unshuf, rs):
    d = x.device
    slab = torch.empty(16 << 20, dtype=torch.float32, device=d)
    gw = torch.full((Cout, 64, 3, 3), float("nan"), device=d)
    gb = torch.full((Cout,), float("nan"), device=d)
    call("srmi_wgrad3x3", ptr(x), ptr(dy), N, H, W, Cout, unshuf, rs, ptr(slab), slab.numel() * 4, unshuf, 1.0,
         ptr(gw), ptr(gb), _lib.SRMI_DTYPE_BF16, S())
    torch.cuda.synchronize()
    return gw, gb


# (H, W, row_splits): rows per chunk = H / row_splits
PLAIN = [(8, 48, 2), (12, 48, 2), (16, 48, 2), (40, 48, 2), (48, 48, 2), (8, 96, 1), (8, 144, 1)]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W,rs", PLAIN)
def test_wgrad48_roles(H, W, rs, N):
    d = dev()
    g = torch.Generator(device="cpu").manual_seed(1000 * H + W + N)
    x = torch.randn(N, H, W, 64, generator=g).to(torch.bfloat16).to(d)
    dy = torch.randn(N, H, W, 64, generator=g).to(torch.bfloat16).to(d)
    gw, gb = run(x, dy, N, H, W, 64, 0, rs)
    ref = torch.nn.grad.conv2d_weight(nchw(x).double().cpu(), (64, 64, 3, 3), nchw(dy).double().cpu(), padding=1)
    check(gw, gb, ref, dy.double().cpu().sum((0, 1, 2)))


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", [(4, 48), (8, 96)])
def test_wgrad48_roles_pixelshuffle(H, W, N):
    d = dev()
    g = torch.Generator(device="cpu").manual_seed(2000 * H + W + N)
    x = torch.randn(N, H, W, 64, generator=g).to(torch.bfloat16).to(d)
    dyp = torch.randn(N, 2 * H, 2 * W, 64, generator=g).to(torch.bfloat16).to(d)
    gw, gb = run(x, dyp, N, H, W, 256, 1, 0)
    dy_log = Fn.pixel_unshuffle(nchw(dyp).double().cpu(), 2)
    ref = torch.nn.grad.conv2d_weight(nchw(x).double().cpu(), (256, 64, 3, 3), dy_log, padding=1)
    check(gw, gb, ref, dy_log.sum((0, 2, 3)))
