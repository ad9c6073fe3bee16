"""The time-slice feed on the GPU (srmi.feed, srmi.llc's read plan; srmi_llc_block_mask
/ srmi_llc_compact_map / srmi_tiles_keep / srmi_tiles_gather_dev through the C ABI)
against the existing whole-file path, LLCSource.load_region_data + get_tiles, whose
outputs tests/test_gpu_llc.py pins to the reference's.  Everything is compared bit for
bit (int32 views, so NaNs count).

Inputs: a small LLC geometry (nx = 384) from the llc_synth functions, a ROI across the
east/west seam, two variables, three time slices.  At tile 48 the ROI is a 6 x 10 grid
in which the template's land drops cells (0,0), (0,1), (1,0), (1,1), (5,8), (5,9) of
each channel; slice 1 has a NaN in ONE wet value of variable 1 only, so its keep count
is odd and the last kept plane is dropped (get_tiles, raw.py:216-233)."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import llc_synth  # noqa: E402
from srmi._lib import call, ptr, stream_handle  # noqa: E402
from srmi.feed import TimesliceFeed  # noqa: E402
from srmi.llc import LLCSource, get_tiles  # noqa: E402

NX = 384
ROI = dict(y0=300, ys=288, x0=528, xs=480)
NVARS, NSLICES, TILE = 2, 3, 48
NAN_SLICE, NAN_PIXEL = 1, (100, 200)  # ROI pixel (y, x): tile (2, 4)


def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> dict(root, tmpl path, paths[i][v], idx (wet index of every wet ROI pixel), n_wet)."""
    root = tmp_path_factory.mktemp("feed")
    tmpl = llc_synth.template(NX, ROI)
    tpath = str(root / "tmpl.data")
    tmpl.astype(">f4").tofile(tpath)
    wet = tmpl != 0
    rank = np.cumsum(wet) - 1
    ys, xs = np.meshgrid(np.arange(ROI["y0"], ROI["y0"] + ROI["ys"]), np.arange(ROI["x0"], ROI["x0"] + ROI["xs"]),
                         indexing="ij")
    cell = llc_synth.llc_index(ys.ravel(), xs.ravel(), NX)
    nan_cell = int(llc_synth.llc_index(ROI["y0"] + NAN_PIXEL[0], ROI["x0"] + NAN_PIXEL[1], NX))
    assert wet[nan_cell]
    paths = []
    for i in range(NSLICES):
        row = []
        for v in range(NVARS):
            vals = llc_synth.wet_values(tmpl, NVARS * i + v)
            if i == NAN_SLICE and v == 1:
                vals[rank[nan_cell]] = np.nan
            p = str(root / f"t{i}_var{v}.data")
            vals.astype(">f4").tofile(p)
            row.append(p)
        paths.append(row)
    return dict(root=root, tmpl=tpath, paths=paths, idx=rank[cell][wet[cell]], n_wet=int(wet.sum()))


@pytest.fixture(scope="module")
def source(data):
    return LLCSource(data["tmpl"], roi=ROI, nx=NX, device=dev())


@pytest.fixture(scope="module")
def existing(data, source):
    """The existing path's result per slice, computed once: (region, tiles, ids, grid)."""
    out = []
    for p in data["paths"]:
        region = source.load_region_data(p)
        tiles, ids, grid = get_tiles(region, TILE, TILE)
        out.append((region, tiles, np.asarray(ids), grid))
    torch.cuda.synchronize()
    assert [t.shape[0] for _, t, _, _ in out] == [54, 53, 54] and out[0][3] == (6, 10)
    dropped = sorted(set(range(60)) - set(out[0][2].tolist()))
    assert dropped[:4] == [0, 1, 10, 11] and len(out[0][2]) == 54  # ids: the first n kept flags (channel 0's)
    return out


# ------------------------------------------------------------------ kernels
def keep_numpy(bad, C):
    keep = np.flatnonzero(bad == 0)
    n = keep.size // C
    return keep[:n * C], n, keep.size


@pytest.mark.parametrize("ncells", [1, 63, 64, 65, 1023, 1025, 4097])
def test_tiles_keep_matches_numpy(ncells):
    rng = np.random.RandomState(ncells)
    for C in (1, 2, 3):
        total = C * ncells
        pats = [np.zeros(total, np.int32), np.ones(total, np.int32), (rng.rand(total) < 0.4).astype(np.int32),
                (rng.rand(total) < 0.97).astype(np.int32)]
        odd = (rng.rand(total) < 0.5).astype(np.int32)  # a pattern with len(keep) % C != 0 (C > 1)
        if C > 1 and (total - int(odd.sum())) % C == 0:
            k = int(np.flatnonzero(odd == 0)[-1]) if (odd == 0).any() else 0
            odd[k] = 1 - odd[k]
        pats.append(odd)
        for bad in pats:
            want, n, nkeep = keep_numpy(bad, C)
            if bad is odd and C > 1:
                assert nkeep % C != 0
            dbad = torch.from_numpy(bad).to(dev())
            src = torch.full((total,), -7, dtype=torch.int32, device=dev())
            count = torch.full((2,), -7, dtype=torch.int32, device=dev())
            call("srmi_tiles_keep", ptr(dbad), C, ncells, ptr(src), ptr(count), stream_handle())
            assert count.tolist() == [n, nkeep]
            got = src.cpu().numpy()
            np.testing.assert_array_equal(got[:n * C], want)
            assert np.all(got[n * C:] == -7)  # nothing is stored past n * C


@pytest.mark.parametrize("C,H,W,t", [(2, 100, 150, 48), (1, 64, 40, 20), (3, 70, 66, 32)])
def test_tiles_gather_dev_matches_tiles_gather(C, H, W, t):
    g = torch.Generator().manual_seed(3)
    region = torch.randn(C, H, W, generator=g)
    gy, gx = H // t, W // t
    region[C - 1, t // 2, t + 1] = float("nan")            # drops cell (0, 1) of the last channel
    if C > 1:
        region[0, (gy - 1) * t, 0] = float("inf")          # and cell (gy - 1, 0) of channel 0
    region = region.to(dev())
    ncells = gy * gx
    st = stream_handle()
    bad = torch.empty(C * ncells, dtype=torch.int32, device=dev())
    call("srmi_tiles_nonfinite", ptr(region), C, H, W, t, t, ptr(bad), st)
    src = torch.full((C * ncells,), -1, dtype=torch.int32, device=dev())
    count = torch.zeros(2, dtype=torch.int32, device=dev())
    call("srmi_tiles_keep", ptr(bad), C, ncells, ptr(src), ptr(count), st)
    n, nkeep = count.tolist()
    assert nkeep == C * ncells - (2 if C > 1 else 1) and n == nkeep // C
    sentinel = -12345.0
    out = torch.full((C * ncells, t, t), sentinel, dtype=torch.float32, device=dev())
    call("srmi_tiles_gather_dev", ptr(region), C, H, W, t, t, ptr(src), ptr(count), C * ncells, ptr(out), st)
    ref = torch.empty(n * C, t, t, dtype=torch.float32, device=dev())
    call("srmi_tiles_gather", ptr(region), C, H, W, t, t, ptr(src), n * C, ptr(ref), st)
    torch.cuda.synchronize()
    assert torch.equal(bits(out[:n * C]), bits(ref))
    assert n * C < C * ncells and bool((out[n * C:] == sentinel).all())  # the planes it must not write
    tiles, ids, _ = get_tiles(region, t, t)
    assert torch.equal(bits(out[:n * C]), bits(tiles.reshape(n * C, t, t)))
    assert src[:n].tolist() == list(ids)


def host_words(idx, n_wet, bw, gap):
    touched = sorted(set((idx // bw).tolist()))
    blocks, prev = 0, None
    for b in touched:
        blocks += 1 if (prev is None or b - prev - 1 > gap) else b - prev
        prev = b
    words = blocks * bw
    if touched[-1] == (n_wet - 1) // bw:
        words -= (touched[-1] + 1) * bw - n_wet
    return words


@pytest.mark.parametrize("bw,gap", [(256, 0), (256, 1), (1024, 0), (1024, 1)])
def test_sparse_read_equals_full_read(data, source, existing, bw, gap):
    assert source.n_wet == data["n_wet"]
    plan = source.read_plan(bw, gap)
    assert plan.nbytes == 4 * host_words(data["idx"], data["n_wet"], bw, gap)
    assert plan.nbytes < 2 * data["n_wet"]  # under half of the file
    npix = source.ys * source.xs
    for i in (0, NAN_SLICE):
        region = torch.empty(NVARS, source.ys, source.xs, dtype=torch.float32, device=dev())
        for v, p in enumerate(data["paths"][i]):
            pinned = torch.empty(plan.n_words, dtype=torch.int32).pin_memory()
            plan.read_into(p, pinned)
            words = pinned.to(dev())
            call("srmi_llc_gather", ptr(words), plan.n_words, ptr(plan.idx), npix, ptr(region[v]), stream_handle())
        torch.cuda.synchronize()
        assert torch.equal(bits(region), bits(existing[i][0]))


def test_block_mask_refuses_an_index_past_the_blocks(source):
    from srmi._lib import SrmiError
    npix = source.ys * source.xs
    n_blocks = -(-source.n_wet // 256)
    mask = torch.empty(n_blocks, dtype=torch.int32, device=dev())
    call("srmi_llc_block_mask", ptr(source.idx), npix, 8, ptr(mask), n_blocks, stream_handle())
    few = int(source.idx.max()) >> 8  # one block short of the last one the ROI touches
    guard = torch.full((few + 1,), -3, dtype=torch.int32, device=dev())
    with pytest.raises(SrmiError, match="SRMI_ERR_SHAPE"):
        call("srmi_llc_block_mask", ptr(source.idx), npix, 8, ptr(guard), few, stream_handle())
    assert int(guard[few]) == -3  # and nothing was stored past the mask


# --------------------------------------------------------------------- feed
@pytest.mark.parametrize("depth", [2, 1])
def test_feed_equals_the_existing_path(data, source, existing, depth):
    got = []
    with TimesliceFeed(source, data["paths"], TILE, depth=depth, block_words=256) as feed:
        for i in list(range(NSLICES)) * 2:  # two epochs: the index wraps, every slot is reused
            tiles, ids, grid = feed.timeslice(i)
            got.append((i, tiles.clone(), ids.copy(), grid))
            tiles.mul_(0.0)  # the consumer may do what it likes with a slice it holds
        torch.cuda.synchronize()
        st = feed.stats()
    # compared only now, after every slice was requested: a slot overwritten early would show
    for i, tiles, ids, grid in got:
        _, rt, rids, rgrid = existing[i]
        assert tiles.shape == rt.shape and torch.equal(bits(tiles), bits(rt))
        assert ids.dtype == rids.dtype and np.array_equal(ids, rids) and grid == rgrid
    assert got[NAN_SLICE][1].shape[0] == 53
    assert len(st["read_s"]) >= 6 and all(b == NVARS * feed.plan.nbytes for b in st["read_bytes"])
    assert len(st["count_wait_s"]) == 6 and len(st["enqueue_s"]) >= 6


def test_feed_missing_file_raises_from_timeslice(data, source, existing):
    paths = [list(p) for p in data["paths"]]
    paths[2][1] = str(data["root"] / "no_such_file.data")
    feed = TimesliceFeed(source, paths, TILE)
    try:
        for i in (0, 1):
            tiles, _, _ = feed.timeslice(i)
            assert torch.equal(bits(tiles), bits(existing[i][1]))
        with pytest.raises(OSError):
            feed.timeslice(2)
        tiles, _, _ = feed.timeslice(0)  # the feed goes on
        assert torch.equal(bits(tiles), bits(existing[0][1]))
    finally:
        feed.close()
    assert not any(t.is_alive() for t in feed._threads)


def test_feed_norm_stats_and_dataset_norm_prepare(data, source, existing):
    """feed.norm_stats() is NormStats.compute over the existing path's tiles (slices 0 and
    2: the statistics need equal tile counts), and feed.prepare with a dataset norm is
    prep_batch on the same rows, into the feed's reused buffer."""
    from srmi.batch import prep_batch
    from srmi.norm import NormStats
    paths = [data["paths"][0], data["paths"][2]]
    ref = NormStats.compute([existing[0][1], existing[2][1]])
    with TimesliceFeed(source, paths, TILE, block_words=256) as feed:
        stats = feed.norm_stats()
        assert torch.equal(bits(stats.tiles), bits(ref.tiles)) and torch.equal(bits(stats.globals), bits(ref.globals))
        with pytest.raises(ValueError):
            feed.prepare("tnorm")
        raw = feed.timeslice(1)[0]
        for norm in ("tnorm", "gscale", "lscale"):
            prep = feed.prepare(norm, stats)
            for start, b, flip in ((0, 16, 5), (48, 6, 0)):
                hr = prep(raw[start:start + b], start, b, flip)
                want = prep_batch(existing[2][1][start:start + b], flip, 4, with_lr=False, norm=norm, stats=ref,
                                  tile_range=(start, start + b))["hr"]
                torch.cuda.synchronize()
                assert hr.shape == want.shape and torch.equal(bits(hr), bits(want)), (norm, start)
        assert prep(raw[:0], 0, 16, 3).shape[0] == 0  # a rank without a tile of the batch


class _Losses:
    """LossRecords' interface, keeping the floats."""

    def __init__(self):
        self.rows = []

    def refresh_state(self):
        pass

    def record_losses(self, tset, epoch, loss, ref_loss, flush=False):
        self.rows.append((epoch, loss, ref_loss))

    def flush(self):
        pass


@pytest.mark.parametrize("norm", ["lnorm", "lscale"])
def test_training_over_the_feed_equals_training_over_resident_tiles(data, source, norm):
    """RCAN (1 group, 2 blocks), two variables, tile 64, batch 16 (two micro-batch
    engines; a short last batch of 9), xyflip on: the per-slice losses and the final
    parameters of train_timeslices over the feed equal, bit for bit, those over tiles
    loaded up front by the existing path with the same prepare.  The model is x2, so
    the LR input is 32 x 32: the engine takes LR widths that are multiples of 32 or 48
    (srmi_engine_create), and a x4 model's 16 x 16 is not one."""
    from srmi.engine import NetSpec
    from srmi.harness import train_timeslices
    from srmi.trainer import FusedTrainer
    spec = NetSpec(arch="rcan", nchannels_in=2, nchannels_out=2, nlayers=1, nblocks=2, scale=2)
    paths = data["paths"][:2]
    resident = [get_tiles(source.load_region_data(p), 64, 64)[0] for p in paths]
    assert [t.shape[0] for t in resident] == [25, 24]  # slice 1's NaN tile: 49 kept planes, the last one dropped
    runs = []
    with TimesliceFeed(source, paths, 64, block_words=256) as feed:
        prepare = feed.prepare(norm)
        for slices in (feed.timeslices(), [lambda i=i: resident[i] for i in range(2)]):
            tr = FusedTrainer(spec, 16, (32, 32), device=dev(), seed=5)
            assert tr.micro == 2
            rec = _Losses()
            train_timeslices(tr, slices, 2, 16, records=rec, refresh_state=True, rng=random.Random(9),
                             prepare=prepare, xyflip=True)
            torch.cuda.synchronize()
            runs.append((rec.rows, tr.params.clone()))
    (la, pa), (lb, pb) = runs
    assert len(la) == 2 and la == lb and all(np.isfinite(r[1]) for r in la)
    assert torch.equal(bits(pa), bits(pb))
