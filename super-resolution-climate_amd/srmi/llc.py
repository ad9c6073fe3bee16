"""On-disk LLC4320 source -> tiles on the device.

Mirrors the reference's SWOTRawDataLoader (sres/base/source/swot/raw.py):

* ``load_file`` (:133-145): read the '>f4' mask template and a '>f4' wet-value
  file, put the values into the wet cells (land = NaN), split the LLC faces
  (``mds2d``, swot/util.py:3-7), assemble ``east | west.T[::-1]`` and cut the
  ROI (``subset_roi``, :38-45) -> [1, ys, xs];
* ``load_region_data`` (:155-158): the variables stacked -> [C, ys, xs];
* ``get_tiles`` (:216-233): floor tiling, removal of tiles whose mean is not
  finite, and -- reproduced on purpose, as the reference does it -- the
  channel-major flattening that packs consecutive kept tiles of the same
  variable into the channel axis when C > 1.

The host only reads raw file bytes (no decoding); the byte swap, mask
expansion, face rearrangement and ROI cut are HIP kernels (tiles.hip).  The
template -> ROI index map is built once per template on the device (mask scan),
after which each file is one gather.

``LLCSource.read_plan`` is the sparse form of the read for srmi.feed: the file
blocks the ROI touches (srmi_llc_block_mask), merged into extents on the host
(``plan_extents``), and the index map into the compact buffer those extents fill
(srmi_llc_compact_map); ``LLCReadPlan.read_into`` reads them.  ``load_file`` still
reads whole files.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call, ptr, stream_handle


def _read_words(path: str) -> np.ndarray:
    """Raw file bytes as uint32 words (the '>f4' values still big-endian)."""
    b = np.fromfile(path, dtype=np.uint8)
    if b.size % 4:
        raise ValueError(f"{path}: size {b.size} is not a multiple of 4 bytes")
    return b.view(np.uint32)


class LLCSource:
    """template_path: the '>f4' hFacC template (13 * nx^2 cells); roi: the
    dataset's roi dict (y0, ys, x0, xs; missing keys = the full extent) or None."""

    def __init__(self, template_path: str, roi: Optional[Dict] = None, nx: int = 4320,
                 device: Optional[torch.device] = None):
        self.nx = nx
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        H, W = 3 * nx, 4 * nx
        roi = roi or {}
        self.x0, self.xs = int(roi.get("x0", 0)), int(roi.get("xs", W))
        self.y0, self.ys = int(roi.get("y0", 0)), int(roi.get("ys", H))
        self.y0, self.x0 = min(self.y0, H), min(self.x0, W)      # numpy slicing semantics
        self.ys, self.xs = min(self.ys, H - self.y0), min(self.xs, W - self.x0)
        words = _read_words(template_path)
        n = words.size
        if n != 13 * nx * nx:
            raise ValueError(f"template has {n} cells, LLC{nx} needs {13 * nx * nx}")
        tmpl = torch.from_numpy(words.view(np.int32)).to(self.device)
        ws = C.c_size_t(0)
        call("srmi_llc_index_map_workspace", n, C.byref(ws))
        work = torch.empty(ws.value, dtype=torch.uint8, device=self.device)
        self.idx = torch.empty(self.ys * self.xs, dtype=torch.int32, device=self.device)
        nwet = torch.zeros(1, dtype=torch.int64, device=self.device)
        call("srmi_llc_index_map", ptr(tmpl), n, nx, self.y0, self.ys, self.x0, self.xs, ptr(self.idx), ptr(nwet),
             ptr(work), ws.value, stream_handle())
        self.n_wet = int(nwet.item())
        del work, tmpl

    def load_file(self, data_path: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One variable, one time index -> [1, ys, xs] fp32 on the device."""
        words = _read_words(data_path)
        if words.size != self.n_wet:
            # numpy's boolean-mask assignment in the reference raises here too
            raise ValueError(f"{data_path}: {words.size} values for {self.n_wet} wet cells")
        data = torch.from_numpy(words.view(np.int32)).to(self.device)
        if out is None:
            out = torch.empty(1, self.ys, self.xs, dtype=torch.float32, device=self.device)
        call("srmi_llc_gather", ptr(data), words.size, ptr(self.idx), self.ys * self.xs, ptr(out), stream_handle())
        return out

    def load_region_data(self, data_paths: Sequence[str]) -> torch.Tensor:
        """The variables stacked on the channel axis -> [C, ys, xs]."""
        out = torch.empty(len(data_paths), self.ys, self.xs, dtype=torch.float32, device=self.device)
        for c, pth in enumerate(data_paths):
            self.load_file(pth, out=out[c:c + 1])
        return out

    def read_plan(self, block_words: int = 1024, max_gap_blocks: int = 0) -> "LLCReadPlan":
        """The file blocks (of block_words words, a power of two) this ROI touches, as
        extents to read into a compact staging buffer, and the index map into that
        buffer (srmi_llc_block_mask, plan_extents, srmi_llc_compact_map).  Once per
        source; load_file's whole-file read stays as it is."""
        shift = _block_shift(block_words)
        n_blocks = max(1, -(-self.n_wet // block_words))
        mask = torch.empty(n_blocks, dtype=torch.int32, device=self.device)
        st = stream_handle(torch.cuda.current_stream(self.device))
        npix = self.ys * self.xs
        call("srmi_llc_block_mask", ptr(self.idx), npix, shift, ptr(mask), n_blocks, st)
        extents, base, n_words = plan_extents(mask.cpu().numpy(), block_words, max_gap_blocks, self.n_wet)
        dbase = torch.from_numpy(base).to(self.device)
        idx = torch.empty(npix, dtype=torch.int32, device=self.device)
        call("srmi_llc_compact_map", ptr(self.idx), npix, shift, ptr(dbase), n_blocks, ptr(idx), st)
        return LLCReadPlan(extents, base, n_words, self.n_wet, block_words, idx)


def _block_shift(block_words: int) -> int:
    if block_words < 1 or block_words > 1 << 30 or block_words & (block_words - 1):
        raise ValueError(f"block_words {block_words} is not a power of two in 1..2^30")
    return int(block_words).bit_length() - 1


def plan_extents(mask, block_words: int, max_gap_blocks: int, n_wet: int):
    """Host side of the read plan.  mask[b] != 0: file block b (words
    [b * block_words, (b + 1) * block_words), the last one clipped to n_wet) is
    needed.  Runs of needed blocks are merged across gaps of at most max_gap_blocks
    blocks; the gap blocks merged in are read too and get bases of their own.

    -> (extents, block_base, n_words): extents = [(file_word_offset, n_words,
    staging_word_offset)], ascending and disjoint, the staging offsets their running
    sum; block_base int32 [len(mask)] = the staging word offset of each block read,
    -1 for the others; n_words = the words read per file.  ValueError at 2^31
    words (the compact index map is int32)."""
    _block_shift(block_words)
    mask = np.asarray(mask).reshape(-1)
    nb = mask.size
    if max_gap_blocks < 0:
        raise ValueError(f"max_gap_blocks {max_gap_blocks} < 0")
    if nb != -(-n_wet // block_words) and not (n_wet == 0 and nb == 1):
        raise ValueError(f"{nb} blocks of {block_words} words do not cover {n_wet} values exactly")
    base = np.full(nb, -1, dtype=np.int32)
    need = np.flatnonzero(mask)
    if need.size == 0:
        return [], base, 0
    cut = np.flatnonzero(np.diff(need) - 1 > max_gap_blocks)
    first = need[np.r_[0, cut + 1]]           # first and last block of every merged run
    last = need[np.r_[cut, need.size - 1]]
    off = first.astype(np.int64) * block_words
    cnt = np.minimum((last.astype(np.int64) + 1) * block_words, n_wet) - off
    stag = np.cumsum(cnt) - cnt
    n_words = int(cnt.sum())
    if n_words >= 1 << 31:
        raise ValueError(f"the plan reads {n_words} words per file; the compact index map holds 2^31 - 1")
    for b0, b1, s in zip(first.tolist(), last.tolist(), stag.tolist()):
        base[b0:b1 + 1] = s + np.arange(b1 - b0 + 1, dtype=np.int64) * block_words
    extents = [(int(o), int(c), int(s)) for o, c, s in zip(off, cnt, stag)]
    return extents, base, n_words


class LLCReadPlan:
    """What LLCSource.read_plan returns.  extents / block_base / n_words: see
    plan_extents; nbytes = the bytes read per file; idx = the device index map into
    the compact words, for srmi_llc_gather(data = the compact words, n_values =
    n_words, idx_map = idx)."""

    def __init__(self, extents: List[Tuple[int, int, int]], block_base: np.ndarray, n_words: int, n_wet: int,
                 block_words: int, idx: Optional[torch.Tensor] = None):
        self.extents, self.block_base, self.n_words = extents, block_base, int(n_words)
        self.n_wet, self.block_words, self.idx = int(n_wet), int(block_words), idx
        self.nbytes = 4 * self.n_words

    def read_into(self, path: str, pinned_words: torch.Tensor) -> None:
        """The plan's extents of one wet-value file -> pinned_words[:n_words] (a
        4-byte host tensor, usually pinned), raw bytes, no decoding.  File I/O only:
        safe in a reader thread."""
        size = os.path.getsize(path)
        if size != 4 * self.n_wet:
            raise ValueError(f"{path}: {size // 4} values for {self.n_wet} wet cells" if size % 4 == 0 else
                             f"{path}: size {size} is not a multiple of 4 bytes")
        if pinned_words.element_size() != 4 or pinned_words.numel() < self.n_words or \
                not pinned_words.is_contiguous() or pinned_words.device.type != "cpu":
            raise ValueError(f"read_into: need a contiguous host tensor of >= {self.n_words} 4-byte words")
        buf = memoryview(pinned_words.numpy()).cast("B")
        fd = os.open(path, os.O_RDONLY)
        try:
            for off, cnt, stag in self.extents:
                a, e, pos = 4 * stag, 4 * (stag + cnt), 4 * off
                while a < e:
                    got = os.preadv(fd, [buf[a:e]], pos)
                    if got <= 0:
                        raise ValueError(f"{path}: short read at byte {pos}")
                    a += got
                    pos += got
        finally:
            os.close(fd)


def min_wet_pixels(min_wet: float, ty: int, tx: int) -> int:
    """A min_wet fraction of the ty x tx tile plane as the pixel count the C ABI takes:
    max(1, ceil(min_wet * ty * tx)), as srmi.superres."""
    if not 0.0 < float(min_wet) <= 1.0:
        raise ValueError(f"min_wet {min_wet!r} outside (0, 1]")
    return max(1, int(math.ceil(float(min_wet) * ty * tx)))


def get_tiles(region: torch.Tensor, ty: int, tx: int,
              min_wet: Optional[float] = None) -> Tuple[torch.Tensor, np.ndarray, Tuple[int, int]]:
    """get_tiles (raw.py:216-233) on a device region [C, H, W] -> (tiles [n//C, C,
    ty, tx], tile ids (the first n//C kept ids of the channel-major flattening, as
    the reference's coords), (gy, gx)).  One host sync for the keep mask (the
    reference does this once per time slice).

    min_wet (no reference counterpart; None: the reference's rule, one non-finite value
    drops the tile): a fraction of the tile plane.  A tile is kept when every channel has
    at least max(1, ceil(min_wet * ty * tx)) finite pixels (srmi_tiles_dry); the kept
    tiles hold their NaN, for prep_batch(land=True) and FusedTrainer(land=True)."""
    if region.dtype != torch.float32 or region.dim() != 3 or not region.is_contiguous():
        raise ValueError("get_tiles: region must be a contiguous fp32 [C, H, W] device tensor")
    Cn, H, W = region.shape
    gy, gx = H // ty, W // tx
    bad = torch.empty(Cn * gy * gx, dtype=torch.int32, device=region.device)
    if min_wet is not None:
        call("srmi_tiles_dry", ptr(region), Cn, H, W, ty, tx, min_wet_pixels(min_wet, ty, tx), ptr(bad), None,
             stream_handle())
    else:
        call("srmi_tiles_nonfinite", ptr(region), Cn, H, W, ty, tx, ptr(bad), stream_handle())
    keep = np.flatnonzero(bad.cpu().numpy() == 0)
    n = keep.size // Cn
    src = torch.from_numpy(keep[:n * Cn].astype(np.int32)).to(region.device)
    tiles = torch.empty(n, Cn, ty, tx, dtype=torch.float32, device=region.device)
    call("srmi_tiles_gather", ptr(region), Cn, H, W, ty, tx, ptr(src), n * Cn, ptr(tiles), stream_handle())
    return tiles, keep[:n], (gy, gx)
