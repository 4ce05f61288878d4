"""The in-image expansion of the MFMA block kernels (csrc/yf_mres_kernels.hip, mres_kernel XS) against the bits of a recorded parent.

mres_kernel expands only the region pixels of a tile that lie inside the image and leaves the depthwise conv's zero padding as zeros
written once.  Which pixels a tile expands, and which wave and slot computes each, depends on where the tile sits in the frame; the
values must not: every in-image pixel sees the MFMAs it saw before, in the same order.  tests/golden/mres_inimage_parent_heads.npz
holds both head tensors of the commit named in its `parent` entry -- the last one whose kernels expand the whole halo'd region -- on an
MI355X, with seeded random weights (tests/random_weights.py) on seeded u8 noise; the test is torch.equal on both heads.

The cases are chosen by their tile grid at stride 8 (16x20-pixel tiles; test_sizes_reach_every_tile_position checks the grids on the
CPU).  The conv4_2 triple's expanded tensor feeds the large head, so head_large covers its writeback from the new pixel mapping.
  b2_128x160        16x20 at stride 8: the one tile of the frame touches all four borders (16x20 of its 18x22 region pixels are inside)
  b3_256x320        32x40: 2x2 tiles, every one a corner (17x21): the three-slot form of the 16x20 tiles
  b2_384x480        48x60: 3x3 tiles: corners, all four kinds of edge (17x22, 18x21) and an interior tile (18x22): the frame keeps the
                    full-region form of the 16x20 tiles; the stride-2 triples and the few-frames 8x10 / 8x4 tiles meet every position too
  b2_288x352        36x44: 3x3 tiles whose last row and column are partial (4 of 16 rows, 4 of 20 columns): short rectangles, waves with
                    no expansion tile at all
  b2_256x320_f16x3  the split-operand instantiations of the shared template
  b2_256x320_f16    the fp16-storage instantiations
What these cases do NOT reach.  A frame with an interior tile (b2_384x480, b2_288x352) keeps the full-region form of the 16x20 tiles, so
the three-slot form of that tiling runs here on corner tiles (256x320) and on the single tile (128x160) only: its edge tiles (17x22,
18x21: 24 M-tiles) and partial tiles are compared with the parent through the 8x10 / 8x4 tilings' in-image form, which shares the code,
not through the 16x20 instantiation itself (a 2x3 or 3x2 grid such as 256x480, or 288x320 for partial tiles, would do that).  At batch 2
and 3 res3_3 .. res3_6 and the stride-2 triples behind them take the few-frames 8x10 / 8x4 tiles, so mres_kernel<16,96,16> on 16x20
tiles and the 8x10-tile conv4_2 triple with its writeback are pinned by b129_256x320 of tests/test_gpu_mres_bits.py alone.

`python tests/test_gpu_mres_inimage.py --record <commit>` on a built checkout of that commit rewrites the fixture."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mres_inimage_parent_heads.npz")
WEIGHT_SEED = 5

#        name              batch  H    W   seed  precision
CASES = [("b2_128x160", 2, 128, 160, 21, None),
         ("b3_256x320", 3, 256, 320, 22, None),
         ("b2_384x480", 2, 384, 480, 23, None),
         ("b2_288x352", 2, 288, 352, 24, None),
         ("b2_256x320_f16x3", 2, 256, 320, 25, "f16x3"),
         ("b2_256x320_f16", 2, 256, 320, 26, "f16")]

TH, TW = 16, 20   # the stride-8 tiles of mres_kernel (yf_mres_kernels.hip, YF_MRES_SHAPES)


def _tile_kinds(H, W):
    """In-image size of the halo'd region (18 x 22) of every 16x20 tile of the stride-8 grid of an H x W frame."""
    gh, gw = H // 8, W // 8
    kinds = set()
    for oy0 in range(0, gh, TH):
        for ox0 in range(0, gw, TW):
            rows = sum(0 <= oy0 - 1 + r < gh for r in range(TH + 2))
            cols = sum(0 <= ox0 - 1 + c < gw for c in range(TW + 2))
            kinds.add((rows, cols))
    return kinds


def test_sizes_reach_every_tile_position():
    sizes = {name: (H, W) for name, _, H, W, _, _ in CASES}
    assert _tile_kinds(*sizes["b2_128x160"]) == {(16, 20)}
    assert _tile_kinds(*sizes["b3_256x320"]) == {(17, 21)}
    assert _tile_kinds(*sizes["b2_256x320_f16x3"]) == {(17, 21)} and _tile_kinds(*sizes["b2_256x320_f16"]) == {(17, 21)}
    assert _tile_kinds(*sizes["b2_384x480"]) == {(17, 21), (17, 22), (18, 21), (18, 22)}
    # partial last tile row and column: 36 = 16 + 16 + 4 rows, 44 = 20 + 20 + 4 columns; their regions keep 5 rows / 5 columns
    assert _tile_kinds(*sizes["b2_288x352"]) == {(17, 21), (17, 22), (17, 5), (18, 21), (18, 22), (18, 5), (5, 21), (5, 22), (5, 5)}


def _heads(yf, dev, batch, H, W, seed, precision):
    from tests.random_weights import random_state_dict
    io = dict(yf.io_params_for(256))
    io["input_shape"] = [H, W, 1]
    m = yf.YoloFastest(io).to(dev).eval()
    m.load_state_dict(random_state_dict(WEIGHT_SEED))
    m.precision = precision
    u8 = np.random.default_rng(seed).integers(0, 256, size=(batch, 1, H, W), dtype=np.uint8)
    x = ((torch.from_numpy(u8).float() - 128.0) / 255.0).to(dev)
    with torch.no_grad():
        hl, hs = m(x)
    torch.cuda.synchronize()
    return hl.float().cpu(), hs.float().cpu()


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE)


@pytest.mark.gpu
@pytest.mark.parametrize("name,batch,H,W,seed,precision", CASES, ids=[c[0] for c in CASES])
def test_heads_are_the_parents_bits(parent, name, batch, H, W, seed, precision):
    import yolo_fastest_amd as yf
    assert torch.cuda.is_available()
    hl, hs = _heads(yf, torch.device("cuda:0"), batch, H, W, seed, precision)
    assert len(str(parent["parent"])) == 40
    want_l, want_s = torch.from_numpy(parent[name + "_large"]), torch.from_numpy(parent[name + "_small"])
    assert hl.shape == want_l.shape and hs.shape == want_s.shape
    assert torch.isfinite(hl).all() and torch.isfinite(hs).all() and hl.abs().max() > 0 and hs.abs().max() > 0
    assert torch.equal(hl, want_l), f"large head: {(hl != want_l).sum().item()} values differ from the parent's"
    assert torch.equal(hs, want_s), f"small head: {(hs != want_s).sum().item()} values differ from the parent's"


def _record(commit):
    sys.path.insert(0, ROOT)
    import yolo_fastest_amd as yf
    out = {"parent": np.array(commit)}
    for name, batch, H, W, seed, precision in CASES:
        hl, hs = _heads(yf, torch.device("cuda:0"), batch, H, W, seed, precision)
        hl, hs = hl.numpy(), hs.numpy()
        out[name + "_large"], out[name + "_small"] = hl, hs
        print(name, tuple(hl.shape), tuple(hs.shape), float(np.abs(hl).max()), float(np.abs(hs).max()))
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record" and len(sys.argv[2]) == 40, __doc__
    _record(sys.argv[2])
