"""The MFMA block kernels (csrc/yf_mres_kernels.hip) against the bits of a recorded parent commit.

tests/golden/mres_parent_heads.npz holds the two head tensors that the commit named in its `parent` entry produces on an MI355X with
the shipped 256x320 weights, fp32, default fusion, on seeded u8 noise, (u8 - 128) / 255.  Changes to what these kernels ISSUE around
their arithmetic (instruction order, register use, scheduling pins) must leave every bit where it was: torch.equal on both heads.

The cases and the launches they reach (the launch forms depend on the batch: yf_mres_kernels.hip, launch_mres):
  b2_96x96     one partial 16x20 tile at stride 8 (res3_1 / res3_2, conv3_2 triple), the 8x10- and 8x4-tile few-frames forms
               of the other blocks, guarded last M-tiles
  b2_160x224   20x28 at stride 8: the 2x2 tiles are partial both ways, ragged edges in the stride-2 triples
  b3_256x320   the stride-16 / stride-32 chains at a few frames: res4 block by block on the producer/consumer kernel's 8x10
               tiles, res5 (+ conv5_2) on the split-sum launches
  b40_160x224  enough workgroups for the many-frames forms at a ragged size: partial 16x20 tiles in res3_3 .. res3_6 (16/96/16)
  b129_256x320 the CHAINED res4 and res5 (+ conv5_2) launches, one workgroup per frame, which only batches above half the CU
               count select
The two large batches are stored as their last frame plus a SHA-256 of both whole tensors.

`python tests/test_gpu_mres_bits.py --write <commit>` on a checkout of that commit (built) rewrites the fixture."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_256x320_epoch28.pth")
FIXTURE = os.path.join(ROOT, "tests", "golden", "mres_parent_heads.npz")

#        name            batch  H    W   seed  stored whole
CASES = [("b2_96x96", 2, 96, 96, 11, True),
         ("b2_160x224", 2, 160, 224, 12, True),
         ("b3_256x320", 3, 256, 320, 13, True),
         ("b40_160x224", 40, 160, 224, 14, False),
         ("b129_256x320", 129, 256, 320, 15, False)]


def _digest(hl, hs):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(hl).tobytes())
    h.update(np.ascontiguousarray(hs).tobytes())
    return h.hexdigest()


def _heads(yf, dev, batch, H, W, seed):
    io = dict(yf.io_params_for(256))
    io["input_shape"] = [H, W, 1]
    m = yf.YoloFastest(io).to(dev).eval()
    m.load_state_dict(torch.load(WEIGHTS, map_location=dev))
    u8 = np.random.default_rng(seed).integers(0, 256, size=(batch, 1, H, W), dtype=np.uint8)
    x = ((torch.from_numpy(u8).float() - 128.0) / 255.0).to(dev)
    with torch.no_grad():
        hl, hs = m(x)
    torch.cuda.synchronize()
    return hl.cpu(), hs.cpu()


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE)


@pytest.mark.parametrize("name,batch,H,W,seed,whole", CASES, ids=[c[0] for c in CASES])
def test_heads_are_the_parents_bits(parent, name, batch, H, W, seed, whole):
    import yolo_fastest_amd as yf
    assert torch.cuda.is_available()
    hl, hs = _heads(yf, torch.device("cuda:0"), batch, H, W, seed)
    assert len(str(parent["parent"])) == 40
    if not whole:
        assert _digest(hl.numpy(), hs.numpy()) == str(parent[name + "_sha256"]), "some frame's heads differ from the parent's"
        hl, hs = hl[-1:], hs[-1:]
    want_l, want_s = torch.from_numpy(parent[name + "_large"]), torch.from_numpy(parent[name + "_small"])
    assert hl.shape == want_l.shape and hs.shape == want_s.shape
    assert torch.equal(hl, want_l), f"large head: {(hl != want_l).sum().item()} values differ from the parent's"
    assert torch.equal(hs, want_s), f"small head: {(hs != want_s).sum().item()} values differ from the parent's"


def _write(commit):
    sys.path.insert(0, ROOT)
    import yolo_fastest_amd as yf
    out = {"parent": np.array(commit)}
    for name, batch, H, W, seed, whole in CASES:
        hl, hs = _heads(yf, torch.device("cuda:0"), batch, H, W, seed)
        hl, hs = hl.numpy(), hs.numpy()
        if not whole:
            out[name + "_sha256"] = np.array(_digest(hl, hs))
            hl, hs = hl[-1:], hs[-1:]
        out[name + "_large"], out[name + "_small"] = hl, hs
        print(name, hl.shape, hs.shape, float(np.abs(hl).max()), float(np.abs(hs).max()))
    np.savez(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--write" and len(sys.argv[2]) == 40, __doc__
    _write(sys.argv[2])
