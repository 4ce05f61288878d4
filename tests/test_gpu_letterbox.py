"""yf_cv_letterbox_u8 and yf_scale_boxes on the device, bit for bit against tests/letterbox_ref.py (yolov5's letterbox geometry, the
reference's cvtColor / cv2.resize arithmetic of oracle/cv_oracle.py, a border of 114; yolov5's scale_boxes + round): integer arithmetic
and IEEE double on both sides, so every comparison is an equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

import letterbox_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_256x320_epoch28.pth")
NETS = [(256, 320), (64, 96)]
# (h, w), at 256 x 320: exact 1/2 without a border; the 2x2-mean path with a border (8 rows, 38 rows); new == the net's size but NOT the
# 2x2-mean path; linear with 64 rows of border; portrait, 88 columns left and right; h r = 50.5 -> 50 (half to even); up by 1.009 with the
# odd border (top 0, bottom 1); up by 10.7 with borders 21 / 22; a single row, a single column; portrait small; a row stride of 111 bytes
SIZES = [(512, 640), (480, 640), (360, 640), (511, 640), (512, 1280), (640, 360), (101, 640), (253, 317), (20, 30), (1, 7), (7, 1), (96, 64),
         (48, 37)]
OFFSET_FRAME = (37, 53)           # passed as a view that starts 1 byte into its allocation


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def frames(dev):
    """-> (the host frames, the same on the device: each its own allocation, the last one a view 1 byte into its allocation)"""
    host = []
    for h, w in SIZES + [OFFSET_FRAME]:
        rng = np.random.default_rng(1000 * h + w)
        noise = rng.integers(0, 256, (h, w, 3), dtype=np.int32)
        ramp = (np.arange(w)[None, :, None] * 3 + np.arange(h)[:, None, None] * 2 + np.arange(3)[None, None, :] * 40) % 256
        host.append(((noise // 3 + ramp) % 256).astype(np.uint8))
    on_dev = [torch.from_numpy(f).to(dev) for f in host[:-1]]
    flat = torch.empty(host[-1].size + 1, dtype=torch.uint8, device=dev)
    flat[1:] = torch.from_numpy(host[-1].reshape(-1)).to(dev)
    on_dev.append(flat[1:].view(host[-1].shape))
    assert on_dev[-1].data_ptr() % 2 == 1 and on_dev[-1].is_contiguous()
    return host, on_dev


@pytest.fixture(scope="module")
def want(frames):
    """The reference, once: {(net, gray_bits): [one letterboxed frame per source frame]}"""
    host, _ = frames
    return {(net, bits): [ref.letterbox_u8(f, net[0], net[1], bits) for f in host] for net in NETS for bits in (14, 15, 0)}


class _Table:
    def __init__(self, n, dev):
        from yolo_fastest_amd import _lib
        nb = _lib.YF_LB_TABLE_ENTRY_BYTES * n
        self.dev = torch.empty(nb, dtype=torch.uint8, device=dev)
        self.host = torch.empty(nb, dtype=torch.uint8).pin_memory()
        self.args = (self.dev.data_ptr(), nb, self.host.data_ptr())


def _letterbox(batch, net, bits, dev):
    """yf_cv_letterbox_u8 on a list of device frames -> uint8 numpy [N, H, W(, 3)]"""
    from yolo_fastest_amd import _lib
    n, (H, W) = len(batch), net
    dst = torch.full((n, H, W) if bits else (n, H, W, 3), 7, dtype=torch.uint8, device=dev)
    table = _Table(n, dev)
    ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in batch])
    hs, ws = (ctypes.c_int * n)(*[f.shape[0] for f in batch]), (ctypes.c_int * n)(*[f.shape[1] for f in batch])
    _lib.check(_lib.lib().yf_cv_letterbox_u8(dev.index, n, ptrs, hs, ws, bits, H, W, dst.data_ptr(), *table.args,
                                             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    return dst.cpu().numpy()


@pytest.mark.parametrize("bits", [14, 15, 0])
@pytest.mark.parametrize("net", NETS)
def test_ragged_batch_in_one_call_bit_exact(frames, want, dev, net, bits):
    _, on_dev = frames
    got = _letterbox(on_dev, net, bits, dev)
    for i, w in enumerate(want[net, bits]):
        assert got[i].shape == w.shape and np.array_equal(got[i], w), (i, (SIZES + [OFFSET_FRAME])[i], int((got[i] != w).sum()))


@pytest.mark.parametrize("bits", [14, 15, 0])
@pytest.mark.parametrize("net", NETS)
def test_every_frame_alone_bit_exact(frames, want, dev, net, bits):
    _, on_dev = frames
    for i, w in enumerate(want[net, bits]):
        got = _letterbox([on_dev[i]], net, bits, dev)
        assert np.array_equal(got[0], w), (i, (SIZES + [OFFSET_FRAME])[i], int((got[0] != w).sum()))


def test_the_border_is_114_and_where_the_geometry_says(frames, want):
    """The reference statement itself: what lies outside [top, top + new_h) x [left, left + new_w) is 114 in all channels."""
    host, _ = frames
    for (net, bits), ws in want.items():
        for f, w in zip(host, ws):
            new_h, new_w, top, _, left, _ = ref.geometry(f.shape[0], f.shape[1], *net)
            mask = np.ones(w.shape[:2], dtype=bool)
            mask[top:top + new_h, left:left + new_w] = False
            assert (w[mask] == 114).all()


@pytest.mark.parametrize("bits", [14, 15])
def test_a_frame_of_the_nets_aspect_ratio_is_the_squashing_entrys_bytes(frames, dev, bits):
    """512 x 640 at 256 x 320: exactly 1/2, no border -- yf_cv_preprocess_u8's bytes; through model.letterbox_u8, which also hands back
    the frames' (h, w)."""
    import yolo_fastest_amd as yf
    io = yf.io_params_for(256)
    m = yf.YoloFastest(io).to(dev).eval()
    m.load_state_dict(torch.load(WEIGHTS, map_location=dev))
    _, on_dev = frames
    f = on_dev[0]
    assert tuple(f.shape) == (512, 640, 3)
    squashed = m.cv_preprocess_u8(f[None], io["input_shape"], gray_bits=bits)
    got, hw = m.letterbox_u8([f, on_dev[1]], io["input_shape"], gray_bits=bits)
    assert torch.equal(got[0], squashed[0]) and hw.dtype == torch.int32 and hw.tolist() == [[512, 640], [480, 640]]
    stack, hw2 = m.letterbox_u8(torch.stack([f, f]), io["input_shape"], gray_bits=bits)
    assert torch.equal(stack[0], squashed[0]) and torch.equal(stack[1], squashed[0]) and hw2.tolist() == [[512, 640]] * 2


def test_a_frames_bytes_do_not_depend_on_its_place_in_the_batch(frames, dev):
    _, on_dev = frames
    n = len(on_dev)
    order = list(np.random.default_rng(11).permutation(n))
    assert order != list(range(n))
    a = _letterbox(on_dev, (256, 320), 15, dev)
    b = _letterbox([on_dev[i] for i in order], (256, 320), 15, dev)
    for k, i in enumerate(order):
        assert np.array_equal(b[k], a[i]), (k, i)


K = 8
COUNTS = [0, 1, K, K + 3, -2]


def _scale_case(net, dev):
    """-> (frame sizes, counts, boxes int32 [N, K, 4] with negatives and values past the net, the expected boxes)"""
    sizes = SIZES + [OFFSET_FRAME]
    n = len(sizes)
    counts = np.array([COUNTS[i % len(COUNTS)] for i in range(n)], dtype=np.int32)
    rng = np.random.default_rng(net[0])
    boxes = rng.integers(-40, max(net) + 60, (n, K, 4), dtype=np.int32)
    boxes[:, 0] = [0, 0, net[1], net[0]]                       # the net's own corners
    expect = boxes.copy()
    for f, (h, w) in enumerate(sizes):
        m = min(max(int(counts[f]), 0), K)
        if m:
            expect[f, :m] = np.array(ref.scale_boxes_ref(boxes[f, :m].tolist(), net[0], net[1], h, w), dtype=np.int32)
    return sizes, counts, boxes, expect


@pytest.mark.parametrize("net", NETS)
def test_scale_boxes_plain_and_packed_bit_exact(dev, net):
    import yolo_fastest_amd as yf
    sizes, counts, boxes, expect = _scale_case(net, dev)
    assert (expect != boxes).any()
    n = len(sizes)
    post = yf.YOLO_post_process(0.3, 0.3, 3, 1, yf.io_params_for(256)["anchors"], [net[0], net[1], 1])
    hw = torch.tensor(sizes, dtype=torch.int32, device=dev)
    # the separate tensors
    raw = dict(boxes=torch.from_numpy(boxes).to(dev), counts=torch.from_numpy(counts).to(dev))
    post.scale_boxes(raw, hw)
    torch.cuda.synchronize(dev)
    assert np.array_equal(raw["boxes"].cpu().numpy(), expect) and np.array_equal(raw["counts"].cpu().numpy(), counts)
    # the packed record block: count | boxes | scores | cls | src, everything but the counted boxes bit-unchanged
    rec0 = np.random.default_rng(5).integers(-2 ** 31, 2 ** 31 - 1, (n, 1 + 8 * K), dtype=np.int64).astype(np.int32)
    rec0[:, 0] = counts
    rec0[:, 1:1 + 4 * K] = boxes.reshape(n, -1)
    want_rec = rec0.copy()
    want_rec[:, 1:1 + 4 * K] = expect.reshape(n, -1)
    views = post.record_views(torch.from_numpy(rec0.copy()).to(dev), K)
    post.scale_boxes(views, hw)
    torch.cuda.synchronize(dev)
    assert np.array_equal(views["records"].cpu().numpy(), want_rec)
