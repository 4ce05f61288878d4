"""The geometric augmentation on the GPU (csrc/yf_aug_kernels.hip: yf_augment_warp_u8; dataset.py with active augment_params keys), bit
for bit against the composition flipud(fliplr(blur_k(Pillow transform(resized)))): `resized` from yf_augment_u8 with neutral parameters,
the transform Pillow's own (tests/warp_ref.py: pil_transform_u8), the blur tests/aug_ref.py's."""
import copy
import ctypes
import logging
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import aug_ref  # noqa: E402, F401
import voc_tree  # noqa: E402
import warp_ref  # noqa: E402

WEIGHTS = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_256x320_epoch28.pth")
LOG = logging.getLogger("test-gpu-dataset-warp")
ACTIVE = dict(degrees=10.0, translate=0.1, scale=1.3, shear=2.0, perspective=0.0005, flipud=0.5)


@pytest.fixture(scope="module")
def yf():
    import yolo_fastest_amd
    return yolo_fastest_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def trees(tmp_path):
    return voc_tree.make_trees(tmp_path)


def _pack(k, fliplr, flipud, coeffs):
    return k | (int(fliplr) << 8) | (int(flipud) << 9) | (0 if coeffs is None else (1 << 10) | (int(coeffs[6] != 0 or coeffs[7] != 0) << 11))


class Call:
    """One set of device buffers for yf_augment_u8 / yf_augment_warp_u8 through the C ABI; outputs pre-filled so that an unwritten byte shows."""
    def __init__(self, dev, src, idx, frames, dh, dw, dc):
        from yolo_fastest_amd import _lib
        self._lib, self.lib, self.dev = _lib, _lib.lib(), dev
        self.S, self.sh, self.sw, self.sc = src.shape
        self.N, self.dh, self.dw, self.dc = len(frames), dh, dw, dc
        self.src = torch.from_numpy(src).to(dev)
        self.idx = torch.tensor(idx, dtype=torch.int32, device=dev)
        self.prm = torch.tensor([_pack(*f) for f in frames], dtype=torch.int32, device=dev)
        ident = [1.0, 0, 0, 0, 1.0, 0, 0, 0]
        self.warp = torch.tensor([ident if f[3] is None else [float(v) for v in f[3]] for f in frames], dtype=torch.float64).to(dev)
        self.scratch = torch.full((self.N, dh, dw, dc), 5, dtype=torch.uint8, device=dev)
        self.u8 = torch.full((self.N, dh, dw, dc), 7, dtype=torch.uint8, device=dev)
        self.x = torch.full((self.N, dc, dh, dw), 9.0, dtype=torch.float32, device=dev)
        self.tab = torch.empty(((dw + dh) * 16,), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self.lib.yf_cv_resize_tables(dev.index, self.sh, self.sw, dh, dw, self.tab.data_ptr(), self.tab.data_ptr() + dw * 16, stream))

    def _head(self, prm):
        return (self.dev.index, self.src.data_ptr(), self.sh, self.sw, self.sc, self.idx.data_ptr(), self.S, self.N, self.tab.data_ptr(),
                self.tab.data_ptr() + self.dw * 16, self.dh, self.dw, self.dc, 15, prm.data_ptr())

    def warp_u8(self):
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        self._lib.check(self.lib.yf_augment_warp_u8(*self._head(self.prm), self.warp.data_ptr(), self.scratch.data_ptr(), self.u8.data_ptr(),
                                                    self.x.data_ptr(), ctypes.c_void_p(stream)))

    def plain_u8(self, params):
        """yf_augment_u8 with (k, fliplr) per frame -> u8 on the host."""
        prm = torch.tensor([k | (int(f) << 8) for k, f in params], dtype=torch.int32, device=self.dev)
        out = torch.empty_like(self.u8)
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        self._lib.check(self.lib.yf_augment_u8(*self._head(prm), out.data_ptr(), None, ctypes.c_void_p(stream)))
        torch.cuda.synchronize()
        return out.cpu().numpy()


def _matrix(h, w, persp, degrees, gain, shear, shift):
    C = np.eye(3); C[0, 2], C[1, 2] = -w / 2, -h / 2
    P = np.eye(3); P[2, 0], P[2, 1] = (0.12 / w, -0.08 / h) if persp else (0.0, 0.0)
    a = math.radians(degrees)
    R = np.eye(3); R[:2, :2] = [[gain * math.cos(a), gain * math.sin(a)], [-gain * math.sin(a), gain * math.cos(a)]]
    S = np.eye(3); S[0, 1], S[1, 0] = math.tan(math.radians(shear[0])), math.tan(math.radians(shear[1]))
    T = np.eye(3); T[0, 2], T[1, 2] = (0.5 + shift[0]) * w, (0.5 + shift[1]) * h
    return T @ S @ R @ P @ C


def _frames(dh, dw):
    """Every blur size x the four flip combinations x (no warp, affine, perspective, all-fill, half-pixel shift): 60 frames."""
    affine = warp_ref.coeffs_of(_matrix(dh, dw, False, 10.0, 1.1, (5.0, -3.0), (0.04, -0.03)))
    affine[6:] = 0.0
    kinds = [None, affine, warp_ref.coeffs_of(_matrix(dh, dw, True, -7.5, 0.8, (0.0, 2.0), (-0.05, 0.02))),
             np.array([1.0, 0, 2.0 * dw, 0, 1.0, -3.0 * dh, 0, 0]), np.array([1.0, 0, 0.5, 0, 1.0, -0.5, 1e-4, 0])]
    return [(k, bool(fl & 1), bool(fl & 2), c) for c in kinds for k in (0, 3, 7) for fl in range(4)]


def _float_of(u8):
    return torch.from_numpy(u8.astype(np.float64) - 128.0).permute(0, 3, 1, 2).div(255.0).float()


@pytest.mark.parametrize("mode", ["same", "half", "linear"])
@pytest.mark.parametrize("dst", [(37, 45, 1), (37, 45, 3), (16, 20, 1)])
def test_warp_kernel_equals_the_pillow_composition(yf, dev, dst, mode):
    dh, dw, dc = dst
    sh, sw = {"same": (dh, dw), "half": (2 * dh, 2 * dw), "linear": (53, 71)}[mode]
    rng = np.random.default_rng(dh * 5 + dc + len(mode))
    src = rng.integers(0, 256, size=(5, sh, sw, 3), dtype=np.uint8)
    src[1] = (np.arange(sw) * 255 // (sw - 1)).astype(np.uint8)[None, :, None]
    frames = _frames(dh, dw)
    idx = [int(i) for i in rng.permutation(len(frames)) % 5]
    idx[7] = -1                                                        # outside the stack: its output frame stays untouched
    call = Call(dev, src, idx, frames, dh, dw, dc)
    resized = call.plain_u8([(0, False)] * len(frames))
    call.warp_u8()
    torch.cuda.synchronize()
    u8, x = call.u8.cpu().numpy(), call.x.cpu()
    want = np.stack([np.full((dh, dw, dc), 7, np.uint8) if idx[n] < 0 else
                     warp_ref.compose_u8(resized[n], c, c is not None and bool(c[6] or c[7]), k, fl, fu, transform=warp_ref.pil_transform_u8)
                     for n, (k, fl, fu, c) in enumerate(frames)])
    bad = [n for n in range(len(frames)) if not np.array_equal(u8[n], want[n])]
    assert not bad, (bad, int((u8 != want).sum()))
    keep = [n for n in range(len(frames)) if idx[n] >= 0]
    assert torch.equal(x[keep], _float_of(want[keep])) and (x[7] == 9.0).all()
    assert np.array_equal(call.scratch.cpu().numpy()[keep], resized[keep])
    # the all-fill frames are 114 everywhere (a blur of a flat image is flat), and the warped ones are mostly image
    for n, (k, fl, fu, c) in enumerate(frames):
        if c is not None and c[2] == 2.0 * dw and idx[n] >= 0:
            assert (u8[n] == warp_ref.FILL).all()
    # frames without bit 10 and bit 9: yf_augment_u8's bytes
    plain = call.plain_u8([(k, fl) for k, fl, _, _ in frames])
    for n, (k, fl, fu, c) in enumerate(frames):
        if c is None and not fu and idx[n] >= 0:
            assert np.array_equal(u8[n], plain[n])
        if c is None and fu and idx[n] >= 0:
            assert np.array_equal(u8[n], plain[n][::-1])


def test_restatement_equals_the_kernel_too(yf, dev):
    """tests/warp_ref.py's numpy transform in place of Pillow's: the same bytes (the CPU suite shows the two equal)."""
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, size=(3, 37, 45, 3), dtype=np.uint8)
    frames = _frames(37, 45)
    idx = [n % 3 for n in range(len(frames))]
    call = Call(dev, src, idx, frames, 37, 45, 3)
    call.warp_u8()
    torch.cuda.synchronize()
    want = np.stack([warp_ref.compose_u8(src[idx[n]], c, c is not None and bool(c[6] or c[7]), k, fl, fu) for n, (k, fl, fu, c) in enumerate(frames)])
    assert np.array_equal(call.u8.cpu().numpy(), want)


def test_replayed_graph_capture_gives_the_same_bytes(yf, dev):
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, size=(4, 53, 71, 3), dtype=np.uint8)
    frames = _frames(37, 45)
    idx = [n % 4 for n in range(len(frames))]
    call = Call(dev, src, idx, frames, 37, 45, 1)
    call.warp_u8()
    torch.cuda.synchronize()
    eager_u8, eager_x = call.u8.clone(), call.x.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.warp_u8()
    for _ in range(2):
        call.u8.fill_(1)
        call.x.fill_(1.0)
        call.scratch.fill_(1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(call.u8, eager_u8) and torch.equal(call.x, eager_x)


def test_arguments_are_checked(yf, dev):
    from yolo_fastest_amd import _lib
    src = np.zeros((1, 8, 8, 3), np.uint8)
    call = Call(dev, src, [0], [(0, False, False, None)], 8, 8, 1)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with pytest.raises(_lib.YFError, match="d_scratch"):
        _lib.check(call.lib.yf_augment_warp_u8(*call._head(call.prm), call.warp.data_ptr(), None, call.u8.data_ptr(), None, stream))
    with pytest.raises(_lib.YFError, match="d_warp"):
        _lib.check(call.lib.yf_augment_warp_u8(*call._head(call.prm), None, call.scratch.data_ptr(), call.u8.data_ptr(), None, stream))


def _ds(trees, channels, dev, keys=ACTIVE, **kw):
    from yolo_fastest_amd.dataset import DetectDataset
    return DetectDataset([256, 320, channels], [512, 640, 3], LOG, aug_params=dict(voc_tree.aug_params(trees), **keys), max_boxes=64,
                         device=dev, **kw)


@pytest.mark.parametrize("cache", [None, "device"])
@pytest.mark.parametrize("channels", [1, 3])
def test_dataset_with_active_keys(yf, trees, dev, cache, channels):
    """A batch from __getitems__ equals item by item (same draws, same bytes), and both equal the Pillow composition of the draws."""
    from yolo_fastest_amd.dataset import DetectBatch, DetectDataset
    ds = _ds(trees, channels, dev, cache=cache)
    assert ds.geometric
    rng = np.random.default_rng(channels)
    warped = flipped = 0
    for rep in range(2):                                               # the cache fills on the first pass, then serves
        idx = [int(i) for i in rng.integers(0, len(ds), size=7)] + [ds.img_list.index(os.path.join(trees["train"], "img", "syn_linear.jpg"))]
        random.seed(rep)
        b = ds.__getitems__(idx)
        state = random.getstate()
        random.seed(rep)
        x, t = DetectDataset.collate_fn([ds[i] for i in idx])
        assert random.getstate() == state
        assert isinstance(b, DetectBatch) and b.imgs.is_cuda and b.imgs.dtype == torch.float32
        assert torch.equal(b.imgs.cpu(), x.float()) and torch.equal(b.targets, t)
        random.seed(rep)
        draws = [ds.draw_ex(i) for i in idx]
        assert torch.equal(torch.from_numpy(np.stack([d[2] for d in draws])), t)
        resized = ds.augment_images(idx, [(0, False)] * len(idx), out_u8=True).cpu().numpy()
        want = np.stack([warp_ref.compose_u8(resized[n], c, True, k, fl, fu, transform=warp_ref.pil_transform_u8)
                         for n, (k, fl, _, fu, c) in enumerate(draws)])
        assert torch.equal(b.imgs.cpu(), _float_of(want))
        warped += sum(int((w != r).any()) for w, r in zip(want, resized))
        flipped += sum(int(d[3]) for d in draws)
    assert warped == 16 and flipped > 0


def test_flipud_alone_and_neutral_keys(yf, trees, dev):
    """flipud without a warp: the plain frame upside down, y = 1 - y; neutral keys: today's bytes (no warp launch is needed for them)."""
    neutral, ud = _ds(trees, 1, dev, keys={}), _ds(trees, 1, dev, keys=dict(flipud=1.0))
    idx = list(range(6))
    random.seed(5)
    a = neutral.__getitems__(idx)
    random.seed(5)
    draws = [ud.draw_ex(i) for i in idx]
    random.seed(5)
    b = ud.__getitems__(idx)
    assert all(d[3] and d[4] is None for d in draws)
    assert not torch.equal(a.imgs, b.imgs)
    # the flipud draw shifts the stream, so compare through the draws: the neutral dataset's launch with ud's (k, flip), rows reversed
    plain = neutral.augment_images(idx, [(d[0], d[1]) for d in draws])
    assert torch.equal(b.imgs, plain.flip(2))


def test_train_runs_with_active_keys(yf, trees, dev, tmp_path, monkeypatch):
    from yolo_fastest_amd import training
    rec = []
    orig = training.train_step

    def step(*a):
        losses = orig(*a)
        rec.append([float(v.detach()) if torch.is_tensor(v) else float(v) for v in losses])
        return losses
    monkeypatch.setattr(training, "train_step", step)
    params = copy.deepcopy(yf.config_params)
    params["io_params"]["save_path"] = str(tmp_path / "active")
    params["augment_params"] = dict(voc_tree.aug_params(trees), **ACTIVE)
    params["train_params"].update(total_epochs=1, batch_size=8, pretrained_pth=WEIGHTS)
    tr = _ds(trees, 1, dev, cache="device")
    va = _ds(trees, 1, dev, val=True, augment=False)
    torch.manual_seed(0)
    random.seed(0)
    training.train(params, dev, None, train_dataset=tr, val_dataset=va, logger=LOG)
    assert len(rec) == 23 // 8 and all(math.isfinite(v) for it in rec for v in it)
