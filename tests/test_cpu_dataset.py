"""DetectDataset without a GPU (dataset.py): the blur restatement the kernel is held to (tests/aug_ref.py), the XML parsing, label
arithmetic and random-draw order against the reference's own DetectDataset (tests/golden/golden_dataset.npz, make_golden_dataset.py),
and the missing CPU image path."""
import logging
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import aug_ref  # noqa: E402
import voc_tree  # noqa: E402
import yolo_fastest_amd as yf  # noqa: E402
from yolo_fastest_amd.dataset import DetectDataset  # noqa: E402

LOG = logging.getLogger("test-dataset")


@pytest.fixture()
def trees(tmp_path):
    return voc_tree.make_trees(tmp_path)


def _ds(trees, in_shape=(256, 320, 1), **kw):
    return DetectDataset(list(in_shape), [512, 640, 3], LOG, aug_params=voc_tree.aug_params(trees), max_boxes=64, device="cpu", **kw)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_blur_impulse_response_is_the_outer_product_of_the_taps(k):
    t = np.array(aug_ref.TAPS[k], np.int64)
    assert t.sum() == 256 and list(t) == list(t[::-1])
    for v in (8, 100, 255):
        img = np.zeros((21, 23), np.uint8)
        img[10, 11] = v
        out = aug_ref.gaussian_blur_u8(img, k).astype(np.int64)
        r = k // 2
        want = (np.outer(t, t) * v + (1 << 15)) >> 16                  # rounding half up
        assert np.array_equal(out[10 - r:10 + r + 1, 11 - r:11 + r + 1], want)
        out[10 - r:10 + r + 1, 11 - r:11 + r + 1] = 0
        assert not out.any()
    img = np.zeros((9, 9), np.uint8); img[4, 4] = 8                     # 64 * 64 * 8 = 2^15: exactly one half
    assert aug_ref.gaussian_blur_u8(img, 3)[3, 3] == 1


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("shape", [(13, 17), (9, 11, 3), (4, 5), (1, 6)])
def test_blur_reflect101_borders_and_constant(k, shape):
    rng = np.random.default_rng(k * 7 + len(shape))
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    r = k // 2
    t = np.array(aug_ref.TAPS[k], np.int64)
    a = img.astype(np.int64)
    a3 = a if a.ndim == 3 else a[:, :, None]
    pad_y = aug_ref.reflect101(np.arange(-r, shape[0] + r), shape[0])
    pad_x = aug_ref.reflect101(np.arange(-r, shape[1] + r), shape[1])
    if min(shape[:2]) > r:                                              # numpy's 'reflect' is BORDER_REFLECT_101 (edge not repeated)
        assert np.array_equal(np.pad(a3, ((r, r), (r, r), (0, 0)), mode="reflect"), a3[pad_y][:, pad_x])
    padded = a3[pad_y][:, pad_x]
    want = np.zeros_like(a3)
    for y in range(shape[0]):
        for x in range(shape[1]):
            win = padded[y:y + k, x:x + k]                             # all four borders reached by the windows at the edges
            want[y, x] = (np.einsum("i,j,ijc->c", t, t, win) + (1 << 15)) >> 16
    got = aug_ref.gaussian_blur_u8(img, k)
    assert np.array_equal(got.reshape(want.shape), want)
    const = np.full(shape, 173, np.uint8)
    assert np.array_equal(aug_ref.gaussian_blur_u8(const, k), const)
    assert np.array_equal(aug_ref.gaussian_blur_u8(img[:, ::-1], k), got[:, ::-1])   # blur and flip commute


def test_xml_parsing_and_config(trees):
    ds = _ds(trees, augment=False)
    assert len(ds) == 23 and sorted(os.path.basename(p) for p in ds.img_list) == sorted(
        [s + ".jpg" for s in voc_tree.bundled_stems() + list(voc_tree.SYNTHETIC)])
    crowd = ds.img_list.index(os.path.join(trees["train"], "img", "syn_crowd.jpg"))
    assert len(ds.dataset_dict[ds.img_list[crowd]]) == 70
    k, flip, boxes = ds.draw(crowd)
    assert (k, flip) == (0, False) and boxes.shape == (64, 6) and boxes.dtype == np.float64 and (boxes[:, 5] == 255.0).all()
    ap = yf.config_params["augment_params"]
    assert ap["fliplr"] == 0.5 and ap["gussian_filter"] == 0.3 and not os.path.isabs(ap["train_dataset_dir"])
    for bad in (dict(in_shape=(256, 320, 2)), dict(in_shape=(256, 320, 1), cache="host"), dict(gray_bits=16)):
        in_shape = bad.pop("in_shape", (256, 320, 1))
        with pytest.raises(ValueError):
            _ds(trees, in_shape, **bad)
    with pytest.raises(ValueError):
        DetectDataset([256, 320, 1], [512, 640, 1], LOG, aug_params=voc_tree.aug_params(trees), device="cpu")


def test_log_lines(trees):
    lines = []

    class H(logging.Handler):
        def emit(self, rec):
            lines.append(rec.getMessage())
    lg = logging.getLogger("test-dataset-lines"); lg.setLevel(logging.INFO); lg.handlers = [H()]; lg.propagate = False
    DetectDataset([256, 320, 1], [512, 640, 3], lg, aug_params=voc_tree.aug_params(trees), device="cpu")
    DetectDataset([256, 320, 1], [512, 640, 3], lg, aug_params=voc_tree.aug_params(trees), device="cpu", val=True, augment=False)
    assert lines == ["Training Datasest Loading..", "Loading:0/23", "Loading finish！ dataset contain 23 items",
                     " Val Datasest Loading..", "Loading:0/20", "Loading finish！ dataset contain 20 items"]


@pytest.mark.parametrize("key", ["c1_s0", "c1_s1", "c1_s2", "c3_s0"])
def test_labels_and_draws_match_the_reference(trees, golden, key):
    g = golden("golden_dataset")
    ds = _ds(trees, (256, 320, 1 if key.startswith("c1") else 3))
    names = [os.path.splitext(os.path.basename(p))[0] for p in ds.img_list]
    random.seed(int(key[-1]))
    for j, stem in enumerate(g[key + "_names"]):
        k, flip, boxes = ds.draw(names.index(str(stem)))
        assert (k, flip) == (int(g[key + "_k"][j]), bool(g[key + "_flip"][j])), (key, j, stem)
        assert k != 5                                                   # the reference's 5x5 branch is unreachable
        if g[key + "_raised"][j]:                                       # the reference raised: no objects (the documented deviation)
            assert str(stem) == "syn_empty" and not boxes.any()
        else:
            assert np.array_equal(boxes, g[key + "_boxes"][j]), (key, j, stem)
    assert g[key + "_raised"].any() and (g[key + "_k"] == 7).any() and (g[key + "_k"] == 3).any() and g[key + "_flip"].any()
    crowd = [j for j, s in enumerate(g[key + "_names"]) if s == "syn_crowd"]
    assert crowd and (g[key + "_boxes"][crowd[0]][:, 5] == 255.0).all()   # 70 objects truncated to 64


@pytest.mark.parametrize("key", ["c1_s0", "c3_s0"])
def test_restatement_reproduces_the_reference_images(trees, golden, key):
    """The CPU restatement the kernel is held to (PIL decode, tests/aug_ref.py, oracle/cv_oracle.py) gives the images the reference's
    own __getitem__ produced with the same decisions (their SHA-256 in the golden file)."""
    import hashlib
    g = golden("golden_dataset")
    ds = _ds(trees, (256, 320, 1 if key.startswith("c1") else 3))
    names = [os.path.splitext(os.path.basename(p))[0] for p in ds.img_list]
    checked = 0
    for j, stem in enumerate(g[key + "_names"]):
        if g[key + "_raised"][j]:
            continue
        u8 = aug_ref.augment_u8(ds._decode(names.index(str(stem))), ds.input_shape, int(g[key + "_k"][j]), bool(g[key + "_flip"][j]))
        assert hashlib.sha256(u8.tobytes()).hexdigest() == str(g[key + "_img_sha256"][j]), (key, j, stem)
        checked += 1
    assert checked >= 8


def test_no_cpu_image_path(trees):
    ds = _ds(trees)
    random.seed(0)
    state = random.getstate()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ds[0]
    with pytest.raises(RuntimeError, match="no CPU path"):
        ds.__getitems__([0, 1])
    assert random.getstate() == state                                   # nothing drawn before refusing
    k, flip, boxes = ds.draw(0)                                          # labels still work
    assert boxes.shape == (64, 6)


def test_batch_object_and_collate():
    import torch
    from yolo_fastest_amd import validation
    from yolo_fastest_amd.dataset import DetectBatch
    b = DetectBatch(torch.zeros(2, 1, 4, 4), torch.zeros(2, 64, 6, dtype=torch.float64))
    assert b.pin_memory() is b and not isinstance(b, (tuple, list))
    imgs, targets = b
    assert imgs is b.imgs and targets is b.targets
    assert DetectDataset.collate_fn(b) is b and validation.collate_fn(b) is b
    items = [(np.full((4, 5, 1), v - 128.0), np.full((64, 6), v, np.float64)) for v in (0, 255)]
    for fn in (DetectDataset.collate_fn, validation.collate_fn):
        x, t = fn(items)
        assert x.dtype == torch.float64 and x.shape == (2, 1, 4, 5) and t.shape == (2, 64, 6)
        assert x[1, 0, 0, 0].item() == 127.0 / 255.0
