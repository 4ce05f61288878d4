"""DetectDataset(letterbox=True) without a GPU (dataset.py): the labels against a line-by-line transcription of yolov5
(tests/letterbox_labels_ref.py) bit for bit in float64, the unchanged order of the `random` draws, the frame-size table, the refusal of
a frame that decodes to another size, neutrality for anchors.label_wh, the untouched default, and the reach of the sizes the GPU test
holds the kernel to.  Every comparison is an equality: both sides are IEEE double (labels) or integer arithmetic (pixels)."""
import logging
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import letterbox_labels_ref as lab  # noqa: E402
import letterbox_ref  # noqa: E402
import voc_mixed  # noqa: E402
import voc_tree  # noqa: E402
from yolo_fastest_amd import anchors  # noqa: E402
from yolo_fastest_amd.dataset import DetectDataset  # noqa: E402

LOG = logging.getLogger("test-dataset-letterbox")
H, W = 256, 320
ACTIVE = dict(degrees=10.0, translate=0.1, scale=1.3, shear=2.0, perspective=0.0005, flipud=0.5)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return voc_mixed.write_tree(tmp_path_factory.mktemp("mixed"), voc_mixed.LABEL_FRAMES)


def _ds(tree, letterbox=True, keys=None, **kw):
    kw.setdefault("max_boxes", 64)
    extra = dict(letterbox=True) if letterbox else {}
    return DetectDataset([H, W, 1], None if letterbox else [512, 640, 3], LOG, aug_params=voc_mixed.aug_params(tree, **(keys or {})),
                         device="cpu", **extra, **kw)


def _frame(ds, i):
    stem = os.path.splitext(os.path.basename(ds.img_list[i]))[0]
    return next(f for f in voc_mixed.LABEL_FRAMES if f.stem == stem)


def test_labels_are_yolov5s_bit_for_bit(tree):
    ds = _ds(tree, augment=False)
    assert len(ds) == len(voc_mixed.LABEL_FRAMES)
    seen = set()
    for i in range(len(ds)):
        f = _frame(ds, i)
        seen.add(f.stem)
        rows = lab.letterboxed_rows(f.boxes, f.hw[0], f.hw[1], H, W)
        k, flip, boxes = ds.draw(i)
        assert (k, flip) == (0, False)
        want = lab.targets(rows, False, False, 64)
        assert boxes.dtype == np.float64 and boxes.tobytes() == want.tobytes(), (f.stem, boxes[:3], want[:3])
        got = np.asarray(ds._labels(i), np.float64).reshape(-1, 5)
        assert got.tobytes() == rows.tobytes(), f.stem
    assert len(seen) == len(voc_mixed.LABEL_FRAMES)


def test_the_label_frames_are_the_cases_they_claim(tree):
    """no border; top 8 / bottom 8; tall; 51 x 77; odd total padding; 9x1 and 1x9; a clipped box; no objects."""
    geo = {f.stem: letterbox_ref.geometry(f.hw[0], f.hw[1], H, W) for f in voc_mixed.LABEL_FRAMES}
    assert geo["a_512x640"] == (256, 320, 0, 0, 0, 0)
    assert geo["b_600x800"][:4] == (240, 320, 8, 8)
    assert geo["c_640x512"][1] < W and geo["c_640x512"][0] == H
    assert geo["d_51x77"][:4] == (212, 320, 22, 22)
    odd = geo["i_253x317"]
    assert (H - odd[0]) % 2 == 1 and odd[2:4] == (0, 1)                    # odd total padding: the float pad 0.5 is not the integer top
    assert geo["e_9x1"][:2] == (256, 28) and geo["f_1x9"][:2] == (36, 320)
    past = lab.letterboxed_rows(next(f for f in voc_mixed.LABEL_FRAMES if f.stem == "g_past").boxes, 480, 640, H, W)
    unclipped = lab.label_file_rows([(2, -30, -12, 700, 500)], 480, 640)[0]
    assert unclipped[3] > 1.0                                              # wider than the frame before the clip
    x1, x2 = (past[0, 1] - past[0, 3] / 2) * W, (past[0, 1] + past[0, 3] / 2) * W
    assert abs(x1) < 1e-9 and abs(x2 - (W - 1e-3)) < 1e-9                  # clipped to [0, W - eps]
    assert not next(f for f in voc_mixed.LABEL_FRAMES if f.stem == "h_empty").boxes


@pytest.mark.parametrize("case", ["plain", "geometric", "mixup", "mosaic"])
def test_the_draws_are_those_of_the_same_dataset_without_letterbox(tree, case):
    keys = dict(plain={}, geometric=ACTIVE, mixup=dict(ACTIVE, mixup=0.6), mosaic=dict(mosaic=0.6, flipud=0.3))[case]
    kw = dict(mixup=True) if case == "mixup" else dict(mosaic=True) if case == "mosaic" else {}
    a, b = _ds(tree, True, keys, **kw), _ds(tree, False, keys, **kw)
    assert [os.path.basename(p) for p in a.img_list] == [os.path.basename(p) for p in b.img_list]
    order = [i % len(a) for i in range(3 * len(a))]
    random.seed(5)
    got = [a.draw_mosaic(i) for i in order]
    state = random.getstate()
    random.seed(5)
    want = [b.draw_mosaic(i) for i in order]
    assert random.getstate() == state                                      # the same number of draws
    hits = dict(k=0, flip=0, ud=0, warp=0, partner=0, mosaic=0)
    for g, w in zip(got, want):
        assert (g[0], g[1], g[3]) == (w[0], w[1], w[3])
        for j in (4, 6):
            assert (g[j] is None) == (w[j] is None) and (g[j] is None or np.array_equal(g[j], w[j]))
        assert g[5] == w[5] and g[7] == w[7]
        assert (g[8] is None) == (w[8] is None)
        if g[8] is not None:
            assert g[8][:3] == w[8][:3] and np.array_equal(g[8][3], w[8][3])
        hits["k"] += g[0] != 0; hits["flip"] += g[1]; hits["ud"] += g[3]; hits["warp"] += g[4] is not None
        hits["partner"] += g[5] is not None; hits["mosaic"] += g[8] is not None
    assert hits["k"] and hits["flip"]
    assert case != "geometric" or (hits["warp"] and hits["ud"])
    assert case != "mixup" or hits["partner"]
    assert case != "mosaic" or hits["mosaic"]


def test_what_follows_labels_takes_the_letterboxed_rows(tree):
    """fliplr / flipud and the max_boxes fill on rows' (no warp: the flips of the transcription's rows are the whole of it)."""
    ds = _ds(tree, True, dict(flipud=0.5), max_boxes=1)
    random.seed(2)
    seen = set()
    for i in [j % len(ds) for j in range(4 * len(ds))]:
        f = _frame(ds, i)
        k, flip, boxes, ud, coeffs = ds.draw_ex(i)
        assert coeffs is None
        want = lab.targets(lab.letterboxed_rows(f.boxes, f.hw[0], f.hw[1], H, W), flip, ud, 1)
        assert boxes.tobytes() == want.tobytes(), f.stem
        seen.add((flip, ud))
    assert len(seen) == 4


def test_frame_sizes_come_from_the_xml_or_the_image_header(tree, tmp_path):
    ds = _ds(tree, augment=False)
    for i in range(len(ds)):
        assert ds._frame_hw[ds.img_list[i]] == _frame(ds, i).hw            # "missing" and "zero" fell back to the header
    # <size> is honoured where it is valid: an XML that lies is believed (and refused at decode time, below)
    lying = voc_mixed.Frame("liar", (40, 60), [(0, 1, 2, 30, 20)])
    d = voc_mixed.write_tree(tmp_path, [lying])
    path = os.path.join(d, "xml", "liar.xml")
    with open(path) as fh:
        text = fh.read()
    with open(path, "w") as fh:
        fh.write(text.replace("<width>60</width>", "<width>120</width>"))
    liar = DetectDataset([H, W, 1], None, LOG, aug_params=voc_mixed.aug_params(d), device="cpu", letterbox=True, augment=False)
    assert liar._frame_hw[liar.img_list[0]] == (40, 120)
    with pytest.raises(ValueError, match="liar.jpg"):
        liar._decode(0)
    # without the argument nothing is recorded and nothing is read
    assert _ds(tree, False)._frame_hw == {}


def test_a_frame_that_decodes_to_another_size_is_refused(tree, monkeypatch):
    ds = _ds(tree, augment=False)
    i = next(j for j in range(len(ds)) if _frame(ds, j).stem == "d_51x77")
    assert ds._decode(i).shape == (51, 77, 3)
    monkeypatch.setitem(ds._frame_hw, ds.img_list[i], (77, 51))
    with pytest.raises(ValueError, match="d_51x77.jpg"):
        ds._decode(i)
    with pytest.raises(ValueError, match="d_51x77.jpg"):                   # the device decode's check is the same method
        ds._check_size(i, (51, 77))


def test_label_wh_is_the_letterboxed_rows_in_net_pixels(tree):
    ds = _ds(tree, augment=False)
    rows = [lab.letterboxed_rows(_frame(ds, i).boxes, *_frame(ds, i).hw, H, W) for i in range(len(ds))]
    want = np.concatenate([r[:, 3:5] for r in rows]) * np.array([W, H], np.float64)
    got = anchors.label_wh(ds)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("key", ["c1_s0", "c3_s0"])
def test_the_default_is_unchanged(tmp_path, golden, key):
    """Without the argument: the draws and boxes of the parent commit on the fixture tree (tests/golden/golden_dataset.npz)."""
    trees = voc_tree.make_trees(tmp_path)
    g = golden("golden_dataset")
    ds = DetectDataset([256, 320, 1 if key.startswith("c1") else 3], [512, 640, 3], LOG, aug_params=voc_tree.aug_params(trees), max_boxes=64,
                       device="cpu")
    assert ds.letterbox is False and ds._frame_hw == {} and ds.origin_img_shape == [512, 640, 3]
    names = [os.path.splitext(os.path.basename(p))[0] for p in ds.img_list]
    random.seed(int(key[-1]))
    for j, stem in enumerate(g[key + "_names"]):
        k, flip, boxes = ds.draw(names.index(str(stem)))
        assert (k, flip) == (int(g[key + "_k"][j]), bool(g[key + "_flip"][j])), (key, j, stem)
        if not g[key + "_raised"][j]:
            assert np.array_equal(boxes, g[key + "_boxes"][j]), (key, j, stem)


def test_the_kernel_tests_sizes_reach_every_branch():
    """The CPU statement itself -- letterbox_ref.letterbox_u8, blur, flips -- runs on every size of the GPU kernel test, and at 64 x 80
    the set reaches: copy, 2x2 mean, linear with a border above and below, left and right, and none."""
    def mode(h, w, g):
        return "copy" if (h, w) == g[:2] else "mean" if (h, w) == (2 * g[0], 2 * g[1]) else "linear"
    geo = {s: letterbox_ref.geometry(s[0], s[1], 64, 80) for s in voc_mixed.KERNEL_SIZES}
    for s in [(64, 80), (48, 80), (63, 80), (64, 79)]:
        assert mode(*s, geo[s]) == "copy"
    assert geo[(48, 80)][2:4] == (8, 8)
    assert geo[(63, 80)][2:] == (0, 1, 0, 0)                               # a bottom-only 1-row border
    assert geo[(64, 79)][2:] == (0, 0, 0, 1)                               # a right-only 1-column border
    assert mode(128, 160, geo[(128, 160)]) == "mean" and geo[(128, 160)][2:] == (0, 0, 0, 0)
    for s, tb in {(51, 77): (5, 6), (600, 800): (2, 2), (37, 120): (19, 20), (1, 9): (27, 28)}.items():
        assert mode(*s, geo[s]) == "linear" and geo[s][2:4] == tb and geo[s][4:] == (0, 0), (s, geo[s])
    for s, lr in {(80, 48): (21, None), (77, 51): (19, None), (100, 33): (29, 30), (9, 1): (36, 37), (3, 3): (8, 8)}.items():
        assert mode(*s, geo[s]) == "linear" and geo[s][4] == lr[0] and (lr[1] is None or geo[s][5] == lr[1]) and geo[s][2:4] == (0, 0), (s, geo[s])
    assert mode(512, 640, geo[(512, 640)]) == "linear" and geo[(512, 640)][2:] == (0, 0, 0, 0)
    assert {geo[s][4] % 4 for s in [(80, 48), (77, 51), (100, 33), (9, 1), (3, 3)]} >= {0, 1, 3}
    # the statement runs on every size, at both destinations, gray and colour, with a blur that reaches the border
    for Hn, Wn in voc_mixed.KERNEL_NETS:
        for h, w in voc_mixed.KERNEL_SIZES:
            bgr = voc_mixed.pixels(h, w)
            g = letterbox_ref.geometry(h, w, Hn, Wn)
            for bits in (15, 0):
                plain = voc_mixed.statement_u8(bgr, Hn, Wn, bits, 0, False)
                out = voc_mixed.statement_u8(bgr, Hn, Wn, bits, 7, True, True)
                assert out.shape == (Hn, Wn, 1 if bits else 3) and out.dtype == np.uint8
                assert np.array_equal(voc_mixed.statement_u8(bgr, Hn, Wn, bits, 0, True, True), plain[::-1, ::-1])
                mask = np.ones((Hn, Wn), bool)
                mask[g[2]:g[2] + g[0], g[4]:g[4] + g[1]] = False
                assert (plain[mask] == 114).all()
