"""tests/draw_ref.py and plot.label_mask against plot.plot_one_box itself, and the text blend against the installed Pillow over all
256 x 256 pairs of destination and mask.  No GPU needed.  These tests read the installed Pillow's behaviour: if a later Pillow blends
or rasterises differently, they say so here, before the device kernel is blamed."""
import os
import sys

import numpy as np
import pytest
from PIL import Image, ImageDraw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import draw_ref  # noqa: E402
from yolo_fastest_amd import plot  # noqa: E402

COLORS = [[106, 90, 205], [199, 97, 20], [112, 128, 105]]
H, W = 120, 160
# (name, [(xyxy, label, colour index)]) drawn in order
CASES = [
    ("inside", [([30, 40, 100, 90], "cloud 0.87", 0)]),
    ("inside, float corners as the post-process returns them", [([30.7, 40.2, 100.9, 90.5], "cloud 0.87", 1)]),
    ("label cut by the top edge", [([20, 5, 90, 60], "nocloud 1.00", 2)]),
    ("label cut by the left and top edges", [([-12, 9, 50, 60], "cloud 0.05", 0)]),
    ("label cut by the right edge", [([140, 50, 158, 100], "nocloud 0.33", 1)]),
    ("partly outside", [([-20, 30, 80, 150], "cloud 0.50", 2), ([90, -10, 200, 70], "nocloud 0.51", 0)]),
    ("wholly outside: larger than the image on every side", [([-20, -10, 200, 150], "cloud 0.50", 2)]),
    ("wholly outside", [([300, 300, 400, 380], "cloud 0.99", 0), ([-90, -80, -30, -20], "cloud 0.98", 1), ([10, -300, 60, -200], "x", 2)]),
    ("label wholly outside, box inside", [([10, 1, 60, 50], "cloud 0.12", 0)]),
    ("zero area", [([50, 60, 50, 60], "cloud 0.01", 1), ([70, 20, 70, 80], "cloud 0.02", 2), ([20, 100, 90, 100], None, 0)]),
    ("swapped corners", [([100, 90, 30, 40], "cloud 0.77", 0), ([120, 30, 60, 70], None, 1)]),
    ("overlapping boxes in order", [([30, 40, 100, 90], "cloud 0.87", 0), ([60, 50, 130, 110], "nocloud 0.66", 1), ([35, 45, 95, 60], "cloud 0.10", 2),
                                    ([30, 40, 100, 90], "cloud 0.88", 1)]),
    ("no label", [([30, 40, 100, 90], None, 0), ([5, 5, 155, 115], "", 2)]),
    ("at the corners", [([0, 0, W - 1, H - 1], "cloud 0.40", 0), ([W - 1, H - 1, W + 5, H + 5], "c", 1), ([0, H - 1, 10, H - 1], "0.00", 2)]),
]
THICKNESS = [None, 1, 2, 3, 4, 5, 6]


def background(seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("ink", [255, 225, 0])
def test_the_text_blend_is_pillows_for_every_destination_and_mask(ink):
    dst = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, 1)
    mask = np.repeat(np.arange(256, dtype=np.uint8)[None, :], 256, 0)
    im = Image.fromarray(np.stack([dst, dst, dst], axis=2).copy())
    ImageDraw.Draw(im).bitmap((0, 0), Image.fromarray(mask), fill=(ink, ink, ink))      # ImageDraw.text's own path: draw_bitmap
    got = np.asarray(im)
    want = draw_ref.blend(dst, ink, mask)
    assert np.array_equal(got[..., 0], want) and np.array_equal(got[..., 1], want) and np.array_equal(got[..., 2], want), \
        "the installed Pillow blends text differently: %d of 65536 pairs differ" % int((got[..., 0] != want).sum())


@pytest.mark.parametrize("tl", THICKNESS)
@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_draw_ref_equals_plot_one_box(case, tl):
    want, got = background(case), background(case)
    for xyxy, label, ci in CASES[case][1]:
        plot.plot_one_box(xyxy, want, color=COLORS[ci], label=label, line_thickness=tl)
        t = tl or plot.default_thickness(H, W)
        draw_ref.plot_one_box(xyxy, got, COLORS[ci], plot.label_mask(label, t) if label else None, line_thickness=tl)
    assert np.array_equal(want, got), (CASES[case][0], tl, int((want != got).any(axis=2).sum()))
    if not CASES[case][0].startswith("wholly outside"):
        assert not np.array_equal(want, background(case))


@pytest.mark.parametrize("tl", [1, 2, 3, 4, 5, 6])
def test_every_label_the_driver_can_format(tl):
    """'%s %.2f' of both class names at a few scores, on a flat and on a noisy background, at the frame size the driver sees."""
    for name in ("cloud", "nocloud"):
        for score in (0.0, 0.07, 0.5, 0.89, 1.0):
            label = "%s %.2f" % (name, score)
            for bg in (np.full((512, 640, 3), 200, np.uint8), np.random.default_rng(tl).integers(0, 256, (512, 640, 3), dtype=np.uint8)):
                want, got = bg.copy(), bg.copy()
                plot.plot_one_box([100.5, 200.25, 300, 400], want, color=COLORS[0], label=label, line_thickness=tl)
                draw_ref.plot_one_box([100.5, 200.25, 300, 400], got, COLORS[0], plot.label_mask(label, tl), line_thickness=tl)
                assert np.array_equal(want, got), (label, tl)


def test_box_record_clips_like_the_reference_rectangles():
    for case in range(len(CASES)):
        for tl in (1, 3, 6):
            want, got = background(case), background(case)
            for xyxy, label, ci in CASES[case][1]:
                draw_ref.plot_one_box(xyxy, want, COLORS[ci], None, line_thickness=tl)
                rec = plot.box_record(xyxy, H, W, COLORS[ci], None, tl, "rgb", 0)
                assert len(rec) == 32
                for q in range(5):
                    x0, y0, x1, y1 = rec[4 * q:4 * q + 4]
                    assert (x1 < x0) or (0 <= x0 <= x1 < W and 0 <= y0 <= y1 < H)
                    if x1 >= x0:
                        got[y0:y1 + 1, x0:x1 + 1] = [rec[20] & 255, rec[20] >> 8 & 255, rec[20] >> 16 & 255]
            assert np.array_equal(want, got)
