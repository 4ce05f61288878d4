"""TEST INFRASTRUCTURE: Pascal-VOC trees of MIXED frame sizes for DetectDataset(letterbox=True), written at test time (nothing is
committed): seeded-noise-over-ramp frames saved with PIL, and XMLs written here.  `Frame` describes one file; `write_tree` writes
<root>/<split>/{img,xml}; `aug_params` points the reference's augment_params keys at such trees."""
import os

import numpy as np

CLASSES = ("carrier", "defender", "destroyer")


class Frame:
    """stem, (h, w), boxes [(class index, x1, y1, x2, y2)] in frame pixels, and what the XML says about the size: "xml" (the true
    <size>), "missing" (no <size> element) or "zero" (<size> with width 0)."""

    def __init__(self, stem, hw, boxes=(), size="xml"):
        self.stem, self.hw, self.boxes, self.size = stem, tuple(hw), [tuple(b) for b in boxes], size


def pixels(h, w):
    """uint8 [h, w, 3] RGB: seeded noise over a ramp (edges and gradients for the resize and the blur to act on)."""
    rng = np.random.default_rng(1000 * h + w)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.int32)
    ramp = (np.arange(w)[None, :, None] * 3 + np.arange(h)[:, None, None] * 2 + np.arange(3)[None, None, :] * 40) % 256
    return ((noise // 3 + ramp) % 256).astype(np.uint8)


def _xml(f):
    h, w = f.hw
    size = ""
    if f.size != "missing":
        size = "  <size>\n    <width>%d</width>\n    <height>%d</height>\n    <depth>3</depth>\n  </size>\n" % (0 if f.size == "zero" else w, h)
    objs = "".join("  <object>\n    <name>%s</name>\n    <difficult>0</difficult>\n    <bndbox>\n      <xmin>%s</xmin>\n      <ymin>%s</ymin>\n"
                   "      <xmax>%s</xmax>\n      <ymax>%s</ymax>\n    </bndbox>\n  </object>\n" % ((CLASSES[int(c)],) + tuple(b))
                   for c, *b in f.boxes)
    return "<?xml version='1.0' encoding='utf-8'?>\n<annotation>\n  <filename>%s.jpg</filename>\n%s%s</annotation>\n" % (f.stem, size, objs)


def write_tree(root, frames, split="train"):
    """-> the directory <root>/<split> holding img/<stem>.jpg and xml/<stem>.xml for every frame."""
    from PIL import Image
    d = os.path.join(str(root), split)
    os.makedirs(os.path.join(d, "img"), exist_ok=True)
    os.makedirs(os.path.join(d, "xml"), exist_ok=True)
    for f in frames:
        Image.fromarray(pixels(*f.hw), "RGB").save(os.path.join(d, "img", f.stem + ".jpg"), quality=92)
        with open(os.path.join(d, "xml", f.stem + ".xml"), "w") as fh:
            fh.write(_xml(f))
    return d


def aug_params(train_dir, val_dir=None, gussian_filter=0.6, fliplr=0.5, **keys):
    p = {"train_dataset_dir": train_dir, "val_dataset_dir": val_dir or train_dir, "degrees": 0.0, "translate": 0.0, "scale": 1.0,
         "shear": 0.0, "perspective": 0.0, "flipud": 0.0, "fliplr": fliplr, "mixup": 0.0, "gussian_filter": gussian_filter}
    p.update(keys)
    return p


def decode_bgr(path):
    """cv2.imread's frame through PIL, as DetectDataset._decode makes it."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])


# The label test's frames at H x W = 256 x 320: no border; top 8 / bottom 8; tall; 51 x 77 (total padding 44 here; it is odd, 5 / 6, at
# the kernel test's 64 x 80) and 253 x 317, whose total padding IS odd at 256 x 320 (top 0, bottom 1, float pad 0.5); 9x1 and 1x9; one box
# reaching past the frame (clipped); one frame without objects; and the <size> variants.
LABEL_FRAMES = [
    Frame("a_512x640", (512, 640), [(0, 10, 20, 200, 300), (2, 320.5, 100.25, 639, 511)]),
    Frame("b_600x800", (600, 800), [(1, 101, 71, 134, 94), (0, 0, 0, 800, 600)]),
    Frame("c_640x512", (640, 512), [(2, 5, 600, 500, 639)]),
    Frame("d_51x77", (51, 77), [(0, 3, 4, 70, 44), (1, 30, 10, 31, 12)], size="missing"),
    Frame("e_9x1", (9, 1), [(0, 0, 2, 1, 7)]),
    Frame("f_1x9", (1, 9), [(1, 2, 0, 7, 1)], size="zero"),
    Frame("g_past", (480, 640), [(2, -30, -12, 700, 500), (0, 600, 400, 660, 470)]),
    Frame("h_empty", (300, 200), []),
    Frame("i_253x317", (253, 317), [(1, 0, 0, 317, 253), (0, 100, 200, 180, 253)]),
]

# The kernel test's source sizes; at destination 64 x 80 they reach every branch (tests/test_cpu_dataset_letterbox.py asserts which):
# copy (no border, rows above and below, a bottom-only row, a right-only column), the 2x2 mean, linear with rows above and below, linear
# with columns left and right (left mod 4 = 0, 1 and 3: quads straddle the border), linear without a border.
KERNEL_SIZES = [(64, 80), (48, 80), (63, 80), (64, 79), (128, 160), (51, 77), (600, 800), (37, 120), (1, 9), (80, 48), (77, 51), (100, 33),
                (9, 1), (3, 3), (512, 640)]
KERNEL_NETS = [(64, 80), (37, 53)]
KS = (0, 3, 5, 7)


def kernel_params(n_sizes=len(KERNEL_SIZES)):
    """(size index, k, fliplr) per batch member: every size with every k, the flip alternating so that each size meets both values."""
    return [(i, k, bool((i + j) & 1)) for i in range(n_sizes) for j, k in enumerate(KS)]


def statement_u8(bgr, H, W, gray_bits, k, fliplr, flipud=False):
    """The CPU statement of a letterboxed item's pixels (no warp): letterbox, blur, flips -> uint8 [H, W, C]."""
    import aug_ref
    import letterbox_ref
    img = aug_ref.gaussian_blur_u8(letterbox_ref.letterbox_u8(bgr, H, W, gray_bits), k)
    if fliplr:
        img = img[:, ::-1]
    if flipud:
        img = img[::-1]
    if img.ndim == 2:
        img = img[:, :, None]
    return np.ascontiguousarray(img)

# The data-set tests' tree: 8 frames of 5 sizes (two stacks of two frames, so that a cache stack holds more than one slot)
DATASET_FRAMES = [
    Frame("m0_512x640", (512, 640), [(0, 40, 60, 300, 280), (1, 400, 300, 620, 500)]),
    Frame("m1_512x640", (512, 640), [(2, 100, 100, 180, 220)], size="missing"),
    Frame("m2_600x800", (600, 800), [(1, 101, 71, 334, 294), (0, 448, 336, 778, 544)]),
    Frame("m3_600x800", (600, 800), []),
    Frame("m4_640x512", (640, 512), [(2, 50, 300, 400, 630)]),
    Frame("m5_640x512", (640, 512), [(0, 10, 10, 500, 200), (1, 200, 400, 300, 520)], size="zero"),
    Frame("m6_51x77", (51, 77), [(0, 3, 4, 70, 44)]),
    Frame("m7_253x317", (253, 317), [(1, 20, 30, 300, 250), (2, 150, 100, 250, 200)]),
]
