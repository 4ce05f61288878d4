#!/usr/bin/env python3
"""Generate tests/golden/voc/ (the VOC fixture data) and tests/golden/golden_dataset.npz by RUNNING THE REFERENCE'S OWN DetectDataset
and Validation (src/model_training/dataloader/detect_dataset.py, validate.py).  Runs only where the reference checkout exists; the GPU
box never executes this script -- it consumes what it wrote.  Nothing of the reference's source text is stored.

cv2 and tensorboardX are absent, so both are stub modules: cv2.imread decodes with PIL (RGB reversed to BGR, as dataset.py does),
cvtColor / resize are oracle/cv_oracle.py's restatement of OpenCV's 8-bit arithmetic and GaussianBlur is tests/aug_ref.py's.  What this
pins is therefore the reference's CONTROL FLOW, random-draw order, label arithmetic and mAP bookkeeping, composed with those
restatements; OpenCV's own blur / resize pixels stay unpinned (no cv2 where this runs).

Recorded, for the 1-channel (256x320x1 from 512x640x3) configuration at several random.seed values and for the 3-channel one at one seed,
over fixed sequences of frame names: the blur kernel size and flip decision of every access, the item (boxes in full; the image as
the SHA-256 of its bytes u8 = img + 128, which keeps the file small and the comparison bit for bit), and what the reference raised for an image without objects (1: IndexError, when it draws a flip, :143; 2: ValueError at the box copy, :159).  And the reference's mAP of the shipped
256x320 checkpoint on the val tree (Validation over DetectDataset(val=True, augment=False), batch 4, torch.manual_seed(0))."""
import hashlib
import logging
import os
import random
import sys
import tempfile
import types
import xml.etree.ElementTree as ET

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]

import aug_ref  # noqa: E402
import voc_tree  # noqa: E402
from oracle import cv_oracle as cv  # noqa: E402

CLASSES = ["carrier", "defender", "destroyer"]
SEEDS = (0, 1, 2)
SEQ_LEN = 8


def write_xml(path, w, h, boxes):
    """boxes: [(cls_name, xmin, ymin, xmax, ymax)] -> a Pascal-VOC annotation."""
    ann = ET.Element("annotation")
    ET.SubElement(ann, "filename").text = os.path.splitext(os.path.basename(path))[0] + ".jpg"
    size = ET.SubElement(ann, "size")
    for tag, v in (("width", w), ("height", h), ("depth", 3)):
        ET.SubElement(size, tag).text = str(v)
    for name, x1, y1, x2, y2 in boxes:
        obj = ET.SubElement(ann, "object")
        ET.SubElement(obj, "name").text = name
        ET.SubElement(obj, "difficult").text = "0"
        bb = ET.SubElement(obj, "bndbox")
        for tag, v in (("xmin", x1), ("ymin", y1), ("xmax", x2), ("ymax", y2)):
            ET.SubElement(bb, tag).text = "%g" % v
    ET.indent(ann)
    ET.ElementTree(ann).write(path, encoding="utf-8", xml_declaration=True)


def synthetic_jpeg(path, h, w, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(xx / (17 + 5 * c) + yy / (23 + 3 * c) + c) for c in range(3)], -1)
    for _ in range(40):
        y0, x0 = rng.integers(0, h - 8), rng.integers(0, w - 8)
        img[y0:y0 + rng.integers(4, 60), x0:x0 + rng.integers(4, 60)] = rng.integers(0, 256, 3)
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(path, quality=90)


def make_fixtures():
    """tests/golden/voc/{xml,img}: XMLs of the 20 bundled frames (boxes: golden_map_256.npz's synthetic targets, in 640x512 pixels)
    and three synthetic colour frames with their XMLs."""
    os.makedirs(os.path.join(voc_tree.VOC, "xml"), exist_ok=True)
    os.makedirs(os.path.join(voc_tree.VOC, "img"), exist_ok=True)
    targets = np.load(os.path.join(HERE, "golden_map_256.npz"))["targets"]          # [20, 64, 6] normalised (xc, yc, w, h, cls, 255)
    for f, stem in enumerate(voc_tree.bundled_stems()):
        boxes = []
        for t in targets[f][targets[f][:, 5] > 1].astype(np.float64):
            xc, yc, bw, bh = t[0] * 640, t[1] * 512, t[2] * 640, t[3] * 512
            boxes.append((CLASSES[int(t[4])], round(xc - bw / 2, 2), round(yc - bh / 2, 2), round(xc + bw / 2, 2), round(yc + bh / 2, 2)))
        if not boxes:      # the reference cannot load a frame without objects (see main): every val frame gets one
            boxes.append((CLASSES[f % 3], 100.0 + 4 * f, 300.0, 140.0 + 4 * f, 322.5))
        write_xml(os.path.join(voc_tree.VOC, "xml", stem + ".xml"), 640, 512, boxes)
    rng = np.random.default_rng(11)
    for seed, (stem, (h, w), n) in enumerate((("syn_linear", (600, 800), 3), ("syn_empty", (512, 640), 0), ("syn_crowd", (512, 640), 70))):
        synthetic_jpeg(os.path.join(voc_tree.VOC, "img", stem + ".jpg"), h, w, seed)
        boxes = []
        for i in range(n):
            x1, y1 = rng.integers(0, w - 40), rng.integers(0, h - 40)
            boxes.append((CLASSES[i % 3], int(x1), int(y1), int(x1 + rng.integers(8, 40)), int(y1 + rng.integers(8, 40))))
        write_xml(os.path.join(voc_tree.VOC, "xml", stem + ".xml"), w, h, boxes)


def stub_modules(blur_log):
    from PIL import Image
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2GRAY = 6

    def imread(path):
        with Image.open(path) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])

    def cvtColor(img, code):
        assert code == cv2.COLOR_BGR2GRAY
        return cv.cvt_bgr2gray(img, 15)

    def GaussianBlur(img, ksize, sigma):
        assert ksize[0] == ksize[1] and sigma == 0
        blur_log.append(ksize[0])
        return aug_ref.gaussian_blur_u8(img, ksize[0])
    cv2.imread, cv2.cvtColor, cv2.resize, cv2.GaussianBlur = imread, cvtColor, cv.resize_linear_u8, GaussianBlur
    sys.modules["cv2"] = cv2
    tb = types.ModuleType("tensorboardX")
    tb.SummaryWriter = object
    sys.modules["tensorboardX"] = tb


class _NpProxy(types.ModuleType):
    """The reference module's `np`, with fliplr recorded."""
    def __init__(self, log):
        super().__init__("numpy_proxy")
        self._log = log

    def __getattr__(self, name):
        return getattr(np, name)

    def fliplr(self, a):
        self._log.append(True)
        return np.fliplr(a)


def main():
    make_fixtures()
    blur_log, flip_log = [], []
    stub_modules(blur_log)
    sys.path[:0] = [os.path.join(REF, "src", "model_training"), os.path.join(REF, "src")]
    import dataloader.detect_dataset as ref_ds                       # the reference
    from validate import Validation                                  # the reference
    from loss.yolo_loss import YOLOLossV3                            # the reference
    from model_training.model.yolo_fastest import YoloFastest        # the reference
    from model_training._config import config_params
    ref_ds.np = _NpProxy(flip_log)
    logger = logging.getLogger("ref-dataset")
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        trees = voc_tree.make_trees(tmp)
        ap = voc_tree.aug_params(trees)
        stems_all = voc_tree.bundled_stems() + list(voc_tree.SYNTHETIC)
        for cfg, in_shape, seeds in (("c1", [256, 320, 1], SEEDS), ("c3", [256, 320, 3], SEEDS[:1])):
            ds = ref_ds.DetectDataset(in_shape, [512, 640, 3], logger, augment=True, aug_params=ap, max_boxes=64)
            names = [os.path.splitext(os.path.basename(p))[0] for p in ds.img_list]
            for seed in seeds:
                rng = np.random.default_rng(100 + seed)
                seq = list(voc_tree.SYNTHETIC) + list(rng.choice(stems_all, SEQ_LEN - len(voc_tree.SYNTHETIC)))
                seq = [seq[i] for i in rng.permutation(len(seq))] + ["syn_empty", "syn_crowd"]
                random.seed(seed)
                ks, flips, raised, imgs, boxes = [], [], [], [], []
                for stem in seq:
                    del blur_log[:], flip_log[:]
                    try:
                        img, box = ds[names.index(stem)]
                        raised.append(0)
                        u8 = (img + 128.0).astype(np.uint8)
                        assert np.array_equal(u8.astype(np.float64) - 128.0, img) and img.dtype == np.float64
                        imgs.append(hashlib.sha256(np.ascontiguousarray(u8).tobytes()).hexdigest())
                        boxes.append(box)
                    except (IndexError, ValueError) as e:      # no objects: IndexError at the flip (:143), else ValueError at :159
                        raised.append(1 if isinstance(e, IndexError) else 2)
                        imgs.append("")
                        boxes.append(np.zeros((64, 6)))
                    ks.append(blur_log[0] if blur_log else 0)
                    flips.append(bool(flip_log))
                key = "%s_s%d" % (cfg, seed)
                out[key + "_names"] = np.array(seq)
                out[key + "_k"] = np.array(ks, np.int32)
                out[key + "_flip"] = np.array(flips)
                out[key + "_raised"] = np.array(raised, np.int32)
                out[key + "_img_sha256"] = np.array(imgs)
                out[key + "_boxes"] = np.stack(boxes)
                print(key, "k", ks, "flip", [int(f) for f in flips], "raised", [int(r) for r in raised])
        # the reference's mAP of the shipped 256x320 checkpoint over the val tree
        io = dict(config_params["io_params"])
        model = YoloFastest(io).eval()
        model.load_state_dict(torch.load(os.path.join(REF, "models/pytorch/256x320/YOLO-Fastest_epoch_28.pth"), map_location="cpu"))
        dev = torch.device("cpu")
        losses = [YOLOLossV3(io["anchors"][i], io["num_cls"], io["input_shape"], dev) for i in range(2)]
        val_ds = ref_ds.DetectDataset([256, 320, 1], [512, 640, 3], logger, augment=False, aug_params=ap, max_boxes=64, val=True)
        params = {"train_params": {"batch_size": 4, "IOU_val_thre": 0.5}, "io_params": dict(io, class_names=CLASSES)}
        torch.manual_seed(0)
        val = Validation(params, logger, val_ds, dev, losses)
        out["mAP"] = np.float64(val.get_mAP(model, 0))
        out["AP"] = np.array([float(val._Validation__calculate_AP(cls=c)) for c in range(3)], np.float64)
        out["target_num"] = val.target_num.numpy().astype(np.float32)
        out["match_tp"] = np.array([sum(m[1] == "TP" for m in val.match_list[c]) for c in range(3)], np.int32)
        out["match_n"] = np.array([len(val.match_list[c]) for c in range(3)], np.int32)
        print("mAP", float(out["mAP"]), "AP", out["AP"].tolist(), "targets", out["target_num"].tolist(), "TP", out["match_tp"].tolist(),
              "matches", out["match_n"].tolist())
    np.savez_compressed(os.path.join(HERE, "golden_dataset.npz"), **out)


if __name__ == "__main__":
    main()
