"""The reference's training data: `DetectDataset` of src/model_training/dataloader/detect_dataset.py:42-162 over a Pascal-VOC tree
(`<dir>/xml/*.xml` + `<dir>/img/<stem>.jpg`), with the image work on the GPU (csrc/yf_aug_kernels.hip, `yf_augment_u8`).

Same constructor, log lines, file order (os.listdir of xml/), label arithmetic and random draws (the global `random` module, in the
reference's order: blur?, which blur, flip?) -- so `__getitem__` returns the reference's item exactly: a float64 HWC image `u8 - 128.0`
(channels in cv2.imread's BGR order; gray for a 1-channel net) and float64 (max_boxes, 6) boxes (xc, yc, w, h, cls, 255.0), normalised
by the CONFIGURED origin_img_shape.  The per-frame pixels -- BGR2GRAY, cv2.resize, cv2.GaussianBlur((7, 7) or (3, 3), 0), np.fliplr --
are one kernel launch (OpenCV's 8-bit fixed-point arithmetic restated; parity with a real OpenCV build is unpinned).
Decoding is PIL's (cv2 is not a dependency), or with `decode="device"` the device JPEG decoder's (jpeg.py: the same bytes).  There is no CPU image path: labels work anywhere, images need the GPU.

Additions: `device`, `gray_bits` (OpenCV's 15- or 14-bit BGR2GRAY coefficients, as YoloFastest.gray_bits), `cache="device"` (decoded
frames kept in GPU memory, one uint8 stack per source size, filled on first access), `class_names` (the reference reads
config_params["io_params"]["class_names"]), `decode="device"` (JPEG decoding on the GPU, csrc/yf_jpeg_kernels.hip: one
decode call per source size for a batch's frames, or for the frames a batch adds to the cache; the same bytes as PIL's; `progressive=True` also takes progressive files there, which are
refused otherwise) and `__getitems__`, which DataLoader calls with a whole batch of indices: the same draws in
index order, ONE launch per source size, float32 device images [N, C, H, W] = collate_fn's `(u8 - 128.0) / 255` bit for bit.

Beyond the reference: the geometric keys of `augment_params` -- `degrees`, `translate`, `scale`, `shear`, `perspective`, `flipud` --, which
the reference reads nowhere, are honoured as yolov5's random_perspective (draw_ex, _draw_warp, _warp_labels): the warp runs on the device
between the resize and the blur (`yf_augment_warp_u8`; pixels pinned to Pillow's Image.transform with BILINEAR and fill 114; OpenCV parity
not claimed), the vertical flip after the horizontal one.  At their neutral values (the reference's _config.py: 0, 0, 1.0, 0, 0, 0) or
absent, draws, labels, launch and bytes are the reference's.

`mixup`, the last key, is OPT-IN: the reference ignores it, so a DetectDataset built without `mixup=True` does not read the key at all (a
config copied from yolov5 with `mixup: 0.9` changes nothing).  With `mixup=True` and augment_params["mixup"] = p > 0 it is yolov5's mixup
(draw_mix): with probability p an item is blended with a partner item `j = random.randint(0, len - 1)` (which may be the item itself) under
`r = random.betavariate(32.0, 32.0)` -- yolov5's np.random.beta(32, 32), taken from `random` instead of numpy's generator so that
random.seed alone still reproduces an epoch.  Each of the two frames is grayed, resized and warped on its own (the partner under eight
draws of its own), the bytes are blended as `(im * r + im2 * (1 - r)).astype(np.uint8)` (IEEE double, one rounding per operation), and the
blur and the flips act on the mixture; the partner's label rows (normalised and warped as its own) follow the item's, before the flips and
the max_boxes fill.  On the device a batch with at least one hit is one resize launch per source size into a u8 scratch and ONE
`yf_augment_mix_u8` launch; a batch without a hit goes through the calls above.

`mosaic` is OPT-IN in the same way (the reference has no such key): with `mosaic=True` and augment_params["mosaic"] = p > 0 it is yolov5's
load_mosaic (draw_mosaic), restated for the rectangular net input H x W: with probability p an item becomes four resized frames -- itself
and `random.choices(range(len), k=3)`, shuffled -- around a centre `yc = int(random.uniform(H // 2, 2 * H - H // 2))`, `xc` likewise, on a
2H x 2W canvas of 114s, and that canvas is warped and cropped back to H x W by the same random_perspective (eight draws ALWAYS; with
neutral keys the central crop), then blurred and flipped.  The tiles' label rows go to canvas pixels, are clipped to the canvas, warped,
clipped to the output and filtered (_mosaic_labels over _warp_boxes, the core _warp_labels shares).  On the device a batch with at least
one hit is one resize launch per source size into a u8 scratch and ONE `yf_augment_mosaic_u8` launch, which samples the canvas without
building it: bit for bit Pillow's Image.transform of the materialised canvas.  A miss costs one draw and goes on as above.  Not built:
mosaic together with mixup (both probabilities above 0: ValueError; yolov5 blends two mosaics there), mosaic9, segments, copy-paste.

`letterbox` is OPT-IN as well: with `letterbox=True` the items are yolov5's letterboxed frames instead of the reference's squashed ones, so
that a tree of MIXED frame sizes trains on what `Detect_YOLO(..., letterbox=True)` later feeds the net.  The rule stands in
include/yolo_fastest_hip.h (yf_augment_letterbox_u8) and here.  The frame is uint8 [h, w, 3] BGR, the net input H x W x C:
  Pixels.  x = flipud?(fliplr?(GaussianBlur_k(warp?(letterbox(BGR2GRAY?(frame)))))): `letterbox` exactly yf_cv_letterbox_u8's (geometry in
    double with round-half-even, the 11-bit cv2.resize arithmetic, copy / 2x2 mean / linear decided on (h, w) against (new_h, new_w), a
    border of 114); blur, flips and warp those of the squashed items, on the WHOLE H x W letterboxed image, border included -- the blur
    mixes 114 into the image's edge rows and reflects (101) at the H x W bounds.  CPU statement:
    aug_ref.gaussian_blur_u8(letterbox_ref.letterbox_u8(...)), then the flips (tests/).  With augment=False an item's bytes are
    model.letterbox_u8's for that frame.
  Labels.  yolov5's LoadImagesAndLabels.__getitem__, non-mosaic branch, in float64, in place of the division by origin_img_shape (_labels):
        rows  = xyxy2xywh(xml pixel boxes) / (w, h)                  # the frame's OWN size: a yolov5 label-file row
        r     = min(H / h, W / w)
        new_w, new_h = int(round(w * r)), int(round(h * r))
        dw, dh = (W - new_w) / 2, (H - new_h) / 2                    # yolov5's FLOAT pad, not the integer left / top of the pixels
        xyxy  = xywhn2xyxy(rows, r * w, r * h, padw=dw, padh=dh)
        rows' = xyxy2xywhn(xyxy, w=W, h=H, clip=True, eps=1e-3)
    Everything behind _labels -- the warp, the mixup partner's rows, the mosaic tiles' rows, both flips, the max_boxes fill,
    anchors.label_wh, check_anchors -- takes rows' unchanged, and the order and number of `random` draws do not change.
    `origin_img_shape` is not read (as in Detect_YOLO), _check_size's rule does not apply.
  Frame sizes.  Labels stay host-only, so the constructor records each frame's (h, w): the XML's <size> when both values are positive
    integers, else the image header (PIL's Image.open(path).size, which decodes nothing).  A frame that decodes to another size, on the
    host or on the device, raises ValueError naming the file.
  Mosaic and mixup compose by the same substitution: tiles and partners are LETTERBOXED frames.  For mosaic this deviates from yolov5, whose
    tiles are unpadded load_image frames: a tile that is not of the net's aspect ratio brings its 114 bars into the canvas.
  Launches.  A batch, whatever its frame sizes and however many stacks they sit in, is ONE yf_augment_letterbox_u8 call (two launches:
    the letterbox into a u8 scratch, then blur / flips / warp over it): no per-size loop, no resize-table pool, no index_copy_.  With mixup or mosaic hits the distinct frames
    are letterboxed by ONE yf_cv_letterbox_u8 launch into the u8 scratch, then yf_augment_mix_u8 / yf_augment_mosaic_u8 run unchanged.
  Validation needs no change: its targets are normalised in the net image, now the letterboxed one; get_mAP and get_metrics score in net
    coordinates (scoring in each frame's native coordinates -- yolov5's val applies scale_boxes to predictions and labels -- is not built).
  Not built: auto=True / rectangular batches, scaleFill, scaleup=False, the INTER_AREA choice of yolov5's load_image, HSV.

Deviation: the reference cannot return an image without objects -- `np.array([])` is 1-D, so a flip raises IndexError (`labels[:, 1]`,
:143) and otherwise the box copy raises ValueError (:159); here such an image is blurred / flipped as drawn and gets all-zero boxes (the
draws stay in the reference's order, so the items after it are the reference's)."""
import ctypes
import logging
import math
import os
import random
import xml.etree.ElementTree as xmlET

import numpy as np
import torch

from . import _lib, jpeg
from .config import config_params


def xyxy2xywh(x):
    """utils/general.py:8-15 for numpy [n, 4]."""
    y = np.zeros_like(x)
    y[:, 0] = (x[:, 0] + x[:, 2]) / 2
    y[:, 1] = (x[:, 1] + x[:, 3]) / 2
    y[:, 2] = x[:, 2] - x[:, 0]
    y[:, 3] = x[:, 3] - x[:, 1]
    return y


def mosaic_placement(q, xc, yc, H, W):
    """yolov5's load_mosaic placement of tile q (0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right; every tile H x W) around the
    centre (xc, yc) of the 2H x 2W canvas -> (x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b): canvas[y1a:y2a, x1a:x2a] = tile[y1b:y2b, x1b:x2b]."""
    if q == 0:
        x1a, y1a, x2a, y2a = max(xc - W, 0), max(yc - H, 0), xc, yc
        x1b, y1b, x2b, y2b = W - (x2a - x1a), H - (y2a - y1a), W, H
    elif q == 1:
        x1a, y1a, x2a, y2a = xc, max(yc - H, 0), min(xc + W, W * 2), yc
        x1b, y1b, x2b, y2b = 0, H - (y2a - y1a), min(W, x2a - x1a), H
    elif q == 2:
        x1a, y1a, x2a, y2a = max(xc - W, 0), yc, xc, min(H * 2, yc + H)
        x1b, y1b, x2b, y2b = W - (x2a - x1a), 0, W, min(y2a - y1a, H)
    else:
        x1a, y1a, x2a, y2a = xc, yc, min(xc + W, W * 2), min(H * 2, yc + H)
        x1b, y1b, x2b, y2b = 0, 0, min(W, x2a - x1a), min(y2a - y1a, H)
    return x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b


class DetectBatch:
    """A batch from `DetectDataset.__getitems__`: `imgs` float32 device [N, C, H, W], `targets` float64 host [N, max_boxes, 6].
    Unpacks as `imgs, targets`.  `pin_memory()` is a no-op: the images already live on the GPU (DataLoader(pin_memory=True) calls it;
    this is deliberately not a tuple or Sequence, which torch would take apart first)."""
    __slots__ = ("imgs", "targets")

    def __init__(self, imgs, targets):
        self.imgs, self.targets = imgs, targets

    def __iter__(self):
        return iter((self.imgs, self.targets))

    def pin_memory(self, device=None):
        return self


class DetectDataset(torch.utils.data.Dataset):
    def __init__(self, input_shape, origin_img_shape, logger, augment=True, aug_params=None, max_boxes=64, val=False, device=None,
                 gray_bits=15, cache=None, class_names=None, decode="host", progressive=False, mixup=False, mosaic=False, letterbox=False):
        if aug_params is None:
            aug_params = config_params["augment_params"]
        self.aug_params = aug_params
        self.letterbox = bool(letterbox)                    # yolov5's letterboxed items; `origin_img_shape` is not read in this mode
        self.origin_img_shape = None if self.letterbox else list(origin_img_shape)
        self.input_shape = list(input_shape)
        if len(self.input_shape) != 3 or self.input_shape[2] not in (1, 3):
            raise ValueError("input_shape[2] must be 1 or 3: image files decode to 3 channels (cv2.imread) and a 1-channel net gets them as gray")
        if not self.letterbox and self.input_shape[2] == 1 and self.origin_img_shape[2] == 1:
            raise ValueError("input_shape[2] == origin_img_shape[2] == 1: the reference skips BGR2GRAY then and yields [H, W, 3, 1] images")
        if self.input_shape[0] <= 0 or self.input_shape[1] <= 0 or (not self.letterbox and (self.origin_img_shape[0] <= 0 or self.origin_img_shape[1] <= 0)):
            raise ValueError("image shapes must be positive")
        if gray_bits not in (14, 15):
            raise ValueError("gray_bits must be 14 or 15")
        if cache not in (None, "device"):
            raise ValueError('cache must be None or "device"')
        jpeg.check_decode(decode, progressive)
        self.logger = logger = logger or logging.getLogger(__name__)
        if val:
            logger.info(" Val Datasest Loading..")
            self.dataset_dir = aug_params["val_dataset_dir"]
        else:
            logger.info("Training Datasest Loading..")
            self.dataset_dir = aug_params["train_dataset_dir"]
        self.fliplr = aug_params["fliplr"]
        self.gussian_filter = aug_params["gussian_filter"]
        # yolov5's geometric keys (absent = the reference's _config.py value = neutral); `mixup` is read with mixup=True only (below)
        self.degrees = float(aug_params.get("degrees", 0.0))
        self.translate = float(aug_params.get("translate", 0.0))
        self.scale = float(aug_params.get("scale", 1.0))
        self.shear = float(aug_params.get("shear", 0.0))
        self.perspective = float(aug_params.get("perspective", 0.0))
        self.flipud = aug_params.get("flipud", 0.0)
        if not 0.0 < self.scale < 2.0:
            raise ValueError("augment_params['scale'] must lie inside (0, 2): the gain is drawn from 1 -+ |scale - 1|")
        for key in ("degrees", "shear", "perspective"):
            if not getattr(self, key) >= 0.0:
                raise ValueError("augment_params[%r] must not be negative: it is the far end of a range around 0" % key)
        if not 0.0 <= self.translate < 1.0:
            raise ValueError("augment_params['translate'] must lie inside [0, 1)")
        self.geometric = bool(augment) and (self.degrees != 0.0 or self.translate != 0.0 or self.scale != 1.0 or self.shear != 0.0
                                            or self.perspective != 0.0)
        self.mixup = 0.0                                    # the probability in use: 0.0 unless opted in (the key is not read then)
        if mixup:
            self.mixup = float(aug_params.get("mixup", 0.0))
            if not 0.0 <= self.mixup <= 1.0:
                raise ValueError("augment_params['mixup'] must lie inside [0, 1]: it is a probability")
        self.mosaic = 0.0                                   # likewise: read with mosaic=True only
        if mosaic:
            self.mosaic = float(aug_params.get("mosaic", 0.0))
            if not 0.0 <= self.mosaic <= 1.0:
                raise ValueError("augment_params['mosaic'] must lie inside [0, 1]: it is a probability")
            if self.mosaic > 0 and self.mixup > 0:
                raise ValueError("mosaic=True together with mixup=True, both probabilities above 0: yolov5 blends two mosaics there, "
                                 "which is not built")
        self.max_boxes = max_boxes
        self.augment = augment
        self.gray_bits = gray_bits
        self.cache = cache
        self.decode = decode
        self.progressive = bool(progressive)
        self.classes = list(class_names if class_names is not None else config_params["io_params"]["class_names"])
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = jpeg.cuda_device(device)

        self.file_path_img = os.path.join(self.dataset_dir, "img")
        self.file_path_xml = os.path.join(self.dataset_dir, "xml")
        self.dataset_dict = {}
        self._frame_hw = {}   # letterbox: image path -> the frame's (h, w), from the XML's <size> or the image header
        pathDir = os.listdir(self.file_path_xml)
        for idx in range(len(pathDir)):
            if idx % 1000 == 0:
                logger.info("Loading:%d/%d" % (idx, len(pathDir)))
            filename = pathDir[idx]
            tree = xmlET.parse(os.path.join(self.file_path_xml, filename))
            _labels = []
            for obj in tree.findall("object"):
                _bbox = obj.find("bndbox")
                x1 = float(_bbox.find("xmin").text)
                y1 = float(_bbox.find("ymin").text)
                x2 = float(_bbox.find("xmax").text)
                y2 = float(_bbox.find("ymax").text)
                _labels.append([self.classes.index(obj.find("name").text), x1, y1, x2, y2])
            _image_name = os.path.join(self.file_path_img, os.path.splitext(filename)[0] + ".jpg")
            self.dataset_dict.update({_image_name: _labels})
            if self.letterbox:
                self._frame_hw[_image_name] = self._xml_size(tree) or self._header_size(_image_name)
        self.img_list = list(self.dataset_dict.keys())
        logger.info("Loading finish！ dataset contain %d items" % (self.__len__()))
        self._stacks = {}     # cache="device": (h, w) -> [uint8 tensor [cap, h, w, 3], filled count]
        self._slot = {}       # cache="device": index -> ((h, w), slot in that stack)
        self._tables = {}     # (h, w) -> uint8 device tensor holding cv::resize's int4 tables [dw + dh]
        self._lb_table = None # letterbox: training._PinnedTable of yf_cv_letterbox_u8 / yf_augment_letterbox_u8

    @staticmethod
    def _xml_size(tree):
        """(h, w) of the XML's <size>, or None unless both values are positive integers."""
        try:
            h, w = int(tree.findtext("size/height").strip()), int(tree.findtext("size/width").strip())
        except (AttributeError, ValueError):
            return None
        return (h, w) if h > 0 and w > 0 else None

    @staticmethod
    def _header_size(path):
        """(h, w) from the image header: PIL reads it without decoding a pixel."""
        from PIL import Image
        with Image.open(path) as im:
            w, h = im.size
        return int(h), int(w)

    def __len__(self):
        return len(self.img_list)

    # ---- labels and draws (host; no GPU needed) ----
    def draw(self, index):
        """The host half of __getitem__ (:126-160): the label arithmetic and the random draws of one item, in the reference's order.
        -> (blur kernel size: 0, 3 or 7; flip; float64 boxes [max_boxes, 6]).  draw_ex returns the geometric draws as well."""
        return self.draw_ex(index)[:3]

    def _draw_warp(self, mosaic=False):
        """yolov5's random_perspective matrix for one item, in continuous pixel coordinates of the net-input image (pixel centres at
        half-integers, as Pillow places them and as the normalised labels mean): M = T S R P C in float64, from eight random.uniform draws
        (perspective x, y, angle, gain, shear x, y, translate x, y; all made even where a range is zero).
        -> (M, gain, the eight coefficients of the output -> input map: inv(M) / inv(M)[2, 2]).
        A draw whose denominator a6 x + a7 y + 1 is not positive at all four corners of the output (the image would fold over) is
        REDRAWN, all eight values; after 100 such draws in a row the configured `perspective` is refused with a ValueError.
        `mosaic`: the input is the 2H x 2W mosaic canvas and the output still H x W (yolov5's border = -s // 2): C moves the CANVAS
        centre (W, H) to the origin; T, the fold-over rule and everything else stay those of the output."""
        H, W = self.input_shape[0], self.input_shape[1]
        g = abs(self.scale - 1.0)
        for _ in range(100):
            C = np.eye(3)
            C[0, 2], C[1, 2] = (-W, -H) if mosaic else (-W / 2, -H / 2)
            P = np.eye(3)
            P[2, 0] = random.uniform(-self.perspective, self.perspective)
            P[2, 1] = random.uniform(-self.perspective, self.perspective)
            a = math.radians(random.uniform(-self.degrees, self.degrees))
            gain = random.uniform(1 - g, 1 + g)
            R = np.eye(3)
            R[0, 0], R[0, 1], R[1, 0], R[1, 1] = gain * math.cos(a), gain * math.sin(a), -gain * math.sin(a), gain * math.cos(a)
            S = np.eye(3)
            S[0, 1] = math.tan(math.radians(random.uniform(-self.shear, self.shear)))
            S[1, 0] = math.tan(math.radians(random.uniform(-self.shear, self.shear)))
            T = np.eye(3)
            T[0, 2] = random.uniform(0.5 - self.translate, 0.5 + self.translate) * W
            T[1, 2] = random.uniform(0.5 - self.translate, 0.5 + self.translate) * H
            M = T @ S @ R @ P @ C
            inv = np.linalg.inv(M)
            coeffs = (inv / inv[2, 2]).reshape(9)[:8].copy()
            if self.perspective == 0:
                coeffs[6:] = 0.0                    # an affine frame: exactly, whatever the inverse's rounding left there
            if all(coeffs[6] * x + coeffs[7] * y + 1 > 0 for x in (0, W) for y in (0, H)):
                return M, gain, coeffs
        raise ValueError("augment_params['perspective'] = %r folds the %dx%d image over in 100 draws out of 100" % (self.perspective, W, H))

    def _warp_labels(self, labels, M, gain):
        """yolov5's label half of random_perspective on normalised (cls, xc, yc, w, h) rows: the four corners of each box through M (with
        the perspective divide), min / max as the new box, clipped to the image; box_candidates keeps a box whose width and height are
        both above 2 pixels, whose area is above 0.1 of the old one times gain^2 and whose aspect ratio is below 20.  float64."""
        H, W = self.input_shape[0], self.input_shape[1]
        x1, x2 = (labels[:, 1] - labels[:, 3] / 2) * W, (labels[:, 1] + labels[:, 3] / 2) * W
        y1, y2 = (labels[:, 2] - labels[:, 4] / 2) * H, (labels[:, 2] + labels[:, 4] / 2) * H
        return self._warp_boxes(labels, x1, y1, x2, y2, M, gain)

    def _warp_boxes(self, labels, x1, y1, x2, y2, M, gain):
        """The pixel-coordinate core of _warp_labels: boxes (x1, y1, x2, y2) in pixels of the warp's INPUT (the net-input image, or the
        mosaic canvas) through M into the H x W output -> the kept rows of `labels`, columns 1 .. 4 the new normalised boxes."""
        H, W = self.input_shape[0], self.input_shape[1]
        n = len(labels)
        xy = np.ones((n * 4, 3))
        xy[:, 0] = np.stack([x1, x2, x1, x2], 1).reshape(-1)
        xy[:, 1] = np.stack([y1, y2, y2, y1], 1).reshape(-1)
        xy = xy @ M.T
        xy = (xy[:, :2] / xy[:, 2:3]).reshape(n, 4, 2)
        nx1, nx2 = xy[:, :, 0].min(1).clip(0, W), xy[:, :, 0].max(1).clip(0, W)
        ny1, ny2 = xy[:, :, 1].min(1).clip(0, H), xy[:, :, 1].max(1).clip(0, H)
        w1, h1 = (x2 - x1) * gain, (y2 - y1) * gain
        w2, h2 = nx2 - nx1, ny2 - ny1
        ar = np.maximum(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16))
        keep = (w2 > 2) & (h2 > 2) & (w2 * h2 / (w1 * h1 + 1e-16) > 0.1) & (ar < 20)
        out = labels.copy()
        out[:, 1], out[:, 2], out[:, 3], out[:, 4] = (nx1 + nx2) / 2 / W, (ny1 + ny2) / 2 / H, w2 / W, h2 / H
        return out[keep]

    def _mosaic_labels(self, tiles, xc, yc, M, gain):
        """yolov5's load_mosaic labels: each tile's normalised rows to canvas pixels (xywhn2xyxy with the tile's padw = x1a - x1b, padh =
        y1a - y1b), concatenated in tile order, clipped to the 2W x 2H canvas, then the label half of random_perspective (_warp_boxes:
        box_candidates compares with the CLIPPED canvas boxes times gain).  -> normalised (cls, xc, yc, w, h) rows, possibly none."""
        H, W = self.input_shape[0], self.input_shape[1]
        rows = []
        for q, t in enumerate(tiles):
            lab = self._labels(t)
            if not len(lab):
                continue
            x1a, y1a, _, _, x1b, y1b, _, _ = mosaic_placement(q, xc, yc, H, W)
            padw, padh = x1a - x1b, y1a - y1b
            box = lab.copy()
            box[:, 1] = W * (lab[:, 1] - lab[:, 3] / 2) + padw
            box[:, 2] = H * (lab[:, 2] - lab[:, 4] / 2) + padh
            box[:, 3] = W * (lab[:, 1] + lab[:, 3] / 2) + padw
            box[:, 4] = H * (lab[:, 2] + lab[:, 4] / 2) + padh
            rows.append(box)
        if not rows:
            return np.zeros((0, 5))
        box = np.concatenate(rows)
        box[:, [1, 3]] = box[:, [1, 3]].clip(0, 2 * W)
        box[:, [2, 4]] = box[:, [2, 4]].clip(0, 2 * H)
        return self._warp_boxes(box, box[:, 1], box[:, 2], box[:, 3], box[:, 4], M, gain)

    def draw_ex(self, index):
        """draw() with the geometric part: -> (k, flip, boxes, flipud, coeffs), coeffs the eight float64 output -> input coefficients of
        the item's warp, or None while the geometric keys are neutral.  Draws: [eight for the warp, when any of degrees / translate /
        scale / shear / perspective is set], [the mixup draws, see draw_mix], blur?, which blur, fliplr?, [flipud?, when flipud > 0].
        Labels: the reference's normalisation, the warp (boxes it drops are compacted out before the max_boxes fill), [the partner's rows],
        x = 1 - x for fliplr, y = 1 - y for flipud.  draw_mix returns the mixup draws as well."""
        return self.draw_mix(index)[:5]

    def _labels(self, index):
        """The reference's normalised (cls, xc, yc, w, h) rows of one item, by the configured origin_img_shape (:126-131); with
        letterbox=True yolov5's rows in the letterboxed net image instead (the module docstring has the rule): the label-file row by the
        frame's own size, xywhn2xyxy with letterbox's ratio and float pad, xyxy2xywhn(clip=True, eps=1e-3).  float64 throughout."""
        labels = np.array(self.dataset_dict[self.img_list[index]])
        if len(labels) and self.letterbox:
            h, w = self._frame_hw[self.img_list[index]]
            H, W = self.input_shape[0], self.input_shape[1]
            labels[:, 1:5] = xyxy2xywh(labels[:, 1:5])
            labels[:, [2, 4]] /= h
            labels[:, [1, 3]] /= w
            r = min(H / h, W / w)
            new_w, new_h = int(round(w * r)), int(round(h * r))
            dw, dh = (W - new_w) / 2, (H - new_h) / 2
            x = labels[:, 1:5].copy()
            box = np.zeros_like(x)                                                   # xywhn2xyxy(x, r * w, r * h, dw, dh)
            box[:, 0] = (r * w) * (x[:, 0] - x[:, 2] / 2) + dw
            box[:, 1] = (r * h) * (x[:, 1] - x[:, 3] / 2) + dh
            box[:, 2] = (r * w) * (x[:, 0] + x[:, 2] / 2) + dw
            box[:, 3] = (r * h) * (x[:, 1] + x[:, 3] / 2) + dh
            box[:, [0, 2]] = box[:, [0, 2]].clip(0, W - 1e-3)                        # xyxy2xywhn(box, W, H, clip=True, eps=1e-3)
            box[:, [1, 3]] = box[:, [1, 3]].clip(0, H - 1e-3)
            labels[:, 1] = ((box[:, 0] + box[:, 2]) / 2) / W
            labels[:, 2] = ((box[:, 1] + box[:, 3]) / 2) / H
            labels[:, 3] = (box[:, 2] - box[:, 0]) / W
            labels[:, 4] = (box[:, 3] - box[:, 1]) / H
        elif len(labels):
            labels[:, 1:5] = xyxy2xywh(labels[:, 1:5])
            labels[:, [2, 4]] /= self.origin_img_shape[0]
            labels[:, [1, 3]] /= self.origin_img_shape[1]
        return labels

    def draw_mix(self, index):
        """The whole record of one item: -> (k, flip, boxes, flipud, coeffs, partner, partner_coeffs, r); the last three are None unless
        mixup is active (mixup=True, augment, augment_params["mixup"] = p > 0) and the item was hit.  The draws, all from the global
        `random` module, in order:
          1. the item's eight warp draws (_draw_warp), when the geometric keys are active;
          2. random.random() < p, when mixup is active; on a hit:
          3.   partner = random.randint(0, len(self) - 1) -- it may be the item itself;
          4.   the partner's own eight warp draws (_draw_warp, with its redraw rule), when geometric;
          5.   r = random.betavariate(32.0, 32.0): yolov5 draws np.random.beta(32.0, 32.0) from numpy's generator; here the value comes
               from `random`, so that random.seed alone reproduces an epoch;
          6. as without mixup: blur?, which blur, fliplr?, [flipud?].
        The partner gets no blur or flip draws: those act on the mixture.  Labels: the partner's rows (the reference's normalisation, then
        the partner's own warp) are appended AFTER the item's; both flips act on all rows; the max_boxes fill runs last, so truncation
        drops partner rows first; an image without objects contributes no rows, on either side.
        With mosaic active (draw_mosaic) the draws are draw_mosaic's, and an item that became a mosaic has coeffs None here."""
        return self.draw_mosaic(index)[:8]

    def draw_mosaic(self, index):
        """draw_mix's eight values and a ninth: None, or (xc, yc, tiles, coeffs) for an item that became a mosaic -- yolov5's
        load_mosaic for the rectangular net input H x W.  Mosaic is active with mosaic=True, augment and augment_params["mosaic"] = p > 0;
        inactive, no draw is added and the ninth value is None.  Active, the draws of an item are:
          1. random.random() < p; on a miss the item goes on as draw_mix describes, from its step 1;
          2. on a hit yc = int(random.uniform(H // 2, 2 * H - H // 2)), THEN xc = int(random.uniform(W // 2, 2 * W - W // 2));
          3. tiles = [index] + random.choices(range(len(self)), k=3), then random.shuffle(tiles): top-left, top-right, bottom-left,
             bottom-right (mosaic_placement);
          4. _draw_warp(mosaic=True)'s eight draws, ALWAYS (with neutral keys the ranges are empty; the warp is then the central crop);
          5. blur?, which blur, fliplr?, [flipud?].
        A hit's first eight values are (k, flip, boxes, flipud, None, None, None, None): the single frame has no warp of its own and no
        partner (mosaic and mixup are not combined).  Labels of a hit: _mosaic_labels, then the flips and the max_boxes fill (truncation
        drops the later rows)."""
        labels = self._labels(index)
        k, flip, flipud, coeffs = 0, False, False, None
        partner = partner_coeffs = r = mosaic = None
        if self.augment:
            if self.mosaic > 0 and random.random() < self.mosaic:
                H, W = self.input_shape[0], self.input_shape[1]
                yc = int(random.uniform(H // 2, 2 * H - H // 2))
                xc = int(random.uniform(W // 2, 2 * W - W // 2))
                tiles = [index] + random.choices(range(len(self)), k=3)
                random.shuffle(tiles)
                M, gain, canvas_coeffs = self._draw_warp(mosaic=True)
                labels = self._mosaic_labels(tiles, xc, yc, M, gain)
                mosaic = (xc, yc, tiles, canvas_coeffs)
            elif self.geometric:
                M, gain, coeffs = self._draw_warp()
                if len(labels):
                    labels = self._warp_labels(labels, M, gain)
            if mosaic is None and self.mixup > 0 and random.random() < self.mixup:
                partner = random.randint(0, len(self) - 1)
                other = self._labels(partner)
                if self.geometric:
                    M, gain, partner_coeffs = self._draw_warp()
                    if len(other):
                        other = self._warp_labels(other, M, gain)
                r = random.betavariate(32.0, 32.0)
                if len(other):
                    labels = np.concatenate([labels, other]) if len(labels) else other
            if random.random() < self.gussian_filter:
                _ret = random.random()
                k = 7 if _ret < 0.4 else 3          # the reference's `elif _ret < 0.2` (5 x 5) cannot be reached
            if random.random() < self.fliplr:
                flip = True
                if len(labels):                     # deviation: no IndexError for an image without objects (nor ValueError below)
                    labels[:, 1] = 1 - labels[:, 1]
            if self.flipud > 0 and random.random() < self.flipud:
                flipud = True
                if len(labels):
                    labels[:, 2] = 1 - labels[:, 2]
        nL = len(labels)
        if nL:
            cls_id = labels[:, 0].copy()
            labels[:, 0:4] = labels[:, 1:5]
            labels[:, 4] = cls_id
        out = np.zeros([self.max_boxes, 6])
        m = min(nL, self.max_boxes)
        if m:                                       # deviation: the reference's copy raises ValueError for no objects
            out[:m, 0:5] = labels[:m]
            out[:m, 5] = 255.0
        return k, flip, out, flipud, coeffs, partner, partner_coeffs, r, mosaic

    # ---- images (GPU) ----
    def _need_gpu(self):
        if self.device.type != "cuda":
            raise RuntimeError("DetectDataset images have no CPU path (csrc/yf_aug_kernels.hip): pass device='cuda'")

    def _decode(self, index):
        """cv2.imread's frame: uint8 [h, w, 3], BGR (PIL decode, channels reversed as detect.py does)."""
        from PIL import Image
        with Image.open(self.img_list[index]) as im:
            rgb = np.asarray(im.convert("RGB"))
        bgr = np.ascontiguousarray(rgb[:, :, ::-1])
        self._check_size(index, bgr.shape[:2])
        return bgr

    def _check_size(self, index, hw):
        if self.letterbox:
            want = self._frame_hw[self.img_list[index]]
            if tuple(hw) != tuple(want):
                raise ValueError("%s decodes to %dx%d, but %dx%d was recorded for it (the XML's <size>, else the image header): its "
                                 "labels were letterboxed for that size" % (self.img_list[index], hw[0], hw[1], want[0], want[1]))
            return
        if list(self.input_shape[0:2]) == list(self.origin_img_shape[0:2]) and list(hw) != list(self.input_shape[0:2]):
            raise ValueError("%s is %dx%d, but origin_img_shape[:2] == input_shape[:2] = %s: the reference does not resize then and "
                             "would yield a mis-shaped image" % (self.img_list[index], hw[0], hw[1], self.input_shape[0:2]))

    def _decode_device(self, indices):
        """decode="device": the frames `indices` in one decode call per source size -> [(indices of the group, uint8 device [n, h, w, 3])]."""
        groups = jpeg.decode_files([self.img_list[i] for i in indices], self.device, progressive=self.progressive)
        out = []
        for g in groups:
            members = [indices[p] for p in g.positions]
            for i in members:
                self._check_size(i, tuple(g.bgr.shape[1:3]))
            out.append((members, g.bgr))
        return out

    def _append(self, indices, frames):
        """cache="device": the frames `indices`, uint8 [k, h, w, 3] of one size (a host array or a device tensor), to the end of that size's
        stack (8 slots at first, doubled while too small); records their slots."""
        hw = tuple(frames.shape[1:3])
        ent = self._stacks.get(hw)
        if ent is None:
            ent = self._stacks[hw] = [torch.empty((8,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=self.device), 0]
        need = ent[1] + len(indices)
        if need > ent[0].shape[0]:
            cap = ent[0].shape[0]
            while cap < need:
                cap *= 2
            grown = torch.empty((cap,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=self.device)
            grown[:ent[1]].copy_(ent[0][:ent[1]])
            ent[0] = grown
        ent[0][ent[1]:need].copy_(torch.as_tensor(frames))
        for k, i in enumerate(indices):
            self._slot[i] = (hw, ent[1] + k)
        ent[1] = need

    # Where the frames of a batch are: per source size (uint8 device stack [n_src, h, w, 3], slot in it per member -- None: the stack is
    # the members in order --, position in the batch per member).
    def _from_cache(self, indices):
        """cache="device": the stacks of the cache; frames not in it yet are decoded (decode="device": in one call per size) and appended."""
        if self.decode == "device":
            for members, bgr in self._decode_device(list(dict.fromkeys(i for i in indices if i not in self._slot))):
                self._append(members, bgr)
        groups = {}
        for pos, i in enumerate(indices):
            if i not in self._slot:
                self._append([i], self._decode(i)[None])
            hw, slot = self._slot[i]
            slots, at = groups.setdefault(hw, ([], []))
            slots.append(slot)
            at.append(pos)
        return [(self._stacks[hw][0][:self._stacks[hw][1]], slots, at) for hw, (slots, at) in groups.items()]

    def _from_device_decode(self, indices):
        """decode="device": each distinct frame decoded once, one call per size."""
        out = []
        for members, bgr in self._decode_device(list(dict.fromkeys(indices))):
            slot = {i: k for k, i in enumerate(members)}
            at = [pos for pos, i in enumerate(indices) if i in slot]
            out.append((bgr, [slot[indices[pos]] for pos in at], at))
        return out

    def _from_host_decode(self, indices):
        """decode="host": every member decoded by PIL, one upload per size."""
        frames = {}
        for pos, i in enumerate(indices):
            bgr = self._decode(i)
            stack, at = frames.setdefault(bgr.shape[:2], ([], []))
            stack.append(bgr)
            at.append(pos)
        return [(torch.from_numpy(np.stack(stack)).to(self.device), None, at) for stack, at in frames.values()]

    def _resize_tables(self, hw, stream):
        H, W = self.input_shape[0], self.input_shape[1]
        if tuple(hw) in ((H, W), (2 * H, 2 * W)):
            return None, None
        t = self._tables.get(hw)
        if t is None:
            t = self._tables[hw] = torch.empty(((W + H) * 16,), dtype=torch.uint8, device=self.device)
            _lib.check(_lib.lib().yf_cv_resize_tables(self.device.index, hw[0], hw[1], H, W, t.data_ptr(), t.data_ptr() + W * 16, stream))
        return t.data_ptr(), t.data_ptr() + W * 16

    def _groups(self, indices):
        """Where the frames `indices` are, by the configured cache / decode."""
        if self.cache == "device":
            return self._from_cache(indices)
        if self.decode == "device":
            return self._from_device_decode(indices)
        return self._from_host_decode(indices)

    def _resize_distinct(self, distinct, stream):
        """The distinct frames `distinct` resized (and grayed) once: yf_augment_u8 with zero parameters, one launch per source size, each
        into its slice of one u8 scratch -> (scratch [len(distinct), H, W, C], item -> its frame in the scratch)."""
        H, W, C = self.input_shape
        dev, lib = self.device, _lib.lib()
        scratch = torch.empty((len(distinct), H, W, C), dtype=torch.uint8, device=dev)
        if self.letterbox:                                   # ONE yf_cv_letterbox_u8 launch over all of them, whatever their sizes
            keep, ptrs, hs, ws = self._frame_pointers(distinct)
            n, table = len(distinct), self._pinned_table(len(distinct))
            _lib.check(lib.yf_cv_letterbox_u8(dev.index, n, (ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*hs), (ctypes.c_int * n)(*ws),
                                              0 if C == 3 else self.gray_bits, H, W, scratch.data_ptr(), *table.args, ctypes.c_void_p(stream)))
            table.uploaded(n, torch.cuda.current_stream(dev))
            del keep
            return scratch, {i: j for j, i in enumerate(distinct)}
        where, base = {}, 0                                  # item -> its frame in the scratch
        for stack, slots, pos in self._groups(distinct):
            hw = tuple(stack.shape[1:3])
            index = None if slots is None else torch.tensor(slots, dtype=torch.int32).to(dev)
            zero = torch.zeros((len(pos),), dtype=torch.int32, device=dev)
            xt, yt = self._resize_tables(hw, stream)
            _lib.check(lib.yf_augment_u8(dev.index, stack.data_ptr(), hw[0], hw[1], 3, None if index is None else index.data_ptr(),
                                         stack.shape[0], len(pos), xt, yt, H, W, C, self.gray_bits, zero.data_ptr(),
                                         scratch[base:base + len(pos)].data_ptr(), None, ctypes.c_void_p(stream)))
            for j, p in enumerate(pos):
                where[distinct[p]] = base + j
            base += len(pos)
        return scratch, where

    def _frame_pointers(self, indices):
        """letterbox: where each frame of `indices` starts, from however many stacks _groups returns: a member's pointer is its stack's
        plus slot * h * w * 3.  -> (the stacks, to be kept until the launch is queued; pointers, heights, widths in batch order)."""
        n = len(indices)
        keep, ptrs, hs, ws = [], [0] * n, [0] * n, [0] * n
        for stack, slots, pos in self._groups(indices):
            stack = stack.contiguous()
            h, w = int(stack.shape[1]), int(stack.shape[2])
            keep.append(stack)
            for j, p in enumerate(pos):
                ptrs[p], hs[p], ws[p] = stack.data_ptr() + (j if slots is None else slots[j]) * h * w * 3, h, w
        return keep, ptrs, hs, ws

    def _pinned_table(self, n):
        """letterbox: the per-frame table of the two letterbox entries, as model.letterbox_u8 keeps it: every call uploads, so the previous
        upload must have left the pinned copy before the entry refills it."""
        from .training import _PinnedTable
        table = self._lb_table
        if table is not None and table.event is not None:
            table.event.synchronize()
        if table is None or table.args[1] < _lib.YF_LB_TABLE_ENTRY_BYTES * n:
            table = self._lb_table = _PinnedTable(_lib.YF_LB_TABLE_ENTRY_BYTES * max(n, 256), self.device)
        return table

    def _letterbox_images(self, indices, packed, warps, out, out_u8, stream):
        """letterbox, a batch without mixup or mosaic hits: ONE yf_augment_letterbox_u8 call for all of it, mixed sizes or not."""
        H, W, C = self.input_shape
        dev, n = self.device, len(indices)
        if not n:
            return
        keep, ptrs, hs, ws = self._frame_pointers(indices)
        prm = torch.tensor(packed, dtype=torch.int32).to(dev)
        geometric = any(p >> 9 for p in packed)
        warp = None
        scratch = torch.empty((n, H, W, C), dtype=torch.uint8, device=dev)
        if geometric:
            neutral = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
            warp = torch.tensor([neutral if w is None else [float(v) for v in w] for w in warps], dtype=torch.float64).to(dev)
        table = self._pinned_table(n)
        _lib.check(_lib.lib().yf_augment_letterbox_u8(
            dev.index, n, (ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*hs), (ctypes.c_int * n)(*ws), 0 if C == 3 else self.gray_bits, H, W,
            prm.data_ptr(), int(geometric), None if warp is None else warp.data_ptr(), scratch.data_ptr(),
            out.data_ptr() if out_u8 else None, None if out_u8 else out.data_ptr(), *table.args, ctypes.c_void_p(stream)))
        table.uploaded(n, torch.cuda.current_stream(dev))
        del keep

    def _mix_images(self, indices, packed, warps, mixes, out, out_u8, stream):
        """A batch with at least one mixup hit: every distinct frame of items and partners resized once (_resize_distinct), then one
        yf_augment_mix_u8 into `out`."""
        H, W, C = self.input_shape
        dev, lib = self.device, _lib.lib()
        distinct = list(dict.fromkeys(list(indices) + [m[0] for m in mixes if m is not None]))
        scratch, where = self._resize_distinct(distinct, stream)
        neutral = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
        first = torch.tensor([where[i] for i in indices], dtype=torch.int32).to(dev)
        second = torch.tensor([-1 if m is None else where[m[0]] for m in mixes], dtype=torch.int32).to(dev)
        prm = torch.tensor(packed, dtype=torch.int32).to(dev)
        warp = torch.tensor([[neutral if w is None else [float(v) for v in w],
                              neutral if m is None or m[1] is None else [float(v) for v in m[1]]] for w, m in zip(warps, mixes)],
                            dtype=torch.float64).to(dev)
        ratio = torch.tensor([1.0 if m is None else m[2] for m in mixes], dtype=torch.float64).to(dev)
        _lib.check(lib.yf_augment_mix_u8(dev.index, scratch.data_ptr(), len(distinct), len(indices), H, W, C, first.data_ptr(), second.data_ptr(),
                                         prm.data_ptr(), warp.data_ptr(), ratio.data_ptr(), out.data_ptr() if out_u8 else None,
                                         None if out_u8 else out.data_ptr(), ctypes.c_void_p(stream)))

    def _mosaic_images(self, indices, packed, warps, mosaics, out, out_u8, stream):
        """A batch with at least one mosaic: every distinct frame of items and tiles resized once (_resize_distinct), then one
        yf_augment_mosaic_u8 into `out`; an item that is no mosaic is its own frame with tile slots 1 .. 3 at -1 (the warp call's bytes)."""
        H, W, C = self.input_shape
        dev, lib = self.device, _lib.lib()
        distinct = list(dict.fromkeys(list(indices) + [int(t) for m in mosaics if m is not None for t in m[2]]))
        scratch, where = self._resize_distinct(distinct, stream)
        neutral = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
        tiles = torch.tensor([[where[i], -1, -1, -1] if m is None else [where[int(t)] for t in m[2]] for i, m in zip(indices, mosaics)],
                             dtype=torch.int32).to(dev)
        centre = torch.tensor([[0, 0] if m is None else [int(m[0]), int(m[1])] for m in mosaics], dtype=torch.int32).to(dev)
        prm = torch.tensor(packed, dtype=torch.int32).to(dev)
        warp = torch.tensor([neutral if w is None else [float(v) for v in w] for w in warps], dtype=torch.float64).to(dev)
        _lib.check(lib.yf_augment_mosaic_u8(dev.index, scratch.data_ptr(), len(distinct), len(indices), H, W, C, tiles.data_ptr(),
                                            centre.data_ptr(), prm.data_ptr(), warp.data_ptr(), out.data_ptr() if out_u8 else None,
                                            None if out_u8 else out.data_ptr(), ctypes.c_void_p(stream)))

    def augment_images(self, indices, params, out_u8=False):
        """The frames `indices` with per-frame `params` -- (k, flip), (k, flip, flipud, coeffs), draw_ex's values, or those extended by
        draw_mix's (partner, partner_coeffs, r) -- through yf_augment_u8, one launch per source size; a size group with a warped or
        flipud frame goes through yf_augment_warp_u8 (two).  With at least one partner: the distinct frames of items and partners resized
        by yf_augment_u8 (one launch per source size) into one u8 scratch, then ONE yf_augment_mix_u8 for the whole batch.
        Extended once more by draw_mosaic's ninth value (None, or (xc, yc, tiles, coeffs)): with at least one mosaic, the distinct
        frames of items and tiles resized the same way, then ONE yf_augment_mosaic_u8 for the whole batch.
        With letterbox=True a batch without partners or mosaics is ONE yf_augment_letterbox_u8 call whatever its frame sizes; with them
        the distinct frames are letterboxed by one yf_cv_letterbox_u8 launch in place of the per-size resizes.
        -> float32 device [N, C, H, W] ((v - 128) / 255), or uint8 device [N, H, W, C] with out_u8."""
        self._need_gpu()
        H, W, C = self.input_shape
        N = len(indices)
        dev = self.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        out = torch.empty((N, H, W, C) if out_u8 else (N, C, H, W), dtype=torch.uint8 if out_u8 else torch.float32, device=dev)
        packed, warps, mixes, mosaics = [], [], [], []
        for k, f, *rest in params:
            ud, coeffs, partner, pcoeffs, r, mosaic = (tuple(rest) + (None, None, None, None))[:6] if rest else (False, None, None, None, None, None)
            if mosaic is not None:
                if partner is not None:
                    raise ValueError("a frame cannot be a mosaic and have a mixup partner: the two are not combined")
                coeffs = mosaic[3]                              # the canvas's coefficients take the frame's slot
            mosaics.append(mosaic)
            warps.append(coeffs)
            mixes.append(None if partner is None else (int(partner), pcoeffs, float(r)))
            packed.append(int(k) | (int(bool(f)) << 8) | (int(bool(ud)) << 9) |
                          (0 if coeffs is None else (1 << 10) | (int(coeffs[6] != 0 or coeffs[7] != 0) << 11)) |
                          (0 if partner is None or pcoeffs is None else (1 << 12) | (int(pcoeffs[6] != 0 or pcoeffs[7] != 0) << 13)))
        lib = _lib.lib()
        if any(m is not None for m in mosaics):
            if any(m is not None for m in mixes):
                raise ValueError("a batch cannot hold mosaics and mixup partners: the two are not combined")
            self._mosaic_images(indices, packed, warps, mosaics, out, out_u8, stream)
            return out
        if any(m is not None for m in mixes):
            self._mix_images(indices, packed, warps, mixes, out, out_u8, stream)
            return out
        if self.letterbox:
            self._letterbox_images(indices, packed, warps, out, out_u8, stream)
            return out
        groups = self._groups(indices)
        for stack, slots, pos in groups:
            hw = tuple(stack.shape[1:3])
            index = None if slots is None else torch.tensor(slots, dtype=torch.int32).to(dev)
            prm = torch.tensor([packed[p] for p in pos], dtype=torch.int32).to(dev)
            whole = len(groups) == 1
            dst = out if whole else torch.empty((len(pos),) + tuple(out.shape[1:]), dtype=out.dtype, device=dev)
            xt, yt = self._resize_tables(hw, stream)
            head = (dev.index, stack.data_ptr(), hw[0], hw[1], 3, None if index is None else index.data_ptr(), stack.shape[0], len(pos), xt, yt,
                    H, W, C, self.gray_bits, prm.data_ptr())
            tail = (dst.data_ptr() if out_u8 else None, None if out_u8 else dst.data_ptr(), ctypes.c_void_p(stream))
            if any(packed[p] >> 9 for p in pos):
                neutral = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
                warp = torch.tensor([neutral if warps[p] is None else [float(v) for v in warps[p]] for p in pos], dtype=torch.float64).to(dev)
                scratch = torch.empty((len(pos), H, W, C), dtype=torch.uint8, device=dev)
                _lib.check(lib.yf_augment_warp_u8(*head, warp.data_ptr(), scratch.data_ptr(), *tail))
            else:
                _lib.check(lib.yf_augment_u8(*head, *tail))
            if not whole:
                out.index_copy_(0, torch.tensor(pos, device=dev), dst)
        return out

    def __getitem__(self, index):
        """The reference's item: (float64 [H, W, C] image u8 - 128.0, float64 [max_boxes, 6] boxes)."""
        self._need_gpu()
        k, flip, boxes, flipud, coeffs, partner, partner_coeffs, r, mosaic = self.draw_mosaic(index)
        u8 = self.augment_images([index], [(k, flip, flipud, coeffs, partner, partner_coeffs, r, mosaic)], out_u8=True)[0].cpu().numpy()
        img = u8 - 128.0
        return np.ascontiguousarray(img), boxes

    def __getitems__(self, indices):
        """A whole batch: the draws of `indices` in order (as item after item would make them), images in one launch per source size.
        -> DetectBatch(float32 device [N, C, H, W], float64 host [N, max_boxes, 6]); collate_fn passes it through."""
        self._need_gpu()
        indices = [int(i) for i in indices]
        draws = [self.draw_mosaic(i) for i in indices]
        tail = 4 if self.augment and self.mosaic > 0 else 3      # the mosaic value travels only where one can occur
        imgs = self.augment_images(indices, [(k, f, ud, coeffs) + tuple(mix[:tail]) for k, f, _, ud, coeffs, *mix in draws])
        targets = torch.from_numpy(np.stack([d[2] for d in draws])) if draws else torch.zeros((0, self.max_boxes, 6), dtype=torch.float64)
        return DetectBatch(imgs, targets)

    @staticmethod
    def collate_fn(batch):
        """detect_dataset.py:105-117 (stack, NHWC -> NCHW, / 255: float64 images) for a list of items; a DetectBatch passes through."""
        if isinstance(batch, DetectBatch):
            return batch
        images = []
        bboxes = []
        for img, box in batch:
            images.append([img])
            bboxes.append([box])
        images = np.concatenate(images, axis=0)
        bboxes = np.concatenate(bboxes, axis=0)
        images = images.transpose(0, 3, 1, 2)
        images = torch.from_numpy(images).div(255.0)
        bboxes = torch.from_numpy(bboxes)
        return images, bboxes
