"""The CPU statement of the letterbox mode (include/yolo_fastest_hip.h: yf_letterbox_geometry, yf_cv_letterbox_u8, yf_scale_boxes): yolov5's
`letterbox(im, (H, W), auto=False, scaleFill=False, scaleup=True)` with the reference's pixel arithmetic (oracle/cv_oracle.py: cvtColor, then
cv2.resize, then a border of 114), and yolov5's `scale_boxes(..., ratio_pad=None)` followed by `.round()`.  Python floats are IEEE doubles
and Python's `round` rounds half to even: the expressions below ARE the rule, the C entries restate them."""
import numpy as np

from oracle import cv_oracle as cv

BORDER = 114


def geometry(h, w, H, W):
    """-> (new_h, new_w, top, bottom, left, right)"""
    r = min(H / h, W / w)
    new_w, new_h = int(round(w * r)), int(round(h * r))
    dw, dh = (W - new_w) / 2, (H - new_h) / 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return new_h, new_w, top, bottom, left, right


def letterbox_u8(bgr, H, W, gray_bits):
    """uint8 [h, w, 3] (BGR) -> uint8 [H, W] (gray_bits 14 | 15) or [H, W, 3] (gray_bits 0)."""
    bgr = np.asarray(bgr)
    h, w = bgr.shape[:2]
    new_h, new_w, top, bottom, left, right = geometry(h, w, H, W)
    assert top + new_h + bottom == H and left + new_w + right == W
    img = cv.cvt_bgr2gray(bgr, gray_bits) if gray_bits else bgr
    img = cv.resize_linear_u8(img, (new_w, new_h))
    out = np.full((H, W) + img.shape[2:], BORDER, dtype=np.uint8)
    out[top:top + new_h, left:left + new_w] = img
    return out


def scale_boxes_ref(boxes, H, W, h, w):
    """boxes: rows of ints (x1, y1, x2, y2) in net coordinates -> rows of ints in the (h, w) frame's."""
    gain = min(H / h, W / w)
    pad_w, pad_h = (W - w * gain) / 2, (H - h * gain) / 2
    out = []
    for b in boxes:
        row = []
        for c, v in enumerate(b):
            pad, lim = (pad_h, h) if c & 1 else (pad_w, w)
            row.append(int(round(min(max((int(v) - pad) / gain, 0), lim))))
        out.append(row)
    return out
