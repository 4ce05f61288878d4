"""TEST INFRASTRUCTURE: the label half of DetectDataset(letterbox=True), transcribed line by line from yolov5 (utils/augmentations.py
`letterbox`, utils/general.py `xywhn2xyxy`, `clip_boxes`, `xyxy2xywhn`, and the non-mosaic branch of utils/dataloaders.py
`LoadImagesAndLabels.__getitem__`) for numpy arrays.  Python floats and numpy float64 are IEEE doubles and the operations are written
in yolov5's order, so dataset.py's `_labels` has to give these rows bit for bit."""
import numpy as np


def letterbox_ratio_pad(shape, new_shape):
    """yolov5's letterbox(im, new_shape, auto=False, scaleFill=False, scaleup=True) without the pixels: shape = (h, w), new_shape = (H, W)
    -> (ratio, (dw, dh)), dw and dh the FLOAT pad of one side."""
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    ratio = r, r
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    dw /= 2
    dh /= 2
    return ratio, (dw, dh)


def xywhn2xyxy(x, w=640, h=640, padw=0, padh=0):
    y = np.copy(x)
    y[..., 0] = w * (x[..., 0] - x[..., 2] / 2) + padw
    y[..., 1] = h * (x[..., 1] - x[..., 3] / 2) + padh
    y[..., 2] = w * (x[..., 0] + x[..., 2] / 2) + padw
    y[..., 3] = h * (x[..., 1] + x[..., 3] / 2) + padh
    return y


def clip_boxes(boxes, shape):
    boxes[..., [0, 2]] = boxes[..., [0, 2]].clip(0, shape[1])
    boxes[..., [1, 3]] = boxes[..., [1, 3]].clip(0, shape[0])


def xyxy2xywhn(x, w=640, h=640, clip=False, eps=0.0):
    if clip:
        clip_boxes(x, (h - eps, w - eps))
    y = np.copy(x)
    y[..., 0] = ((x[..., 0] + x[..., 2]) / 2) / w
    y[..., 1] = ((x[..., 1] + x[..., 3]) / 2) / h
    y[..., 2] = (x[..., 2] - x[..., 0]) / w
    y[..., 3] = (x[..., 3] - x[..., 1]) / h
    return y


def label_file_rows(pixel_boxes, h, w):
    """The rows of a yolov5 label file from VOC pixel boxes [(cls, x1, y1, x2, y2)] of an h x w frame: (cls, xc, yc, bw, bh) / (w, h), in
    the reference's arithmetic (detect_dataset.py:126-131 with the frame's own size)."""
    rows = np.array(pixel_boxes, np.float64).reshape(-1, 5)
    out = rows.copy()
    out[:, 1] = (rows[:, 1] + rows[:, 3]) / 2
    out[:, 2] = (rows[:, 2] + rows[:, 4]) / 2
    out[:, 3] = rows[:, 3] - rows[:, 1]
    out[:, 4] = rows[:, 4] - rows[:, 2]
    out[:, [2, 4]] /= h
    out[:, [1, 3]] /= w
    return out


def letterboxed_rows(pixel_boxes, h, w, H, W):
    """__getitem__'s non-mosaic branch: `labels[:, 1:] = xywhn2xyxy(labels[:, 1:], ratio[0] * w, ratio[1] * h, padw=pad[0], padh=pad[1])`,
    then `labels[:, 1:5] = xyxy2xywhn(labels[:, 1:5], w=img.shape[1], h=img.shape[0], clip=True, eps=1e-3)`.  -> (cls, xc, yc, bw, bh) rows."""
    labels = label_file_rows(pixel_boxes, h, w)
    if not len(labels):
        return labels
    ratio, pad = letterbox_ratio_pad((h, w), (H, W))
    labels[:, 1:] = xywhn2xyxy(labels[:, 1:], ratio[0] * w, ratio[1] * h, padw=pad[0], padh=pad[1])
    labels[:, 1:5] = xyxy2xywhn(labels[:, 1:5], w=W, h=H, clip=True, eps=1e-3)
    return labels


def targets(rows, fliplr, flipud, max_boxes):
    """rows -> DetectDataset's (max_boxes, 6) boxes (xc, yc, w, h, cls, 255.0): the flips, then the fill."""
    rows = rows.copy()
    out = np.zeros((max_boxes, 6))
    if len(rows):
        if fliplr:
            rows[:, 1] = 1 - rows[:, 1]
        if flipud:
            rows[:, 2] = 1 - rows[:, 2]
        m = min(len(rows), max_boxes)
        out[:m, 0:4] = rows[:m, 1:5]
        out[:m, 4] = rows[:m, 0]
        out[:m, 5] = 255.0
    return out
