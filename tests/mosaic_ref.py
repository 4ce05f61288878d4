"""TEST INFRASTRUCTURE: yolov5's mosaic (utils/dataloaders.py: load_mosaic; utils/augmentations.py: random_perspective, box_candidates)
restated for a rectangular net input H x W, the yardstick of mosaic_kernel (csrc/yf_aug_kernels.hip, yf_augment_mosaic_u8) and of
DetectDataset.draw_mosaic's labels.  Every tile is already H x W, so `s * 2` becomes 2W / 2H:
    canvas = np.full((2H, 2W, C), 114); canvas[y1a:y2a, x1a:x2a] = tile[y1b:y2b, x1b:x2b] for the four tiles around (xc, yc)
    image  = flipud(fliplr(blur_k(Image.transform((W, H), AFFINE | PERSPECTIVE, coeffs, BILINEAR, fillcolor=114) of the canvas)))
The canvas is materialised here, which the kernel never does; the transform is warp_ref's (Pillow itself, or its numpy restatement)."""
import numpy as np

import aug_ref
import warp_ref

FILL = warp_ref.FILL


def placement(q, xc, yc, H, W):
    """load_mosaic's rectangles of tile q (0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right)
    -> (x1a, y1a, x2a, y2a) on the canvas, (x1b, y1b, x2b, y2b) in the tile."""
    if q == 0:
        x1a, y1a, x2a, y2a = max(xc - W, 0), max(yc - H, 0), xc, yc
        x1b, y1b, x2b, y2b = W - (x2a - x1a), H - (y2a - y1a), W, H
    elif q == 1:
        x1a, y1a, x2a, y2a = xc, max(yc - H, 0), min(xc + W, 2 * W), yc
        x1b, y1b, x2b, y2b = 0, H - (y2a - y1a), min(W, x2a - x1a), H
    elif q == 2:
        x1a, y1a, x2a, y2a = max(xc - W, 0), yc, xc, min(2 * H, yc + H)
        x1b, y1b, x2b, y2b = W - (x2a - x1a), 0, W, min(y2a - y1a, H)
    else:
        x1a, y1a, x2a, y2a = xc, yc, min(xc + W, 2 * W), min(2 * H, yc + H)
        x1b, y1b, x2b, y2b = 0, 0, min(W, x2a - x1a), min(y2a - y1a, H)
    return (x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b)


def canvas_u8(tiles4, xc, yc):
    """tiles4: four uint8 [H, W] or [H, W, C] in the order TL, TR, BL, BR -> the uint8 canvas [2H, 2W(, C)]: the literal slice assignments."""
    tiles4 = [np.asarray(t) for t in tiles4]
    H, W = tiles4[0].shape[:2]
    assert all(t.dtype == np.uint8 and t.shape == tiles4[0].shape for t in tiles4)
    canvas = np.full((2 * H, 2 * W) + tiles4[0].shape[2:], FILL, np.uint8)
    for q, tile in enumerate(tiles4):
        (x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b) = placement(q, xc, yc, H, W)
        canvas[y1a:y2a, x1a:x2a] = tile[y1b:y2b, x1b:x2b]
    return canvas


def canvas_px(tiles4, xc, yc, cx, cy):
    """The kernel's rule for ONE canvas pixel (cx, cy): the quadrant from cx < xc, cy < yc; that quadrant's tile byte at (cx - padw,
    cy - padh) if (cx, cy) lies inside the tile's canvas rectangle; 114 otherwise."""
    H, W = np.asarray(tiles4[0]).shape[:2]
    q = (0 if cx < xc else 1) + (0 if cy < yc else 2)
    (x1a, y1a, x2a, y2a), (x1b, y1b, _, _) = placement(q, xc, yc, H, W)
    if x1a <= cx < x2a and y1a <= cy < y2a:
        padw, padh = x1a - x1b, y1a - y1b
        return tiles4[q][cy - padh, cx - padw]
    return np.full(np.asarray(tiles4[0]).shape[2:], FILL, np.uint8)


def compose_u8(tiles4, xc, yc, coeffs, perspective, k, fliplr, flipud, transform=warp_ref.pil_transform_u8):
    """What yf_augment_mosaic_u8 makes of one mosaic: flipud(fliplr(blur_k(transform(canvas, size=(H, W)))))."""
    H, W = np.asarray(tiles4[0]).shape[:2]
    img = transform(canvas_u8(tiles4, xc, yc), coeffs, perspective, size=(H, W))
    img = aug_ref.gaussian_blur_u8(np.ascontiguousarray(img), k)
    if fliplr:
        img = img[:, ::-1]
    if flipud:
        img = img[::-1]
    return np.ascontiguousarray(img)


def neutral_coeffs(H, W):
    """The output -> canvas map of the neutral warp: M = T C with C = translate(-W, -H), T = translate(W / 2, H / 2)."""
    return np.array([1.0, 0.0, W / 2, 0.0, 1.0, H / 2, 0.0, 0.0])


# ---- labels: yolov5's own functions, restated ----
def xywhn2xyxy(x, w, h, padw, padh):
    """utils/general.py: normalised (xc, yc, w, h) -> pixel (x1, y1, x2, y2) with a pad."""
    y = np.copy(x)
    y[..., 0] = w * (x[..., 0] - x[..., 2] / 2) + padw
    y[..., 1] = h * (x[..., 1] - x[..., 3] / 2) + padh
    y[..., 2] = w * (x[..., 0] + x[..., 2] / 2) + padw
    y[..., 3] = h * (x[..., 1] + x[..., 3] / 2) + padh
    return y


def box_candidates(box1, box2, wh_thr=2, ar_thr=20, area_thr=0.1, eps=1e-16):
    """utils/augmentations.py; ar_thr 20 is the value DetectDataset._warp_labels uses (yolov5's at the time of random_perspective's
    introduction; later releases raised it to 100)."""
    w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
    w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
    return (w2 > wh_thr) & (h2 > wh_thr) & (w2 * h2 / (w1 * h1 + eps) > area_thr) & (ar < ar_thr)


def mosaic_labels(rows4, xc, yc, H, W, M, gain):
    """rows4: per tile the normalised (cls, xc, yc, w, h) rows (possibly none), TL, TR, BL, BR; M the forward 3 x 3 matrix canvas ->
    output, gain its scale draw -> the normalised (cls, xc, yc, w, h) rows of the H x W output, float64.  load_mosaic's label lines,
    then random_perspective's."""
    labels4 = []
    for q, rows in enumerate(rows4):
        rows = np.asarray(rows, np.float64)
        if rows.size:
            (x1a, y1a, _, _), (x1b, y1b, _, _) = placement(q, xc, yc, H, W)
            lab = rows.copy()
            lab[:, 1:] = xywhn2xyxy(rows[:, 1:], W, H, x1a - x1b, y1a - y1b)
            labels4.append(lab)
    if not labels4:
        return np.zeros((0, 5))
    targets = np.concatenate(labels4, 0)
    targets[:, [1, 3]] = targets[:, [1, 3]].clip(0, 2 * W)
    targets[:, [2, 4]] = targets[:, [2, 4]].clip(0, 2 * H)
    n = len(targets)
    xy = np.ones((n * 4, 3))
    xy[:, :2] = targets[:, [1, 2, 3, 4, 1, 4, 3, 2]].reshape(n * 4, 2)          # x1y1, x2y2, x1y2, x2y1
    xy = xy @ M.T
    xy = (xy[:, :2] / xy[:, 2:3]).reshape(n, 8)
    x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
    new = np.concatenate((x.min(1), y.min(1), x.max(1), y.max(1))).reshape(4, n).T
    new[:, [0, 2]] = new[:, [0, 2]].clip(0, W)
    new[:, [1, 3]] = new[:, [1, 3]].clip(0, H)
    keep = box_candidates(targets[:, 1:5].T * gain, new.T)
    targets, new = targets[keep], new[keep]
    out = np.zeros((len(targets), 5))
    out[:, 0] = targets[:, 0]
    out[:, 1] = ((new[:, 0] + new[:, 2]) / 2) / W                               # xyxy2xywhn
    out[:, 2] = ((new[:, 1] + new[:, 3]) / 2) / H
    out[:, 3] = (new[:, 2] - new[:, 0]) / W
    out[:, 4] = (new[:, 3] - new[:, 1]) / H
    return out


def targets_of(rows, fliplr, flipud, max_boxes):
    """Normalised (cls, xc, yc, w, h) rows -> DetectDataset's (max_boxes, 6) boxes (xc, yc, w, h, cls, 255): the flips, then the fill;
    rows past max_boxes are dropped."""
    rows = np.array(rows, np.float64).reshape(-1, 5)
    if fliplr:
        rows[:, 1] = 1 - rows[:, 1]
    if flipud:
        rows[:, 2] = 1 - rows[:, 2]
    out = np.zeros((max_boxes, 6))
    m = min(len(rows), max_boxes)
    out[:m, 0:4] = rows[:m, 1:5]
    out[:m, 4] = rows[:m, 0]
    out[:m, 5] = 255.0
    return out
