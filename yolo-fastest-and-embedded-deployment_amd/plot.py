"""`plot_one_box` -- the reference's box + label drawing (src/model_training/utils/general.py:56-67) without OpenCV.

Same signature and geometry: rectangle c1-c2 with `line_thickness` (default round(0.002 * (h + w) / 2) + 1), a FILLED label
box from c1 to (c1.x + text_w, c1.y - text_h - 3) and the label text at (c1.x, c1.y - 2) in [225, 255, 255].
The reference hands cv2 a BGR image, BGR colours, and cv2.imwrite stores what a viewer sees as RGB; here `img` is an RGB numpy
array (PIL decode), so a colour given in the reference's order is reversed before drawing -- the saved file shows the same
colours as the reference's result images (tests/golden/golden_results.npz holds samples of those).  What cannot be
reproduced without cv2 is the glyph rasterisation (Hershey simplex at scale tl/5): PIL's built-in font is used at the height
cv2.getTextSize reports for that scale (~22 * scale px)."""
import numpy as np


def plot_one_box(xyxy, img, color=None, label=None, line_thickness=None):
    """Draws in place on `img` (uint8 RGB [h,w,3], C-contiguous) and returns it."""
    from PIL import Image, ImageDraw, ImageFont
    tl = line_thickness or round(0.002 * (img.shape[0] + img.shape[1]) / 2) + 1
    if color is None:
        import random
        color = [random.randint(0, 255) for _ in range(3)]
    rgb = tuple(int(c) for c in reversed(color))          # the reference's colours are BGR
    c1, c2 = (int(xyxy[0]), int(xyxy[1])), (int(xyxy[2]), int(xyxy[3]))
    im = Image.fromarray(img)
    d = ImageDraw.Draw(im)
    # cv2.rectangle(thickness=tl) strokes a line of width tl CENTRED on the rectangle's edges
    lo, hi = tl // 2, tl - 1 - tl // 2
    x1, x2 = min(c1[0], c2[0]), max(c1[0], c2[0])
    y1, y2 = min(c1[1], c2[1]), max(c1[1], c2[1])
    for (a, b, c, e) in ((x1 - lo, y1 - lo, x2 + hi, y1 + hi), (x1 - lo, y2 - lo, x2 + hi, y2 + hi),
                         (x1 - lo, y1 - lo, x1 + hi, y2 + hi), (x2 - lo, y1 - lo, x2 + hi, y2 + hi)):
        d.rectangle([a, b, c, e], fill=rgb)
    if label:
        scale = tl / 5.0
        th = max(int(round(22 * scale)), 6)                # cv2.getTextSize(FONT_HERSHEY_SIMPLEX, scale)[0][1] ~ 22 * scale
        try:
            font = ImageFont.load_default(size=th + 2)
        except TypeError:                                  # older Pillow: fixed-size bitmap font
            font = ImageFont.load_default()
        l, t, r, b = d.textbbox((0, 0), label, font=font)
        tw = r - l
        lc2 = (c1[0] + tw, c1[1] - th - 3)
        d.rectangle([c1[0], lc2[1], lc2[0], c1[1]], fill=rgb)
        d.text((c1[0], c1[1] - 2 - th - t), label, fill=(255, 255, 225), font=font)   # [225, 255, 255] BGR
    img[...] = np.asarray(im)
    return img


# ---- the same drawing on device frames (csrc/yf_jpeg_enc_kernels.hip: draw_boxes_kernel) ----

TEXT_INK = (255, 255, 225)                                 # RGB; [225, 255, 255] in the reference's BGR


def default_thickness(h, w):
    return round(0.002 * (h + w) / 2) + 1


def label_mask(label, tl):
    """What plot_one_box's `d.text` lays over the image for `label` at line thickness `tl`, rendered once by PIL with the same font:
    (mask uint8 [mh, mw] coverage, ox, oy, tw, th).  The mask's top-left pixel lands on (c1.x + ox, c1.y + oy); the filled label box is
    [c1.x, c1.y - th - 3, c1.x + tw, c1.y]."""
    from PIL import Image, ImageDraw, ImageFont
    scale = tl / 5.0
    th = max(int(round(22 * scale)), 6)
    try:
        font = ImageFont.load_default(size=th + 2)
    except TypeError:
        font = ImageFont.load_default()
    probe = ImageDraw.Draw(Image.new("RGB", (1, 1)))       # plot_one_box measures on an RGB image
    l, t, r, b = probe.textbbox((0, 0), label, font=font)
    tw = r - l
    c1 = (8, th + 8)
    im = Image.new("L", (int(r) + 24, c1[1] + int(b - t) + 16), 0)
    ImageDraw.Draw(im).text((c1[0], c1[1] - 2 - th - t), label, fill=255, font=font)   # over black, ink 255: the blend returns the mask
    a = np.asarray(im)
    ys, xs = np.nonzero(a)
    if len(ys) == 0:
        return np.zeros((0, 0), np.uint8), 0, 0, tw, th
    y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
    assert 0 < x0 and x1 < a.shape[1] and 0 < y0 and y1 < a.shape[0], "label rendered outside its canvas"
    return np.ascontiguousarray(a[y0:y1, x0:x1]), int(x0) - c1[0], int(y0) - c1[1], tw, th


def box_record(xyxy, h, w, color, mask, tl, order, atlas_offset):
    """The 32 int32 of one yf_draw_boxes_u8 record: plot_one_box's five rectangles clipped to h x w, colour, ink, label mask placement."""
    rgb = tuple(int(c) for c in reversed(color))
    c1, c2 = (int(xyxy[0]), int(xyxy[1])), (int(xyxy[2]), int(xyxy[3]))
    lo, hi = tl // 2, tl - 1 - tl // 2
    x1, x2 = min(c1[0], c2[0]), max(c1[0], c2[0])
    y1, y2 = min(c1[1], c2[1]), max(c1[1], c2[1])
    rects = [(x1 - lo, y1 - lo, x2 + hi, y1 + hi), (x1 - lo, y2 - lo, x2 + hi, y2 + hi), (x1 - lo, y1 - lo, x1 + hi, y2 + hi),
             (x2 - lo, y1 - lo, x2 + hi, y2 + hi)]
    text = [0, 0, 0, 0, 0]
    if mask is not None:
        m, ox, oy, tw, th = mask
        rects.append((c1[0], c1[1] - th - 3, c1[0] + tw, c1[1]))
        text = [c1[0] + ox, c1[1] + oy, m.shape[1], m.shape[0], atlas_offset]
    else:
        rects.append((0, 0, -1, -1))
    rec = []
    for a, b, c, e in rects:
        rec += [max(a, 0), max(b, 0), min(c, w - 1), min(e, h - 1)]
        if rec[-2] < rec[-4] or rec[-1] < rec[-3]:
            rec[-4:] = [0, 0, -1, -1]

    def pack(c):
        c = c if order == "rgb" else c[::-1]
        return c[0] | c[1] << 8 | c[2] << 16
    return rec + [pack(rgb), pack(TEXT_INK)] + text + [0] * 5


def draw_boxes_device(frames, boxes_per_frame, labels_per_frame, colors, line_thickness=None, order="rgb", cache=None):
    """plot_one_box for every box of every frame of a batch in one launch, in place on uint8 device frames [n, h, w, 3] whose channels
    are in `order` ("rgb", or "bgr" as the device JPEG decoder hands frames out): bit for bit what the host function draws on the RGB
    frame when called per box in the same order.  boxes_per_frame[f]: xyxy per box; labels_per_frame[f]: a string or None per box (or
    None for no labels); colors[f]: the reference's BGR colour per box.  Label text is rendered by PIL on the host, once per distinct
    string and thickness (`cache`, a dict, keeps the masks between calls).  Stream-ordered; returns `frames`."""
    import ctypes

    import torch

    from . import _lib
    if not torch.is_tensor(frames) or not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 \
            or not frames.is_contiguous():
        raise ValueError("expected a contiguous uint8 GPU tensor [n, h, w, 3]")
    if order not in ("rgb", "bgr"):
        raise ValueError('order must be "rgb" or "bgr"')
    n, h, w = frames.shape[:3]
    if len(boxes_per_frame) != n or len(colors) != n or (labels_per_frame is not None and len(labels_per_frame) != n):
        raise ValueError("one list of boxes, labels and colours per frame")
    tl = line_thickness or default_thickness(h, w)
    cache = {} if cache is None else cache
    begin, recs, atlas, placed, used = [0], [], [], {}, 0
    for f in range(n):
        for k, xyxy in enumerate(boxes_per_frame[f]):
            label = labels_per_frame[f][k] if labels_per_frame is not None and labels_per_frame[f] is not None else None
            mask, off = None, 0
            if label:
                key = (label, tl)
                if key not in cache:
                    cache[key] = label_mask(label, tl)
                mask = cache[key]
                if key not in placed:
                    placed[key] = used
                    atlas.append(mask[0].reshape(-1))
                    used += mask[0].size
                off = placed[key]
            recs.append(box_record(xyxy, h, w, colors[f][k], mask, tl, order, off))
        begin.append(len(recs))
    if not recs:
        return frames
    dev = frames.device
    host = np.concatenate([np.asarray(begin, np.int32), np.asarray(recs, np.int32).reshape(-1)])
    table = torch.from_numpy(host).to(dev, non_blocking=True)
    d_atlas = torch.from_numpy(np.concatenate(atlas + [np.zeros(4, np.uint8)])).to(dev, non_blocking=True)
    stream = torch.cuda.current_stream(dev)
    _lib.check(_lib.lib().yf_draw_boxes_u8(dev.index, ctypes.c_void_p(frames.data_ptr()), n, h, w, ctypes.c_void_p(table.data_ptr()),
                                           ctypes.c_void_p(table.data_ptr() + 4 * (n + 1)), ctypes.c_void_p(d_atlas.data_ptr()),
                                           ctypes.c_void_p(stream.cuda_stream)))
    table.record_stream(stream)
    d_atlas.record_stream(stream)
    return frames
