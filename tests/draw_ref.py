"""`plot.plot_one_box` restated in numpy (test infrastructure): integer rectangles clipped to the image and the label's coverage mask
blended with PIL's 8-bit arithmetic.  The mask is an input (`plot.label_mask` renders it with PIL; glyph rasterisation is not restated).
tests/test_cpu_draw.py holds it to plot_one_box itself and the blend to the installed Pillow, exhaustively."""
import numpy as np

INK = (255, 255, 225)


def blend(dst, ink, mask):
    """ImagingFill2 / fill_mask_L of the installed Pillow: one rounding of the whole sum, not one per product."""
    t = np.asarray(dst, np.int64) * (255 - np.asarray(mask, np.int64)) + int(ink) * np.asarray(mask, np.int64) + 128
    return ((t >> 8) + t) >> 8


def fill(img, a, b, c, e, rgb):
    """ImageDraw.rectangle([a, b, c, e], fill=rgb): corners inclusive, clipped."""
    h, w = img.shape[:2]
    x0, y0, x1, y1 = max(a, 0), max(b, 0), min(c, w - 1), min(e, h - 1)
    if x0 <= x1 and y0 <= y1:
        img[y0:y1 + 1, x0:x1 + 1] = rgb


def plot_one_box(xyxy, img, color, mask=None, line_thickness=None):
    """In place on `img` (uint8 RGB [h, w, 3]); `mask` = plot.label_mask(label, tl) or None."""
    h, w = img.shape[:2]
    tl = line_thickness or round(0.002 * (h + w) / 2) + 1
    rgb = tuple(int(c) for c in reversed(color))
    c1, c2 = (int(xyxy[0]), int(xyxy[1])), (int(xyxy[2]), int(xyxy[3]))
    lo, hi = tl // 2, tl - 1 - tl // 2
    x1, x2 = min(c1[0], c2[0]), max(c1[0], c2[0])
    y1, y2 = min(c1[1], c2[1]), max(c1[1], c2[1])
    fill(img, x1 - lo, y1 - lo, x2 + hi, y1 + hi, rgb)
    fill(img, x1 - lo, y2 - lo, x2 + hi, y2 + hi, rgb)
    fill(img, x1 - lo, y1 - lo, x1 + hi, y2 + hi, rgb)
    fill(img, x2 - lo, y1 - lo, x2 + hi, y2 + hi, rgb)
    if mask is not None:
        m, ox, oy, tw, th = mask
        fill(img, c1[0], c1[1] - th - 3, c1[0] + tw, c1[1], rgb)
        X, Y = c1[0] + ox, c1[1] + oy
        x0, y0, x1, y1 = max(X, 0), max(Y, 0), min(X + m.shape[1], w), min(Y + m.shape[0], h)
        if x0 < x1 and y0 < y1:
            mm = m[y0 - Y:y1 - Y, x0 - X:x1 - X]
            for ch in range(3):
                img[y0:y1, x0:x1, ch] = blend(img[y0:y1, x0:x1, ch], INK[ch], mm)
    return img
