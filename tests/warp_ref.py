"""TEST INFRASTRUCTURE: numpy restatement of Pillow's `Image.transform(size, AFFINE | PERSPECTIVE, data, resample=BILINEAR,
fillcolor=fill)` for uint8 images, the yardstick of warp_kernel (csrc/yf_aug_kernels.hip, yf_augment_warp_u8), and the composition that
kernel computes.  Pinned to Pillow; OpenCV parity not claimed (cv2.warpAffine / warpPerspective use fixed-point tables).

Pillow's arithmetic (src/libImaging/Geometry.c: affine_transform / perspective_transform, bilinear_filter8 / bilinear_filter32RGB) is
plain IEEE double arithmetic, one rounding per operation, which numpy's float64 element-wise operations reproduce.  Per output pixel
(x, y), with the eight coefficients a0 .. a7 of the output -> input map:
    xin = x + 0.5, yin = y + 0.5
    sx = (a0 * xin + a1 * yin) + a2, sy = (a3 * xin + a4 * yin) + a5; PERSPECTIVE: each divided by (a6 * xin + a7 * yin) + 1.0
    fill if sx < 0, sx >= W, sy < 0 or sy >= H; otherwise sx -= 0.5, sy -= 0.5, x0 = floor(sx), y0 = floor(sy), dx = sx - x0, dy = sy - y0,
    columns x0 and x0 + 1 and row y0 clamped to the image: v1 = a + (b - a) * dx on row y0, v2 the same on row y0 + 1 if that row exists,
    else v2 = v1; v = v1 + (v2 - v1) * dy, stored as (uint8)v (a truncation)."""
import numpy as np

FILL = 114     # yolov5's border value; every channel


def transform_u8(img, coeffs, perspective, fill=FILL, size=None):
    """img uint8 [h, w] or [h, w, c]; coeffs: 8 float64 (a6, a7 are not read unless `perspective`) -> uint8 of `size` (h, w), default img's."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    a = np.asarray(coeffs, np.float64)
    H, W = img.shape[:2]
    oh, ow = size if size is not None else (H, W)
    yin, xin = np.meshgrid(np.arange(oh, dtype=np.float64) + 0.5, np.arange(ow, dtype=np.float64) + 0.5, indexing="ij")
    sx = (a[0] * xin + a[1] * yin) + a[2]
    sy = (a[3] * xin + a[4] * yin) + a[5]
    if perspective:
        sx = sx / ((a[6] * xin + a[7] * yin) + 1.0)
        sy = sy / ((a[6] * xin + a[7] * yin) + 1.0)
    inside = ~((sx < 0.0) | (sx >= W) | (sy < 0.0) | (sy >= H))
    sx = np.where(inside, sx, 0.5) - 0.5
    sy = np.where(inside, sy, 0.5) - 0.5
    x0 = np.floor(sx)
    y0 = np.floor(sy)
    dx = sx - x0
    dy = sy - y0
    x0 = x0.astype(np.int64)
    y0 = y0.astype(np.int64)
    xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    ya = np.clip(y0, 0, H - 1)
    below = (y0 + 1 >= 0) & (y0 + 1 < H)
    yb = np.where(below, y0 + 1, 0)
    px = img.astype(np.float64)
    if px.ndim == 3:
        dx, dy, below_, inside_ = dx[..., None], dy[..., None], below[..., None], inside[..., None]
    else:
        below_, inside_ = below, inside
    v1 = px[ya, xa] + (px[ya, xb] - px[ya, xa]) * dx
    v2 = np.where(below_, px[yb, xa] + (px[yb, xb] - px[yb, xa]) * dx, v1)
    v = v1 + (v2 - v1) * dy
    return np.where(inside_, v.astype(np.uint8), np.uint8(fill)).astype(np.uint8)


def pil_transform_u8(img, coeffs, perspective, fill=FILL, size=None):
    """The same through Pillow itself."""
    from PIL import Image
    img = np.asarray(img)
    oh, ow = size if size is not None else img.shape[:2]
    im = Image.fromarray(img if img.ndim == 2 or img.shape[2] == 3 else img[:, :, 0])
    c = [float(v) for v in coeffs]
    out = im.transform((ow, oh), Image.Transform.PERSPECTIVE if perspective else Image.Transform.AFFINE, c if perspective else c[:6],
                       resample=Image.Resampling.BILINEAR, fillcolor=fill if img.ndim == 2 or img.shape[2] == 1 else (fill,) * 3)
    return np.asarray(out).reshape((oh, ow) + img.shape[2:])


def compose_u8(resized, coeffs, perspective, k, fliplr, flipud, transform=transform_u8):
    """What yf_augment_warp_u8 makes of one resized (and gray) uint8 frame [H, W, C]: flipud(fliplr(blur_k(transform(resized)))).
    coeffs None: no warp.  `transform`: this file's restatement or pil_transform_u8."""
    import aug_ref
    img = np.asarray(resized)
    if coeffs is not None:
        img = transform(img, coeffs, perspective)
    img = aug_ref.gaussian_blur_u8(np.ascontiguousarray(img), k)
    if fliplr:
        img = img[:, ::-1]
    if flipud:
        img = img[::-1]
    return np.ascontiguousarray(img)


def coeffs_of(M):
    """The eight coefficients of the output -> input map of a forward 3 x 3 matrix M (continuous pixel coordinates)."""
    inv = np.linalg.inv(np.asarray(M, np.float64))
    return (inv / inv[2, 2]).reshape(9)[:8].copy()
