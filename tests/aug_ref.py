"""TEST INFRASTRUCTURE: numpy restatement of the image half of the reference's DetectDataset (dataloader/detect_dataset.py:90-162), the
yardstick of csrc/yf_aug_kernels.hip.  cvtColor / resize are oracle/cv_oracle.py's; this adds cv2.GaussianBlur(img, (k, k), 0) for
uint8 images and the composition the kernel computes.

GaussianBlur, 8-bit, sigma = 0, k <= 7 (OpenCV's fixed-point path, modules/imgproc/src/smooth.simd.hpp): the kernel is the small
Gaussian table as ufixedpoint16 (1/256 units), separable; the row pass sums exactly (at most 255 * 256 fits uint16), the column pass
multiplies those sums by the taps again (2^-16 units) and rounds half up: dst = (sum + 2^15) >> 16.  BORDER_REFLECT_101 on all sides
(the default), each channel on its own.  Parity with a real OpenCV build is UNPINNED: cv2 is not available where this was written."""
import numpy as np

TAPS = {3: (64, 128, 64), 5: (16, 64, 96, 64, 16), 7: (8, 28, 56, 72, 56, 28, 8)}


def reflect101(i, n):
    """cv::borderInterpolate(i, n, BORDER_REFLECT_101) for an int array i."""
    i = np.asarray(i, np.int64).copy()
    if n == 1:
        return np.zeros_like(i)
    while True:
        bad = (i < 0) | (i >= n)
        if not bad.any():
            return i
        i = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def gaussian_blur_u8(img, k):
    """cv2.GaussianBlur(img, (k, k), 0) for uint8 [h, w] or [h, w, c]; k = 0 returns a copy."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if k == 0:
        return img.copy()
    t = np.array(TAPS[k], np.int64)
    r = k // 2
    a = img.astype(np.int64)
    h, w = a.shape[:2]
    xs = reflect101(np.arange(-r, w + r), w)
    rows = sum(t[i] * a[:, xs[i:i + w]] for i in range(k))
    assert rows.max(initial=0) <= 0xFFFF                       # the row pass is exact in uint16
    ys = reflect101(np.arange(-r, h + r), h)
    out = (sum(t[j] * rows[ys[j:j + h]] for j in range(k)) + (1 << 15)) >> 16
    return out.astype(np.uint8)


def augment_u8(bgr, input_shape, k, flip, gray_bits=15, resize=True):
    """What the reference's load_rect + augmentation make of one cv2.imread frame (uint8 [h, w, 3], BGR), before `- 128.0`:
    cvtColor for a 1-channel net, cv2.resize to input_shape (`resize`: the reference's configured shapes differ), the blur, the flip.
    -> uint8 [H, W, C] (C = input_shape[2], channels still BGR)."""
    from oracle import cv_oracle as cv
    img = np.asarray(bgr)
    if input_shape[2] == 1 and img.ndim == 3 and img.shape[2] == 3:
        img = cv.cvt_bgr2gray(img, gray_bits)
    if resize:
        img = cv.resize_linear_u8(img, (input_shape[1], input_shape[0]))
    img = gaussian_blur_u8(img, k)
    if flip:
        img = np.fliplr(img)
    if img.ndim == 2:
        img = img[:, :, None]
    return np.ascontiguousarray(img)
