"""TEST INFRASTRUCTURE: yolov5's mixup on uint8 frames, the yardstick of mix_kernel (csrc/yf_aug_kernels.hip, yf_augment_mix_u8), and the
composition that kernel computes: flipud(fliplr(blur_k(mix))) with
    mix = (A * r + B * (1 - r)).astype(np.uint8)        A, B uint8 arrays, r a Python float: yolov5's own expression, in numpy
    A, B = warp_ref.pil_transform_u8(resized, coeffs, persp) each, or the resized frame itself; without a partner mix = A
numpy evaluates the expression element-wise in float64 with one rounding per operation (two products, one sum; 1 - r once, in Python),
and the conversion truncates: what the kernel has to reproduce without an FMA or a rearrangement."""
import numpy as np

import aug_ref
import warp_ref


def mix_u8(a, b, r):
    """yolov5's utils/augmentations.py mixup on the pixels: `(im * r + im2 * (1 - r)).astype(np.uint8)`."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and isinstance(r, float)
    return (a * r + b * (1 - r)).astype(np.uint8)


def _is_persp(coeffs):
    return bool(coeffs[6] != 0 or coeffs[7] != 0)


def compose_u8(first, coeffs, second, second_coeffs, r, k, fliplr, flipud, transform=warp_ref.pil_transform_u8):
    """What yf_augment_mix_u8 makes of one output: `first` / `second` resized (and gray) uint8 frames [H, W, C], `second` None for no
    partner; coeffs None: that frame is not warped; a frame whose coefficients end in a non-zero a6 or a7 is a perspective one."""
    img = np.asarray(first)
    if coeffs is not None:
        img = transform(img, coeffs, _is_persp(coeffs))
    if second is not None:
        other = np.asarray(second)
        if second_coeffs is not None:
            other = transform(other, second_coeffs, _is_persp(second_coeffs))
        img = mix_u8(np.ascontiguousarray(img), np.ascontiguousarray(other), float(r))
    img = aug_ref.gaussian_blur_u8(np.ascontiguousarray(img), k)
    if fliplr:
        img = img[:, ::-1]
    if flipud:
        img = img[::-1]
    return np.ascontiguousarray(img)
