"""tests/warp_ref.py (the numpy restatement that pins warp_kernel) against Pillow itself, byte for byte: gray and 3-channel images,
AFFINE and PERSPECTIVE, identity, a pure half-pixel shift, and a map that lands wholly outside the image."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_ref  # noqa: E402

SIZES = [(7, 9), (33, 47), (256, 320)]


def _image(h, w, c, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    img[: h // 3] = (np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)[None, :, None]     # a ramp above the noise
    return img if c == 3 else img[:, :, 0]


def _matrix(h, w, perspective, degrees=10.0, gain=1.1, shear=(5.0, -3.0), shift=(0.04, -0.03)):
    """A forward map of the kind DetectDataset draws: rotation, gain, shear and translation about the centre (+ a perspective row)."""
    C = np.eye(3); C[0, 2], C[1, 2] = -w / 2, -h / 2
    P = np.eye(3)
    if perspective:
        P[2, 0], P[2, 1] = 0.12 / w, -0.08 / h
    a = math.radians(degrees)
    R = np.eye(3); R[:2, :2] = [[gain * math.cos(a), gain * math.sin(a)], [-gain * math.sin(a), gain * math.cos(a)]]
    S = np.eye(3); S[0, 1], S[1, 0] = math.tan(math.radians(shear[0])), math.tan(math.radians(shear[1]))
    T = np.eye(3); T[0, 2], T[1, 2] = (0.5 + shift[0]) * w, (0.5 + shift[1]) * h
    return T @ S @ R @ P @ C


def _cases(h, w):
    ident = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0])
    half = np.array([1.0, 0, 0.5, 0, 1.0, -0.5, 0, 0])
    out = [("identity", ident, False), ("identity-as-perspective", ident, True), ("half-pixel", half, False), ("half-pixel-p", half, True)]
    for persp in (False, True):
        for name, kw in (("rot", {}), ("shrink", dict(degrees=-7.5, gain=0.8, shear=(0.0, 2.0), shift=(-0.05, 0.02))),
                         ("grow", dict(degrees=3.0, gain=1.37, shear=(-4.0, 0.0), shift=(0.0, 0.0)))):
            c = warp_ref.coeffs_of(_matrix(h, w, persp, **kw))
            if not persp:
                c[6:] = 0.0
            out.append((name + ("-p" if persp else "-a"), c, persp))
    return out


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_restatement_equals_pillow(size, channels):
    h, w = size
    img = _image(h, w, channels, h * 7 + channels)
    white = np.full(img.shape, 255, np.uint8)
    for name, c, persp in _cases(h, w):
        want = warp_ref.pil_transform_u8(img, c, persp)
        got = warp_ref.transform_u8(img, c, persp)
        assert got.shape == want.shape == img.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (name, size, channels, int((got != want).sum()))
        covered = warp_ref.pil_transform_u8(white, c, persp, fill=0) != 0          # the pixels Pillow sampled rather than filled
        assert covered.mean() >= 0.5, (name, size, float(covered.mean()))


def test_identity_and_half_pixel_shift_values():
    img = _image(33, 47, 1, 3)
    assert np.array_equal(warp_ref.transform_u8(img, [1, 0, 0, 0, 1, 0, 0, 0], False), img)
    got = warp_ref.transform_u8(img, [1, 0, 0.5, 0, 1, 0, 0, 0], False).astype(int)      # halfway between x and x + 1, truncated
    a = img.astype(int)
    want = np.concatenate([(a[:, :-1] + a[:, 1:]) // 2, np.full((33, 1), warp_ref.FILL)], axis=1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("perspective", [False, True])
def test_map_wholly_outside_is_all_fill(perspective, channels):
    for h, w in SIZES:
        img = _image(h, w, channels, 11)
        c = np.array([1.0, 0, 2.0 * w, 0, 1.0, -3.0 * h, 1e-4 if perspective else 0.0, 0.0])
        want = warp_ref.pil_transform_u8(img, c, perspective)
        assert (want == warp_ref.FILL).all()
        assert np.array_equal(warp_ref.transform_u8(img, c, perspective), want)


def test_output_size_other_than_the_input():
    img = _image(33, 47, 3, 5)
    c = warp_ref.coeffs_of(_matrix(33, 47, True))
    assert np.array_equal(warp_ref.transform_u8(img, c, True, size=(20, 61)), warp_ref.pil_transform_u8(img, c, True, size=(20, 61)))
