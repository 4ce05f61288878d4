"""tests/jpeg_enc_ref.py against the installed Pillow, byte for byte, and the host half of the device encoder (yf_jpeg_enc_setup: header
and tables) against both.  No GPU needed.  The yardstick is what PIL writes here: if a later Pillow / libjpeg writes other bytes, these
tests say so."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_enc_ref as ref  # noqa: E402
from yolo_fastest_amd import _lib, jpeg  # noqa: E402
from yolo_fastest_amd.plot import plot_one_box  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "test_data")
FILES = sorted(os.listdir(DATA))
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 16), (16, 17), (37, 53), (480, 640), (512, 640)]
QUALITIES = [1, 10, 25, 50, 75, 90, 95, 100]
SUBS = ["4:2:0", "4:2:2", "4:4:4"]
PATTERNS = ["noise", "flat0", "flat128", "flat255", "hramp", "vramp", "checker"]


def pil_bytes(a, quality, subsampling=None):
    b = io.BytesIO()
    kw = {} if subsampling is None else {"subsampling": subsampling}
    Image.fromarray(a).save(b, "JPEG", quality=quality, **kw)
    return b.getvalue()


def pattern(name, h, w, ch, seed=0):
    shape = (h, w, 3) if ch == 3 else (h, w)
    if name == "noise":
        return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    if name.startswith("flat"):
        return np.full(shape, int(name[4:]), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "hramp":
        p = xx * 255 // max(w - 1, 1)
    elif name == "vramp":
        p = yy * 255 // max(h - 1, 1)
    else:
        p = ((yy + xx) & 1) * 255
    p = p.astype(np.uint8)
    return np.stack([p, 255 - p, p], axis=2) if ch == 3 else p


def frame(name):
    return np.asarray(Image.open(os.path.join(DATA, name)).convert("RGB"))


@pytest.mark.parametrize("name", FILES)
def test_bundled_frames_as_the_result_writer_saves_them(name):
    a = frame(name)
    assert ref.encode(a, 95, "4:2:0") == pil_bytes(a, 95)                        # Detect_YOLO._save's arguments
    b = a.copy()
    rng = np.random.default_rng(len(name))
    for k in range(3):
        x, y = int(rng.integers(0, a.shape[1] - 60)), int(rng.integers(0, a.shape[0] - 60))
        plot_one_box([x, y, x + 50 + 40 * k, y + 40 + 30 * k], b, label="cloud 0.%d7" % k, color=[[106, 90, 205], [199, 97, 20], [112, 128, 105]][k],
                     line_thickness=3)
    assert not np.array_equal(a, b)
    assert ref.encode(b, 95, "4:2:0") == pil_bytes(b, 95)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("size", SIZES)
def test_every_padding_case_with_every_subsampling(size, sub):
    k = SIZES.index(size) + SUBS.index(sub)
    for j, q in enumerate((QUALITIES[k % 8], QUALITIES[(k + 3) % 8], 95)):
        a = pattern("noise", size[0], size[1], 3, seed=k + j)
        assert ref.encode(a, q, sub) == pil_bytes(a, q, sub), (size, sub, q)


@pytest.mark.parametrize("pat", PATTERNS)
@pytest.mark.parametrize("quality", QUALITIES)
def test_patterns_at_every_quality(pat, quality):
    for (h, w), sub in (((37, 53), SUBS[quality % 3]), ((16, 17), SUBS[(quality + 1) % 3]), ((64, 48), "4:2:0")):
        a = pattern(pat, h, w, 3, seed=quality)
        assert ref.encode(a, quality, sub) == pil_bytes(a, quality, sub), (pat, quality, h, w, sub)
    g = pattern(pat, 37, 53, 1, seed=quality)
    assert ref.encode(g, quality) == pil_bytes(g, quality)


@pytest.mark.parametrize("size", SIZES)
def test_gray_at_every_size(size):
    for q, pat in ((95, "noise"), (100, "checker"), (50, "hramp")):
        g = pattern(pat, size[0], size[1], 1, seed=size[0])
        assert ref.encode(g, q) == pil_bytes(g, q), (size, q, pat)


def test_default_subsampling_is_420_and_the_names_match_pils_numbers():
    a = pattern("noise", 17, 19, 3)
    assert pil_bytes(a, 95) == pil_bytes(a, 95, "4:2:0") == pil_bytes(a, 95, 2)
    assert pil_bytes(a, 95, "4:2:2") == pil_bytes(a, 95, 1) and pil_bytes(a, 95, "4:4:4") == pil_bytes(a, 95, 0)


def test_noise_at_quality_100_outgrows_the_first_reservation():
    """tests/test_gpu_jpeg_enc.py relies on it for the overflow case."""
    a = pattern("noise", 64, 64, 3)
    assert len(pil_bytes(a, 100, "4:4:4")) > 64 * 64 * 3 + 1024


# ---- yf_jpeg_enc_setup: host only ----

def split_header(d):
    """(bytes up to and including SOS, the quantisation tables in zig-zag order)"""
    i, q = 2, []
    while True:
        m, ln = d[i + 1], (d[i + 2] << 8) | d[i + 3]
        if m == 0xDB:
            q.append(list(d[i + 5:i + 69]))
        i += 2 + ln
        if m == 0xDA:
            return d[:i], q


@pytest.mark.parametrize("kind", SUBS + ["gray"])
def test_setup_blob_header_and_tables_equal_pils_for_every_quality(kind):
    for quality in range(1, 101):
        for h, w in ((17, 9), (512, 640)) if quality in (1, 95) else ((17, 9),):
            a = np.zeros((h, w) if kind == "gray" else (h, w, 3), np.uint8)
            want, q = split_header(pil_bytes(a, quality, None if kind == "gray" else kind))
            s = jpeg.enc_setup(h, w, 1 if kind == "gray" else 3, quality, "4:4:4" if kind == "gray" else kind)
            assert s.header == want, (kind, quality)
            assert want == ref.header(h, w, a.ndim if a.ndim == 3 else 1, quality, *ref.SUBSAMPLING["4:4:4" if kind == "gray" else kind])
            for t in range(len(q)):
                nat = np.empty(64, np.int64)
                nat[ref.ZIGZAG] = q[t]
                assert list(s.divisors[t]) == list(8 * nat), (kind, quality, t)
                # the reciprocals give the rounded division for every magnitude the DCT of 8-bit samples can reach
                v = np.arange(0, 1 << 15, dtype=np.uint64)[:, None]
                d = (8 * nat).astype(np.uint64)[None, :]
                got = ((v + (d >> np.uint64(1))) * np.asarray(s.reciprocals[t], np.uint64)[None, :]) >> np.uint64(32)
                assert np.array_equal(got, (v + (d >> np.uint64(1))) // d)


def test_setup_refuses_what_is_not_built():
    for args in ((0, 8, 3, 95, "4:2:0"), (8, 8193, 3, 95, "4:2:0"), (8, 8, 2, 95, "4:2:0"), (8, 8, 3, 0, "4:2:0"), (8, 8, 3, 101, "4:2:0"),
                 (8, 8, 3, 95, "4:1:1"), (8192, 8192, 3, 95, "4:4:4")):
        with pytest.raises(ValueError):
            jpeg.enc_setup(*args)
    assert jpeg.enc_setup(8192, 8192, 1, 95, "4:4:4").header[:2] == b"\xff\xd8"
    lib = _lib.lib()
    need = ctypes.c_size_t()
    assert lib.yf_jpeg_enc_setup(8, 8, 3, 95, 7, None, 0, ctypes.byref(need)) == _lib.YF_E_INVALID
    assert b"subsampling" in lib.yf_last_error_string()
