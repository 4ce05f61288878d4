"""JPEG test inputs made at test time with PIL (nothing committed): the seeded image contents, the encoder settings of the device decoder's
test matrix, and the corruptions of tests/test_gpu_jpeg.py."""
import contextlib
import io

import numpy as np
from PIL import Image, ImageFile

SIZES = [(1, 1), (8, 8), (7, 9), (17, 33), (64, 48), (640, 512), (801, 603)]      # (w, h)
LAYOUTS = ["gray", "444", "422", "420"]
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


@contextlib.contextmanager
def big_encoder_buffer():
    """PIL sizes the buffer of an optimize / progressive encode by w * h (2 w h at quality >= 95), too small for 4:4:4 noise at quality
    100 ("Suspension not allowed here"): room for any such file while inside."""
    orig = ImageFile._save

    def _save(im, fp, tile, bufsize=0):
        return orig(im, fp, tile, max(bufsize, 8 * im.size[0] * im.size[1] + 65536))
    ImageFile._save = _save
    try:
        yield
    finally:
        ImageFile._save = orig


def image(content, w, h, rng):
    """uint8 [h, w, 3]: 'noise' (uniform) or 'smooth' (gradients)."""
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 127 // max(w + h - 2, 1)], 2).astype(np.uint8)


def encode(a, layout, **kw):
    """JPEG bytes of `a` in `layout` (gray: channel 0 as an L image; 444 / 422 / 420: RGB with that chroma subsampling)."""
    im = Image.fromarray(np.ascontiguousarray(a[:, :, 0])) if layout == "gray" else Image.fromarray(a)
    if layout != "gray":
        kw["subsampling"] = SUBSAMPLING[layout]
    b = io.BytesIO()
    with big_encoder_buffer():
        im.save(b, "JPEG", **kw)
    return b.getvalue()


def settings():
    """quality {10, 75, 100} x optimize {off, on} x restart markers {none, every block, every MCU row}: 18 encoder settings."""
    out = []
    for q in (10, 75, 100):
        for opt in (False, True):
            for rst in (None, "block", "row"):
                kw = dict(quality=q, optimize=opt)
                if rst == "block":
                    kw["restart_marker_blocks"] = 1
                elif rst == "row":
                    kw["restart_marker_rows"] = 1
                out.append(kw)
    return out


def scan_start(d):
    """Offset of the first entropy-coded byte (after the SOS segment)."""
    sos = d.find(b"\xff\xda")
    return sos + 2 + ((d[sos + 2] << 8) | d[sos + 3])


def sof_start(d):
    for m in (b"\xff\xc0", b"\xff\xc1"):
        k = d.find(m)
        if k >= 0:
            return k
    raise ValueError("no SOF0 / SOF1")


def truncated(d):
    """The file cut in the middle of its scan (no EOI)."""
    s0 = scan_start(d)
    return d[:s0 + (len(d) - s0) // 2]


def altered(d):
    """128 bytes in the middle of the scan replaced by stuffed 0xFF bytes: 512 one-bits, where every 16-bit window is the all-ones code
    that no JPEG Huffman table has (the standard reserves it), so decoding must meet a bad code there."""
    s0 = scan_start(d)
    mid = s0 + (len(d) - s0) // 2
    return d[:mid] + b"\xff\x00" * 64 + d[mid + 128:]


def pil_bgr(d):
    """What DetectDataset._decode / Detect_YOLO._read_bgr return for these bytes."""
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[:, :, ::-1])
