"""The host half of the device JPEG decoder (csrc/yf_jpeg_kernels.hip, yolo_fastest_amd/jpeg.py): what yf_jpeg_pack accepts and refuses,
the component geometry it derives and the Huffman lookup tables it builds.  No GPU needed; inputs are made here with PIL."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_gen as jg  # noqa: E402
from yolo_fastest_amd import _lib, jpeg  # noqa: E402


def info(blob, frame=0):
    a = (ctypes.c_int * 25)()
    _lib.check(_lib.lib().yf_jpeg_frame_info(ctypes.c_void_p(blob.data_ptr()), frame, a, 25))
    return list(a)


def smooth(w, h):
    return jg.image("smooth", w, h, None)


@pytest.mark.parametrize("layout,kw", [("gray", {}), ("444", {}), ("422", {}), ("420", {}), ("420", {"optimize": True}),
                                       ("420", {"restart_marker_blocks": 1}), ("gray", {"restart_marker_rows": 1}),
                                       ("422", {"restart_marker_rows": 2})])
def test_pack_accepts_the_supported_layouts(layout, kw):
    d = jg.encode(smooth(40, 24), layout, **kw)
    blob, h, w = jpeg.pack([d], pin=False)
    assert (h, w) == (24, 40)
    i = info(blob)
    assert i[0] == (1 if layout == "gray" else 3)
    assert i[1] == (0 if layout == "gray" else 1)            # JFIF: YCbCr
    if "restart_marker_blocks" in kw:
        assert i[6] == 1
    if "restart_marker_rows" in kw:
        assert i[6] == kw["restart_marker_rows"] * i[2]       # rows of MCUs
    assert jpeg.workspace_bytes(blob) > 0


def test_pack_refuses_progressive_cmyk_and_a_truncated_sof():
    from PIL import Image
    import io
    d = jg.encode(smooth(32, 32), "420", progressive=True)
    with pytest.raises(ValueError, match=r"<bytes #0>: progressive JPEG \(SOF2\) is not supported"):
        jpeg.pack([d], pin=False)
    b = io.BytesIO()
    Image.fromarray(smooth(32, 32)).convert("CMYK").save(b, "JPEG")
    with pytest.raises(ValueError, match=r"4-component \(CMYK / YCCK\) files are not supported"):
        jpeg.pack([b.getvalue()], pin=False)
    d = jg.encode(smooth(32, 32), "420")
    cut = d[:jg.sof_start(d) + 9]
    with pytest.raises(ValueError, match=r"SOF0 segment runs past the end of the file"):
        jpeg.pack([cut], pin=False)
    # the frame index of the refusal is named; frames of two sizes cannot share one blob
    good = jg.encode(smooth(32, 32), "gray")
    with pytest.raises(ValueError, match=r"<bytes #1>: progressive"):
        jpeg.pack([good, jg.encode(smooth(32, 32), "gray", progressive=True)], pin=False)
    with pytest.raises(ValueError, match=r"differs from frame 0"):
        jpeg.pack([good, jg.encode(smooth(16, 32), "gray")], pin=False)


def test_frame_size_names_the_file(tmp_path):
    p = tmp_path / "p.jpg"
    p.write_bytes(jg.encode(smooth(16, 16), "444", progressive=True))
    with pytest.raises(ValueError, match="p.jpg: progressive"):
        jpeg.frame_size(p.read_bytes(), str(p))
    assert jpeg.frame_size(jg.encode(smooth(17, 9), "420")) == (9, 17)


def ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize("w,h", [(1, 1), (7, 9), (17, 33), (640, 512), (801, 603)])
@pytest.mark.parametrize("layout", jg.LAYOUTS + ["440"])
def test_blocks_per_component_and_mcu_count(w, h, layout):
    from PIL import Image
    import io
    if layout == "440":          # luma 1 x 2: PIL cannot write it; patch the sampling bytes of a 4:4:4 file (the scan is not decoded here)
        d = bytearray(jg.encode(smooth(w, h), "444"))
        s = jg.sof_start(d)
        d[s + 11] = 0x12
        d = bytes(d)
        hs, vs = 1, 2
    else:
        d = jg.encode(smooth(w, h), layout)
        hs, vs = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}[layout]
    blob, _, _ = jpeg.pack([d], pin=False)
    i = info(blob)
    if layout == "gray":
        mx, my = ceil(w, 8), ceil(h, 8)
        assert i[:6] == [1, 0, mx, my, mx * my, 1]
        assert i[7:13] == [1, 1, mx, my, w, h] and i[13:] == [0] * 12
        return
    mx, my = ceil(w, 8 * hs), ceil(h, 8 * vs)
    assert i[:6] == [3, 1, mx, my, mx * my, hs * vs + 2]
    assert i[7:13] == [hs, vs, mx * hs, my * vs, w, h]
    for c in (1, 2):
        assert i[7 + 6 * c:13 + 6 * c] == [1, 1, mx, my, ceil(w, hs), ceil(h, vs)]
    assert Image.open(io.BytesIO(d)).size == (w, h)


def dht_tables(d):
    """(class, id, [(length, code, symbol)]) of every DHT table in the file, canonical codes as the standard assigns them."""
    out, i = [], 2
    while i < len(d):
        assert d[i] == 0xFF
        m = d[i + 1]
        if m == 0xDA:
            break
        ln = (d[i + 2] << 8) | d[i + 3]
        if m == 0xC4:
            k = i + 4
            while k < i + 2 + ln:
                tc, th = d[k] >> 4, d[k] & 15
                bits = list(d[k + 1:k + 17])
                vals = list(d[k + 17:k + 17 + sum(bits)])
                codes, code, p = [], 0, 0
                for length in range(1, 17):
                    for _ in range(bits[length - 1]):
                        codes.append((length, code, vals[p]))
                        code += 1
                        p += 1
                    code <<= 1
                out.append((tc, th, codes))
                k += 17 + sum(bits)
        i += 2 + ln
    return out


@pytest.mark.parametrize("layout,kw", [("420", {}), ("420", {"optimize": True, "quality": 100}), ("gray", {"optimize": True}),
                                       ("444", {"optimize": True, "quality": 10})])
def test_every_huffman_code_looks_up_to_its_length_and_symbol(layout, kw):
    rng = np.random.default_rng(5)
    d = jg.encode(jg.image("noise", 96, 64, rng), layout, **kw)
    blob, _, _ = jpeg.pack([d], pin=False)
    lib = _lib.lib()
    tables = dht_tables(d)
    assert len(tables) >= (2 if layout == "gray" else 4)
    length, sym = ctypes.c_int(), ctypes.c_int()
    longest = 0
    for tc, th, codes in tables:
        for ln, code, s in codes:
            for tail in (0, (1 << (16 - ln)) - 1):               # whatever follows the code in the 16-bit window
                window = (code << (16 - ln)) | tail
                _lib.check(lib.yf_jpeg_huff_lookup(ctypes.c_void_p(blob.data_ptr()), 0, tc * 4 + th, window, ctypes.byref(length),
                                                   ctypes.byref(sym)))
                assert (length.value, sym.value) == (ln, s), (tc, th, ln, code, s)
            longest = max(longest, ln)
        # the all-ones window is no code
        _lib.check(lib.yf_jpeg_huff_lookup(ctypes.c_void_p(blob.data_ptr()), 0, tc * 4 + th, 0xFFFF, ctypes.byref(length), ctypes.byref(sym)))
        assert length.value == 0
    assert longest > 9                                             # the maxcode / valoffset path was exercised too
