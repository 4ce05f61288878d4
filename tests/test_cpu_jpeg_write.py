"""tests/jpeg_write.py is a real encoder (PIL decodes every setting, close to the source and to Pillow's own encode), and the host half
of the device JPEG decoder on the streams it writes: libjpeg's colour-space guess, 4:4:0 geometry and every refusal with its message.
No GPU needed."""
import ctypes
import io
import itertools
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_gen as jg  # noqa: E402
import jpeg_write as jw  # noqa: E402
from yolo_fastest_amd import _lib, jpeg  # noqa: E402


def info(d):
    blob, _, _ = jpeg.pack([d], pin=False)
    a = (ctypes.c_int * 25)()
    _lib.check(_lib.lib().yf_jpeg_frame_info(ctypes.c_void_p(blob.data_ptr()), 0, a, 25))
    return list(a)


def pil_rgb(d):
    return np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))


def psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))


SETTINGS = [dict(), dict(huff="opt"), dict(huff="deep"), dict(q16=True), dict(qidx=[3, 2, 1], dcidx=[3, 1, 2], acidx=[3, 2, 1]),
            dict(dht="merged"), dict(redefine=True, dht="merged"), dict(ri=1, fill=1), dict(ri=5, fill=3, eoi_fill=2),
            dict(rgb=True, ids=[82, 71, 66], markers=(("adobe", 0),)), dict(markers=()), dict(ids=[7, 200, 0], markers=()),
            dict(extra=((0xFE, b"comment"), (0xE3, b"\x00" * 40)), trailing=b"\x00garbage"), dict(quality=5), dict(quality=100)]


@pytest.mark.parametrize("layout", jw.LAYOUTS)
@pytest.mark.parametrize("k", range(len(SETTINGS)))
def test_pil_decodes_every_setting(layout, k):
    a = jw.textured(37, 21, k)
    d = jw.encode(a, layout, **SETTINGS[k])
    im = Image.open(io.BytesIO(d))
    assert im.size == (37, 21)
    im.load()
    assert im.mode == ("L" if layout == "gray" else "RGB")
    got = np.asarray(im.convert("RGB"))
    ref = a if layout != "gray" else np.repeat(a[:, :, :1], 3, 2)
    assert psnr(got, ref) > (15 if SETTINGS[k].get("quality") == 5 else 24), (layout, SETTINGS[k])


@pytest.mark.parametrize("layout", ["gray", "444"])
@pytest.mark.parametrize("quality", [75, 90, 100])
def test_psnr_of_standard_tables(layout, quality):
    a = jw.textured(96, 64, quality)
    got = pil_rgb(jw.encode(a, layout, quality))
    ref = a if layout == "444" else np.repeat(a[:, :, :1], 3, 2)
    assert psnr(got, ref) >= 30, psnr(got, ref)


@pytest.mark.parametrize("layout,tol", [("gray", 2), ("444", 4), ("420", 6)])
@pytest.mark.parametrize("quality", [75, 90, 100])
def test_agrees_with_pillows_own_encode(layout, tol, quality):
    """The same image, quality and layout written by Pillow and by the writer: the gray decodes agree within +-2 levels.  Colour adds
    the difference of the source's colour conversion (float here, libjpeg's integer tables there) and of the chroma downsampling."""
    a = jg.image("smooth", 96, 64, None)
    ours = pil_rgb(jw.encode(a, layout, quality))
    theirs = pil_rgb(jg.encode(a, layout, quality=quality))
    assert int(np.abs(ours.astype(int) - theirs).max()) <= tol


def test_optimised_and_deep_tables():
    """K.2 tables decode like the standard ones; 'deep' counts make 16-bit codes (the limiter acts); a flat frame makes one-code tables."""
    a = jw.textured(64, 48, 1)
    std = pil_rgb(jw.encode(a, "420"))
    for huff in ("opt", "deep"):
        assert np.array_equal(pil_rgb(jw.encode(a, "420", huff=huff)), std)
    d = jw.encode(a, "420", huff="deep")
    longest = [max(i + 1 for i in range(16) if s[1 + i]) for m, s in jw._segments(d) if m == 0xC4]
    assert max(longest) == 16
    flat = jw.encode(np.full((16, 16, 3), 90, np.uint8), "gray", huff="opt")
    ac = [s for m, s in jw._segments(flat) if m == 0xC4 and s[0] == 0x10][0]
    assert list(ac[1:17]) == [1] + [0] * 15 and ac[17] == 0
    assert np.array_equal(pil_rgb(flat), np.full((16, 16, 3), 90, np.uint8))


# ------------------------------------------------------------------------------------------------ libjpeg's colour-space guess
def pil_took_rgb(a, d):
    """True if PIL's decode is the components unconverted (libjpeg guessed RGB), False if it converted them as YCbCr."""
    got = pil_rgb(d).astype(int)
    err = np.abs(got - a).max(), np.abs(got - a).mean()
    assert err[0] <= 8 or err[1] >= 20, err                          # clearly one or the other
    return bool(err[0] <= 8)


@pytest.mark.parametrize("markers,ids", jw.GUESS_CASES)
def test_colour_guess_matches_libjpeg(markers, ids):
    a, d = jw.colour_case(markers, ids)
    assert info(d)[1] == (2 if pil_took_rgb(a, d) else 1), (markers, ids)


@pytest.mark.parametrize("n", range(9, 17))
def test_short_jfif_segment_in_a_pillow_keep_rgb_file(n):
    """Pillow's keep_rgb file (Adobe transform 0, IDs R, G, B) with an APP0 "JFIF" segment of length n inserted: libjpeg counts it only
    from length 16 (14 bytes of data)."""
    a = jg.image("smooth", 40, 24, None)
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", keep_rgb=True, quality=95)
    d = b.getvalue()
    assert d[2:4] == b"\xff\xee"
    app0 = b"\xff\xe0" + n.to_bytes(2, "big") + (b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")[:n - 2]
    d2 = d[:2] + app0 + d[2:]
    took_rgb = pil_took_rgb(a, d2)
    assert took_rgb == (n < 16)
    assert info(d2)[1] == (2 if took_rgb else 1)
    if took_rgb:
        assert np.array_equal(pil_rgb(d2), pil_rgb(d))


# ------------------------------------------------------------------------------------------------ geometry of 4:4:0
def ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize("w,h", [(1, 1), (7, 9), (17, 33), (801, 603)])
def test_geometry_of_real_440_files(w, h):
    d = jw.encode(jg.image("smooth", w, h, None), "440")
    assert Image.open(io.BytesIO(d)).size == (w, h)
    i = info(d)
    mx, my = ceil(w, 8), ceil(h, 16)
    assert i[:7] == [3, 1, mx, my, mx * my, 4, 0]
    assert i[7:13] == [1, 2, mx, 2 * my, w, h]
    for c in (1, 2):
        assert i[7 + 6 * c:13 + 6 * c] == [1, 1, mx, my, w, ceil(h, 2)]


@pytest.mark.parametrize("ri", [1, 3, 64, 1000])
def test_restart_interval_and_count(ri):
    d = jw.encode(jg.image("smooth", 801, 603, None), "gray", ri=ri)
    i = info(d)
    assert i[6] == ri and i[4] == 101 * 76


# ------------------------------------------------------------------------------------------------ refusals
def replace_segment(d, marker, fn):
    """The file with the payload of its first `marker` segment replaced by fn(payload)."""
    i = 2
    while True:
        m, ln = d[i + 1], (d[i + 2] << 8) | d[i + 3]
        if m == marker:
            p = fn(bytearray(d[i + 4:i + 2 + ln]))
            return d[:i + 2] + (len(p) + 2).to_bytes(2, "big") + bytes(p) + d[i + 2 + ln:]
        i += 2 + ln


def patched(d, marker, at, value):
    def fn(p):
        p[at] = value
        return p
    return replace_segment(d, marker, fn)


def refused(d, msg):
    with pytest.raises(ValueError, match=r"<bytes #0>: " + msg):
        jpeg.pack([d], pin=False)


LAYOUT_MSG = r"unsupported sampling layout \(luma 1 or 2 in each direction, chroma 1 x 1\)"


def test_refusals_name_their_reason():
    a = jg.image("smooth", 40, 24, None)
    d444 = jw.encode(a, "444")
    two = replace_segment(d444, 0xC0, lambda p: p[:5] + bytes([2]) + p[6:12])
    refused(two, "only 1- or 3-component files are supported")
    for hv in (0x31, 0x13, 0x41, 0x14, 0x33):                        # luma sampling 3 or 4
        refused(patched(d444, 0xC0, 7, hv), LAYOUT_MSG)
    for c in (1, 2):                                                 # chroma not 1 x 1
        for hv in (0x21, 0x12, 0x22):
            refused(patched(d444, 0xC0, 7 + 3 * c, hv), LAYOUT_MSG)
    refused(replace_segment(d444, 0xC0, lambda p: p[:1] + b"\x00\x00" + p[3:]), r"image height 0 \(DNL-defined height\) is not supported")
    # the first scan holds one component of three: non-interleaved, several scans
    refused(replace_segment(d444, 0xDA, lambda p: bytes([1, 1, 0x00, 0, 63, 0])),
            r"the first scan does not hold every component \(multi-scan sequential files are not supported\)")
    for at, v in ((7, 1), (8, 62), (8, 0), (9, 0x10)):              # Ss, Se, Ah / Al
        refused(patched(d444, 0xDA, at, v), "scan is not a sequential full-spectrum scan")
    for dim in (1, 3):                                               # 8193 pixels high or wide
        refused(replace_segment(d444, 0xC0, lambda p: p[:dim] + (8193).to_bytes(2, "big") + p[dim + 2:]), "image larger than 8192 x 8192")


def test_refuses_bad_huffman_tables():
    d = jw.encode(jg.image("smooth", 40, 24, None), "gray")

    def dc_symbol_16(p):                                             # the DC table's last value (category 11) -> 16
        assert p[0] == 0x00
        p[17 + sum(p[1:17]) - 1] = 16
        return p

    def oversubscribed(p):                                           # three 1-bit codes, the same number of symbols
        n = sum(p[1:17])
        p[1:17] = bytes([3, 0, n - 3] + [0] * 13)
        return p
    refused(replace_segment(d, 0xC4, dc_symbol_16), "bad Huffman table")
    refused(replace_segment(d, 0xC4, oversubscribed), "bad Huffman table")
    refused(replace_segment(d, 0xC4, lambda p: bytes([0x04]) + p[1:]), r"bad DHT table class or index")


def test_largest_accepted_sizes():
    for w, h in ((8192, 8), (8, 8192)):
        for layout in ("gray", "420"):
            d = jw.encode(jg.image("smooth", w, h, None), layout)
            assert jpeg.frame_size(d) == (h, w)


def test_every_table_index_and_16_bit_dqt_pack():
    d = jw.encode(jg.image("smooth", 40, 24, None), "420", q16=True, qidx=[3, 0, 2], dcidx=[3, 1, 2], acidx=[3, 2, 1], dht="merged",
                  redefine=True)
    assert [m for m, _ in jw._segments(d) if m in (0xC0, 0xC1)] == [0xC1] and [s[0] >> 4 for m, s in jw._segments(d) if m == 0xDB] == [1]
    assert info(d)[:2] == [3, 1]
    for combo in itertools.product((0, 3), (1, 2)):
        d = jw.encode(jg.image("smooth", 16, 16, None), "444", dcidx=[combo[0], combo[1], combo[1]], acidx=[combo[1], combo[0], combo[0]])
        assert info(d)[0] == 3
