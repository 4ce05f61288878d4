"""The host half of progressive JPEG decoding (yf_jpeg_pack_ex / yf_jpeg_scan_info / yf_jpeg_huff_lookup_ex in csrc/yf_jpeg_kernels.hip,
`progressive=True` in yolo_fastest_amd/jpeg.py and both drivers): what the packer accepts, the scan scripts and dependency levels it
derives, every refusal with its reason, the per-scan Huffman lookups, and the test writer itself (tests/jpeg_write_prog.py) against PIL.
No GPU needed."""
import ctypes
import logging
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_gen as jg  # noqa: E402
import jpeg_write as jw  # noqa: E402
import jpeg_write_prog as jp  # noqa: E402
from yolo_fastest_amd import _lib, jpeg  # noqa: E402


def smooth(w, h):
    return jg.image("smooth", w, h, None)


def script_of(blob, frame=0):
    """[(component mask, Ss, Se, Ah, Al)] in file order, levels per scan, level count."""
    n = jpeg.scan_info(blob, frame)["scans"]
    infos = [jpeg.scan_info(blob, frame, s) for s in range(n)]
    return ([(i["comp_mask"], i["ss"], i["se"], i["ah"], i["al"]) for i in infos], [i["level"] for i in infos],
            infos[0]["levels"] if infos else 0)


def masks(script):
    return [(sum(1 << c for c in comps), ss, se, ah, al) for comps, ss, se, ah, al in script]


def test_flag_zero_is_yf_jpeg_pack():
    d = jg.encode(smooth(32, 32), "420", progressive=True)
    with pytest.raises(ValueError, match=r"<bytes #0>: progressive JPEG \(SOF2\) is not supported"):
        jpeg.pack([d], pin=False)
    with pytest.raises(ValueError, match=r"<bytes #0>: progressive JPEG \(SOF2\) is not supported"):
        jpeg.pack([d], pin=False, progressive=False)
    with pytest.raises(ValueError, match=r"x.jpg: progressive JPEG \(SOF2\) is not supported"):
        jpeg.frame_size(d, "x.jpg")
    assert jpeg.frame_size(d, "x.jpg", progressive=True) == (32, 32)
    # the C entry itself: flags = 0 refuses, and packs a baseline file into the bytes yf_jpeg_pack makes
    lib = _lib.lib()
    b = jg.encode(smooth(32, 32), "420")
    blobs = []
    for ex in (False, True):
        ptrs = (ctypes.c_void_p * 1)(ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p))
        sizes = (ctypes.c_size_t * 1)(len(b))
        need, h, w = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int()
        args = (ctypes.byref(need), ctypes.byref(h), ctypes.byref(w))
        assert (lib.yf_jpeg_pack_ex(1, ptrs, sizes, 0, None, 0, *args) if ex else lib.yf_jpeg_pack(1, ptrs, sizes, None, 0, *args)) == 0
        buf = ctypes.create_string_buffer(need.value)
        if ex:
            assert lib.yf_jpeg_pack_ex(1, ptrs, sizes, 0, buf, need.value, *args) == 0
        else:
            assert lib.yf_jpeg_pack(1, ptrs, sizes, buf, need.value, *args) == 0
        blobs.append(buf.raw)
    assert blobs[0] == blobs[1]
    ptrs = (ctypes.c_void_p * 1)(ctypes.cast(ctypes.c_char_p(d), ctypes.c_void_p))
    sizes = (ctypes.c_size_t * 1)(len(d))
    assert lib.yf_jpeg_pack_ex(1, ptrs, sizes, 0, None, 0, *args) == _lib.YF_E_INVALID
    assert b"progressive JPEG (SOF2) is not supported" in lib.yf_last_error_string()
    assert lib.yf_jpeg_pack_ex(1, ptrs, sizes, 2, None, 0, *args) == _lib.YF_E_INVALID


@pytest.mark.parametrize("layout", jg.LAYOUTS)
@pytest.mark.parametrize("kw", [{}, {"optimize": True, "quality": 30}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1}])
def test_pillow_files_are_accepted_with_their_scripts(layout, kw):
    d = jg.encode(smooth(40, 24), layout, progressive=True, **kw)
    blob, h, w = jpeg.pack([d], pin=False, progressive=True)
    assert (h, w) == (24, 40)
    nc = 1 if layout == "gray" else 3
    script, levels, nlevel = script_of(blob)
    assert script == masks(jp.pillow_script(nc))
    assert nlevel == 3
    assert levels == ([0, 0, 0, 1, 1, 2] if nc == 1 else [0, 0, 0, 0, 0, 1, 1, 1, 1, 2])      # 3, 2, 1 and 5, 4, 1 scans per level
    # each scan's bytes are where the file has them, up to the next marker
    for s in range(len(script)):
        i = jpeg.scan_info(blob, 0, s)
        assert d[i["offset"] - 3:i["offset"]] == bytes([script[s][1], script[s][2], (script[s][3] << 4) | script[s][4]])
        end = i["offset"] + i["length"]
        assert d[end] == 0xFF and d[end + 1] in (0xC4, 0xDA, 0xD9, 0xDD)
    mcux = -(-40 // (8 * jw.SAMPLING[layout][0]))
    if "restart_marker_blocks" in kw:
        assert all(jpeg.scan_info(blob, 0, s)["ri"] == 1 for s in range(len(script)))
    if "restart_marker_rows" in kw:
        assert jpeg.scan_info(blob, 0, 0)["ri"] == mcux
    assert jpeg.workspace_bytes(blob) > 0
    # a baseline frame reports no scans
    bb, _, _ = jpeg.pack([jg.encode(smooth(40, 24), layout)], pin=False, progressive=True)
    assert jpeg.scan_info(bb)["scans"] == 0


def test_levels_follow_dependency_not_file_order():
    """A chain in which every AC scan refines the one before it: one scan per level behind the first.  (A DC scan and an AC scan never
    overlap, so level 0 always holds the first scan of each of the two chains.)"""
    a = jw.textured(24, 16, 1)
    script = jp.scripts(1)["chain"]
    blob, _, _ = jpeg.pack([jp.encode(a, "gray", 90, script)], pin=False, progressive=True)
    got, levels, nlevel = script_of(blob)
    assert got == masks(script)
    assert levels == [0, 0, 1, 2, 3, 4] and nlevel == 5
    # the same chain with the DC coded in three scans spread between its links: the levels of the AC chain do not move
    spread = [((0,), 0, 0, 0, 2), script[1], script[2], ((0,), 0, 0, 2, 1), script[3], script[4], script[5], ((0,), 0, 0, 1, 0)]
    blob, _, _ = jpeg.pack([jp.encode(a, "gray", 90, spread)], pin=False, progressive=True)
    assert script_of(blob)[1] == [0, 0, 1, 1, 2, 3, 4, 2]
    # colour: chains of different components are independent
    blob, _, _ = jpeg.pack([jp.encode(a, "420", 90, jp.scripts(3)["deep"])], pin=False, progressive=True)
    got, levels, nlevel = script_of(blob)
    assert levels == [0] * 6 + [1] * 3 + [2] * 3 + [3] * 3 + [1] * 3 + [2] * 3 and nlevel == 4


def test_a_call_may_mix_kinds_of_one_size():
    a = smooth(40, 24)
    datas = [jg.encode(a, "420"), jg.encode(a, "gray", progressive=True), jg.encode(a, "444", restart_marker_blocks=1)]
    blob, h, w = jpeg.pack(datas, pin=False, progressive=True)
    assert [jpeg.scan_info(blob, k)["scans"] for k in range(3)] == [0, 6, 0]
    with pytest.raises(ValueError, match=r"<bytes #1>: progressive"):
        jpeg.pack(datas, pin=False)
    with pytest.raises(ValueError, match=r"differs from frame 0"):
        jpeg.pack([datas[0], jg.encode(smooth(16, 24), "gray", progressive=True)], pin=False, progressive=True)


REFUSALS = [                                # (script, writer keywords, reason)
    ([((0,), 0, 5, 0, 0), ((0,), 6, 63, 0, 0)], {}, r"a DC scan \(Ss = 0\) with Se != 0"),
    ([((0, 1, 2), 0, 0, 0, 0), ((0, 1), 1, 63, 0, 0)], {"layout": "444"}, r"an AC scan \(Ss > 0\) with more than one component"),
    ([((0,), 0, 0, 0, 0), ((0,), 9, 5, 0, 0)], {}, r"an AC scan with Se < Ss or Se > 63"),
    ([((0,), 0, 0, 0, 0), ((0,), 1, 64, 0, 0)], {}, r"an AC scan with Se < Ss or Se > 63"),
    ([((0,), 0, 0, 0, 14)], {}, r"successive approximation bit position Al > 13"),
    ([((0,), 0, 0, 0, 3), ((0,), 0, 0, 3, 1)], {}, r"a refinement scan with Al != Ah - 1"),
    ([((0,), 0, 0, 0, 3), ((0,), 0, 0, 2, 1)], {}, r"a refinement scan whose Ah is not the Al its band was last coded at"),
    ([((0,), 0, 0, 0, 0), ((0,), 1, 63, 2, 1)], {}, r"a refinement scan whose Ah is not the Al its band was last coded at"),
    ([((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((0,), 5, 9, 0, 0)], {}, r"a first scan \(Ah = 0\) of coefficients already coded"),
    ([((0,), 1, 63, 0, 0), ((0,), 0, 0, 0, 0)], {}, r"an AC scan of a component whose DC has not been coded"),
    ([((0,), 0, 0, 0, 0), ((0,), 1, 62, 0, 0)], {}, r"incomplete progression"),
    ([((0,), 0, 0, 0, 1), ((0,), 1, 63, 0, 0)], {}, r"incomplete progression"),
    ([((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0)], {"layout": "420"}, r"incomplete progression"),
    (None, {"precision": 12}, r"12-bit \(or other non-8-bit\) progressive JPEG is not supported"),
    (None, {"sof": 0xCA}, r"arithmetic-coded JPEG is not supported"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_refusals_name_the_file_and_the_reason(k, tmp_path):
    script, kw, reason = REFUSALS[k]
    kw = dict(kw)
    layout = kw.pop("layout", "gray")
    d = jp.encode(jw.textured(24, 16, k), layout, 90, script, **kw)
    p = tmp_path / "refused.jpg"
    p.write_bytes(d)
    with pytest.raises(ValueError, match=r"refused.jpg: " + reason):
        jpeg.frame_size(d, str(p), progressive=True)
    with pytest.raises(ValueError, match=r"<bytes #1>: " + reason):
        jpeg.pack([jp.encode(jw.textured(24, 16, k), layout, 90), d], pin=False, progressive=True)


def test_more_than_256_scans_and_a_missing_table_are_refused():
    a = jw.textured(8, 8, 3)
    # 64 one-coefficient bands x 4 passes + 1 = 257 scans of a valid progression
    script = [((0,), 0, 0, 0, 3)] + [((0,), 0, 0, ah, ah - 1) for ah in (3, 2, 1)]
    for k in range(1, 64):
        script += [((0,), k, k, 0, 3)] + [((0,), k, k, ah, ah - 1) for ah in (3, 2, 1)]
    script += [((0,), 0, 0, 0, 0)]                                   # the 257th
    assert len(script) == 257
    d = jp.encode(a, "gray", 90, script)
    with pytest.raises(ValueError, match=r"more than 256 scans"):
        jpeg.pack([d], pin=False, progressive=True)
    ok = jp.encode(a, "gray", 90, script[:256])
    blob, _, _ = jpeg.pack([ok], pin=False, progressive=True)
    assert jpeg.scan_info(blob)["scans"] == 256 and jpeg.scan_info(blob)["levels"] == 4
    assert np.array_equal(jg.pil_bgr(ok), jg.pil_bgr(jp.baseline(a, "gray", 90)))
    # the last scan's DHT segment cut out: its AC table index 0 was defined by an earlier scan, so take a file whose first AC scan is
    # chroma (table 1) and drop that segment
    d = jp.encode(jw.textured(16, 16, 4), "444", 90, [((0, 1, 2), 0, 0, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0), ((0,), 1, 63, 0, 0)])
    k = d.find(b"\xff\xc4", d.find(b"\xff\xda"))
    cut = d[:k] + d[k + 2 + ((d[k + 2] << 8) | d[k + 3]):]
    with pytest.raises(ValueError, match=r"scan uses a Huffman table that was never defined"):
        jpeg.pack([cut], pin=False, progressive=True)


def test_progressive_needs_device_decode_in_both_drivers(tmp_path):
    import voc_tree
    import yolo_fastest_amd as yf
    from yolo_fastest_amd.dataset import DetectDataset
    trees = voc_tree.make_trees(tmp_path)
    log = logging.getLogger("test-cpu-jpeg-prog")
    with pytest.raises(ValueError, match='progressive=True needs decode="device"'):
        DetectDataset([256, 320, 1], [512, 640, 3], log, aug_params=voc_tree.aug_params(trees), device="cpu", progressive=True)
    with pytest.raises(ValueError, match='progressive=True needs decode="device"'):
        yf.Detect_YOLO("cpu", "no-such-file.pth", {"io_params": yf.io_params_for(256)}, log, decode="host", progressive=True)
    ds = DetectDataset([256, 320, 1], [512, 640, 3], log, aug_params=voc_tree.aug_params(trees), device="cpu", decode="device", progressive=True)
    assert ds.progressive and ds.decode == "device"


def _dht_tables(d):
    """Per scan in file order: {table id (0..3 DC, 4..7 AC): (bits, values)} as the DHT segments in front of it define them (cumulative)."""
    cur, out, i = {}, [], 2
    while i < len(d):
        assert d[i] == 0xFF
        if d[i + 1] == 0xFF:
            i += 1
            continue
        m = d[i + 1]
        if m == 0xD9:
            break
        ln = (d[i + 2] << 8) | d[i + 3]
        s = d[i + 4:i + 2 + ln]
        if m == 0xC4:
            k = 0
            while k < len(s):
                bits = list(s[k + 1:k + 17])
                cur[(s[k] >> 4) * 4 + (s[k] & 15)] = (bits, list(s[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
        i += 2 + ln
        if m == 0xDA:
            out.append(dict(cur))
            while not (d[i] == 0xFF and d[i + 1] not in (0x00, 0xFF) and not 0xD0 <= d[i + 1] <= 0xD7):
                i += 1
    return out


@pytest.mark.parametrize("source", ["pillow", "pillow_optimize", "writer_redefine", "writer_merged"])
def test_every_code_of_every_scan_table_decodes_through_the_lookup(source):
    a = jw.textured(48, 40, 2)
    if source.startswith("pillow"):
        d = jg.encode(a, "420", progressive=True, quality=95, optimize=source == "pillow_optimize")
    else:
        d = jp.encode(a, "420", 95, jp.scripts(3)["pairs"], redefine=source == "writer_redefine", dht="merged" if source == "writer_merged" else "split")
    blob, _, _ = jpeg.pack([d], pin=False, progressive=True)
    tables = _dht_tables(d)
    n = jpeg.scan_info(blob)["scans"]
    assert n == len(tables)
    lib = _lib.lib()
    length, symbol = ctypes.c_int(), ctypes.c_int()
    checked = 0
    for s in range(n):
        i = jpeg.scan_info(blob, 0, s)
        if i["ss"] == 0 and i["ah"]:
            used = []                                                 # a DC refinement names no table
        elif i["ss"] == 0:
            used = sorted({0 if c == 0 else 1 for c in range(3) if i["comp_mask"] >> c & 1})
        else:
            used = [4 + (0 if i["comp_mask"] == 1 else 1)]
        for t in range(8):
            rc = lib.yf_jpeg_huff_lookup_ex(ctypes.c_void_p(blob.data_ptr()), 0, s, t, 0, ctypes.byref(length), ctypes.byref(symbol))
            assert (rc == 0) == (t in used), (s, t)
        for t in used:
            for sym, (code, ln) in jw.canonical(*tables[s][t]).items():
                for tail in (0, (1 << (16 - ln)) - 1):
                    _lib.check(lib.yf_jpeg_huff_lookup_ex(ctypes.c_void_p(blob.data_ptr()), 0, s, t, (code << (16 - ln)) | tail,
                                                          ctypes.byref(length), ctypes.byref(symbol)))
                    assert (length.value, symbol.value) == (ln, sym), (s, t, sym)
                    checked += 1
            _lib.check(lib.yf_jpeg_huff_lookup_ex(ctypes.c_void_p(blob.data_ptr()), 0, s, t, 0xFFFF, ctypes.byref(length), ctypes.byref(symbol)))
            assert length.value == 0                                  # the reserved all-ones code
    assert checked > 100


@pytest.mark.parametrize("w,h", [(17, 9), (33, 17), (72, 56)])
@pytest.mark.parametrize("layout", jw.LAYOUTS)
def test_the_writer_is_a_real_encoder(layout, w, h):
    """PIL decodes every script of the matrix, to the pixels PIL decodes from the writer's baseline file of the same coefficients; and
    the packer reads back the script that was written."""
    nc = 1 if layout == "gray" else 3
    a = jw.textured(w, h, 31 * w + h)
    want = jg.pil_bgr(jp.baseline(a, layout, 90))
    for name, script in jp.scripts(nc).items():
        n = len(script)
        for kw in ({}, {"ri": 1, "fill": 1}, {"ri": [(5 if i % 2 else 0) for i in range(n)], "dht": "merged", "redefine": True, "marker_fill": 2},
                   {"ri": 7, "late_dqt": True}, {"max_run": 3}):
            d = jp.encode(a, layout, 90, script, **kw)
            assert np.array_equal(jg.pil_bgr(d), want), (name, kw)
            blob, hh, ww = jpeg.pack([d], pin=False, progressive=True)
            assert (hh, ww) == (h, w) and script_of(blob)[0] == masks(script)
            if isinstance(kw.get("ri"), list):
                assert [jpeg.scan_info(blob, 0, s)["ri"] for s in range(n)] == kw["ri"]


def test_the_writer_reaches_the_eob_run_limit():
    flat = np.full((1024, 2048), 100, np.uint8)
    script = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)]
    d = jp.encode(flat, "gray", 90, script)
    blob, _, _ = jpeg.pack([d], pin=False, progressive=True)
    i = jpeg.scan_info(blob, 0, 1)
    # EOB14 with all 14 extra bits set (32767 blocks), then EOB0 for the last block: 2 symbols of an optimal 2-symbol table (1 bit each)
    # + 14 bits = 16 bits
    assert i["length"] <= 4                                      # 17 or 18 bits, and a stuffed zero behind the 0xFF they hold
    assert np.array_equal(jg.pil_bgr(d), jg.pil_bgr(jp.baseline(flat, "gray", 90)))
