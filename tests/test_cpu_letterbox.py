"""The letterbox mode's host half (no GPU): yf_letterbox_geometry against the Python rule (tests/letterbox_ref.py), the ABI surface of the
three new entries, and their refusals, which come before the GPU is touched."""
import ctypes
import os
import re

import pytest

import letterbox_ref as ref
from yolo_fastest_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = [(256, 320), (64, 96)]


def _geometry(lib, h, w, H, W):
    out = (ctypes.c_int32 * 6)()
    assert lib.yf_letterbox_geometry(h, w, H, W, out) == _lib.YF_OK
    return tuple(out)


@pytest.mark.parametrize("net", NETS)
def test_geometry_equals_the_python_rule(net):
    lib = _lib.lib()
    H, W = net
    for a in range(1, 701):
        for b in (1, 7, 317, 640, 641):
            for h, w in ((a, b), (b, a)):
                got = _geometry(lib, h, w, H, W)
                assert got == ref.geometry(h, w, H, W), (h, w, net)
                new_h, new_w, top, bottom, left, right = got
                assert top + new_h + bottom == H and left + new_w + right == W and min(top, bottom, left, right) >= 0
                assert new_h == H or new_w == W


@pytest.mark.parametrize("net", NETS + [(512, 640)])
def test_frames_of_the_nets_aspect_ratio_get_no_border(net):
    lib = _lib.lib()
    H, W = net
    seen = 0
    for k in range(1, 4001):
        if (k * H) % 64 or (k * W) % 64:
            continue
        h, w = k * H // 64, k * W // 64
        assert _geometry(lib, h, w, H, W) == (H, W, 0, 0, 0, 0) == ref.geometry(h, w, H, W), (h, w)
        seen += 1
    assert seen >= 2000


def test_the_listed_frame_sizes_are_the_cases_they_are_listed_for():
    lib = _lib.lib()
    want = {(512, 640): (256, 320, 0, 0, 0, 0), (480, 640): (240, 320, 8, 8, 0, 0), (360, 640): (180, 320, 38, 38, 0, 0),
            (511, 640): (256, 320, 0, 0, 0, 0), (512, 1280): (128, 320, 64, 64, 0, 0), (640, 360): (256, 144, 0, 0, 88, 88),
            (101, 640): (50, 320, 103, 103, 0, 0), (253, 317): (255, 320, 0, 1, 0, 0), (20, 30): (213, 320, 21, 22, 0, 0)}
    for (h, w), g in want.items():
        assert _geometry(lib, h, w, 256, 320) == g == ref.geometry(h, w, 256, 320), (h, w)
    assert 101 * min(256 / 101, 320 / 640) == 50.5            # the half that goes to even


def test_geometry_refuses_non_positive_sizes():
    lib = _lib.lib()
    out = (ctypes.c_int32 * 6)()
    for a in ((0, 5, 256, 320), (5, 0, 256, 320), (5, 5, 0, 320), (5, 5, 256, 0), (-1, 5, 256, 320), (5, 5, 256, -320)):
        assert lib.yf_letterbox_geometry(*a, out) == _lib.YF_E_INVALID, a
    assert lib.yf_letterbox_geometry(5, 5, 256, 320, None) == _lib.YF_E_INVALID


def test_header_bindings_and_exports_carry_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "yolo_fastest_hip.h")).read()
    want = {
        "yf_letterbox_geometry": "int src_h, int src_w, int dst_h, int dst_w, int32_t out[6]",
        "yf_cv_letterbox_u8": "int device, int N, const void *const *d_frames, const int *heights, const int *widths, int gray_bits, int dst_h, "
                              "int dst_w, uint8_t *d_dst, void *d_table, size_t table_bytes, void *h_table_pinned, void *stream",
        "yf_scale_boxes": "int device, int32_t *d_boxes, long frame_stride, const int32_t *d_counts, long count_stride, int N, int K_max, "
                          "int net_h, int net_w, const int32_t *d_frame_hw, void *stream",
    }
    lib = _lib.lib()
    for name, args in want.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, hdr, re.M)
        assert m and re.sub(r"\s+", " ", m.group(1)) == args, name
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][1]) == args.count(",") + 1 and hasattr(lib, name)
    assert re.search(r"#define\s+YF_LB_TABLE_ENTRY_BYTES\s+40\b", hdr) and _lib.YF_LB_TABLE_ENTRY_BYTES == 40
    assert lib.yf_abi_version() == 1 == _lib.ABI_VERSION and re.search(r"#define\s+YF_ABI_VERSION\s+1\b", hdr)


def test_letterbox_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()                   # host memory: a call that got past the checks would fail, not be refused
    p = ctypes.addressof(buf)
    eb = _lib.YF_LB_TABLE_ENTRY_BYTES
    good = dict(N=2, frames=[p, p + 64], hs=[4, 3], ws=[5, 2], gray=15, H=64, W=96, dst=p, table=p, table_bytes=2 * eb, pinned=p)

    def call(**kw):
        a = dict(good, **kw)
        n = 2
        frames = None if a["frames"] is None else (ctypes.c_void_p * n)(*a["frames"])
        hs = None if a["hs"] is None else (ctypes.c_int * n)(*a["hs"])
        ws = None if a["ws"] is None else (ctypes.c_int * n)(*a["ws"])
        return lib.yf_cv_letterbox_u8(0, a["N"], frames, hs, ws, a["gray"], a["H"], a["W"], a["dst"], a["table"], a["table_bytes"], a["pinned"], None)
    for kw in (dict(N=0), dict(N=-1), dict(frames=None), dict(hs=None), dict(ws=None), dict(dst=None), dict(table=None), dict(pinned=None),
               dict(frames=[p, None]), dict(hs=[4, 0]), dict(ws=[-5, 2]), dict(hs=[4, 8193]), dict(ws=[8193, 2]), dict(H=0), dict(W=-96),
               dict(H=8193), dict(gray=1), dict(gray=16), dict(gray=-14), dict(table_bytes=2 * eb - 1), dict(table_bytes=0),
               dict(hs=[4, 1], ws=[5, 700])):       # the last one: new_h rounds to 0, where cv2.resize raises
        assert call(**kw) == _lib.YF_E_INVALID, kw
        assert b"yf_cv_letterbox_u8" in lib.yf_last_error_string()
    assert bytes(buf) == bytes(4096)                  # no refused call wrote the pinned copy


def test_scale_boxes_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    good = dict(boxes=p, fs=16, counts=p, cs=1, N=2, K=4, H=64, W=96, hw=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.yf_scale_boxes(0, a["boxes"], a["fs"], a["counts"], a["cs"], a["N"], a["K"], a["H"], a["W"], a["hw"], None)
    for kw in (dict(boxes=None), dict(counts=None), dict(hw=None), dict(N=0), dict(N=-2), dict(K=0), dict(K=-1), dict(H=0), dict(W=0), dict(fs=15),
               dict(cs=0), dict(fs=-16)):
        assert call(**kw) == _lib.YF_E_INVALID, kw
        assert b"yf_scale_boxes" in lib.yf_last_error_string()
