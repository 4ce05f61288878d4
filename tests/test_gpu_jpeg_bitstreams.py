"""The device JPEG decoder (csrc/yf_jpeg_kernels.hip) bit for bit against PIL on the streams Pillow's encoder never writes, made at test
time by tests/jpeg_write.py: 4:4:0, RGB colour under every marker combination, SOF1 with 16-bit DQT, table indices 1..3, one-code and
16-bit-code tables, merged and redefined DHT segments, restart intervals around the 64-lane split with fill bytes, frames of one size that
differ in everything else within one call, 8192-pixel sides, the worst case of the speculative synchronisation (flat frames, round counts
from tests/jpeg_sync.py), and every status flag with the output guard bytes intact."""
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_gen as jg  # noqa: E402
import jpeg_sync as js  # noqa: E402
import jpeg_write as jw  # noqa: E402

ST_BAD_CODE, ST_BAD_INDEX, ST_TRUNCATED, ST_RESTART = 1, 2, 4, 8


@pytest.fixture(scope="module")
def jpeg():
    from yolo_fastest_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def decode_one_call(jpeg, datas, dev):
    """All `datas` (one size) in ONE yf_jpeg_decode_u8 call -> (host bgr [n, h, w, 3], host status [n])."""
    blob, h, w = jpeg.pack(datas)
    bgr, st = jpeg.decode_blob(blob, h, w, dev)
    torch.cuda.synchronize(dev)
    return bgr.cpu().numpy(), st.cpu().numpy()


def assert_bitwise(got, st, datas, what):
    for i, d in enumerate(datas):
        want = jg.pil_bgr(d)
        assert st[i] == 0, (what, i, int(st[i]))
        assert got[i].shape == want.shape, (what, i)
        ndiff = int((got[i] != want).any(2).sum())
        assert ndiff == 0, (what, i, ndiff, int(np.abs(got[i].astype(int) - want).max()))


def check(jpeg, dev, datas, what):
    got, st = decode_one_call(jpeg, datas, dev)
    assert_bitwise(got, st, datas, what)
    return got


SIZES_440 = jg.SIZES + [(5, 2), (9, 3), (13, 4), (33, 17), (40, 31)]     # chroma height 1 and 2; a partly filled last MCU row


@pytest.mark.parametrize("w,h", SIZES_440)
@pytest.mark.parametrize("content", ["noise", "smooth"])
def test_440(jpeg, dev, content, w, h):
    """Luma 1 x 2 (the h1v2 upsampler): standard and optimised tables, with and without restart markers, qualities 10 .. 100 (75 only
    for the two large sizes)."""
    rng = np.random.default_rng(31 * w + h + (content == "noise"))
    a = jg.image(content, w, h, rng)
    mcux = -(-w // 8)
    qs = (10, 75, 100) if w * h < 100000 else (75,)
    datas = [jw.encode(a, "440", q, huff=huff, ri=ri) for q in qs for huff in ("std", "opt") for ri in (0, 1, mcux)]
    check(jpeg, dev, datas, ("440", content, w, h))


def test_rgb_files(jpeg, dev):
    """Pillow's keep_rgb files (Adobe transform 0, IDs R, G, B; Pillow writes them at 4:4:4 only) and the writer's RGB files in every
    layout; then every colour-guess case of tests/test_cpu_jpeg_write.py, which the packer must read as libjpeg does."""
    rng = np.random.default_rng(8)
    for w, h in ((1, 1), (17, 33), (64, 48), (801, 603)):
        a = jg.image("noise", w, h, rng) if w < 100 else jw.textured(w, h, 3)
        datas = []
        for kw in (dict(quality=75), dict(quality=100), dict(quality=90, optimize=True), dict(quality=75, restart_marker_blocks=1)):
            b = io.BytesIO()
            Image.fromarray(a).save(b, "JPEG", keep_rgb=True, **kw)
            datas.append(b.getvalue())
        for layout in ("444", "440", "422", "420"):
            for markers, ids in (((("adobe", 0),), [1, 2, 3]), ((), [82, 71, 66]), ((("adobe", 0),), [82, 71, 66])):
                datas.append(jw.encode(a, layout, 85, rgb=True, markers=markers, ids=ids, huff="opt" if layout == "420" else "std"))
        check(jpeg, dev, datas, ("rgb", w, h))
    for layout in ("444", "420", "440"):
        check(jpeg, dev, [jw.colour_case(markers, ids, layout)[1] for markers, ids in jw.GUESS_CASES], ("colour guess", layout))


def test_sof1_16_bit_tables(jpeg, dev):
    """Pillow's own tables with entries 256 .. 1000 (it then writes 16-bit DQT and SOF1) and the writer's 16-bit tables with small values."""
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    big = [[256 + (i * 47 + t * 13) % 745 for i in range(64)] for t in range(2)]
    datas = []
    for layout in ("gray", "444", "420"):
        im = Image.fromarray(a[:, :, 0]) if layout == "gray" else Image.fromarray(a)
        kw = {} if layout == "gray" else {"subsampling": jg.SUBSAMPLING[layout]}
        b = io.BytesIO()
        im.save(b, "JPEG", qtables=big[:1] if layout == "gray" else big, **kw)
        d = b.getvalue()
        assert b"\xff\xc1" in d[:d.find(b"\xff\xda")]
        datas.append(d)
    for layout in jw.LAYOUTS:
        for q in (50, 95, 100):
            datas.append(jw.encode(a, layout, q, q16=True))
    check(jpeg, dev, datas, "sof1")


def test_table_indices_and_shapes(jpeg, dev):
    """Luma on DC / AC table 3 and chroma on 1 / 2, quantisation table 3, one-code tables, 16-bit codes, merged and redefined DHT."""
    rng = np.random.default_rng(13)
    a = jw.textured(96, 64, 13)
    n = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    flat = np.full((64, 96, 3), 93, np.uint8)
    idx = dict(qidx=[3, 2, 1], dcidx=[3, 1, 2], acidx=[3, 2, 1])
    datas = []
    for layout in jw.LAYOUTS:
        datas += [jw.encode(a, layout, 80, **idx), jw.encode(n, layout, 100, huff="deep", **idx), jw.encode(a, layout, 75, huff="deep"),
                  jw.encode(flat, layout, 75, huff="opt"), jw.encode(a, layout, 90, huff="opt", dht="merged"),
                  jw.encode(a, layout, 90, redefine=True), jw.encode(n, layout, 60, huff="opt", dht="merged", redefine=True, **idx),
                  jw.encode(a, layout, 70, qidx=[0, 0, 0], dcidx=[0, 0, 0], acidx=[0, 0, 0])]
    longest = max(max(i + 1 for i in range(16) if s[1 + i]) for d in datas for m, s in jw._segments(d) if m == 0xC4)
    assert longest == 16
    assert any(sum(s[1:17]) == 1 for d in datas for m, s in jw._segments(d) if m == 0xC4)      # a one-code table
    check(jpeg, dev, datas, "tables")


def ri_near_64_intervals(nmcu):
    """Restart intervals whose interval counts are the attainable ones nearest 63, 64 and 65 on either side."""
    return {r for n in (63, 64, 65) for r in (-(-nmcu // n), -(-nmcu // n) - 1)}


@pytest.mark.parametrize("fill", [0, 1, 3])
@pytest.mark.parametrize("layout,w,h", [("gray", 801, 603), ("420", 640, 512)])
def test_restart_intervals(jpeg, dev, layout, w, h, fill):
    """Intervals around the lane split lo = lane * nint / 64: 63, 64 and 65 intervals, a partly filled last interval, ri > nmcu."""
    mcux, mcuy = jw.mcu_counts(w, h, layout)
    nmcu = mcux * mcuy
    ris = sorted({1, 2, 3, 7, mcux - 1, mcux + 1, nmcu - 1, nmcu, nmcu + 5} | ri_near_64_intervals(nmcu))
    nints = {-(-nmcu // ri) for ri in ris}
    assert {63, 64, 65} <= nints if layout == "gray" else 64 in nints       # 1 280 MCUs: 61, 64 and 68 intervals around 64
    a = jw.textured(w, h, 21)
    datas = [jw.encode(a, layout, 75, ri=ri, fill=fill, huff="opt" if ri % 2 else "std") for ri in ris]
    check(jpeg, dev, datas, (layout, fill))


def test_mixed_call(jpeg, dev):
    """Frames of one size that differ in layout, colour, SOF, tables and restart markers: one call equals PIL and the per-frame calls."""
    rng = np.random.default_rng(17)
    w, h = 72, 40
    datas = [jg.encode(jg.image("noise", w, h, rng), "420", quality=80), jg.encode(jg.image("smooth", w, h, rng), "gray", quality=90)]
    for k, layout in enumerate(jw.LAYOUTS):
        a = jg.image("noise" if k % 2 else "smooth", w, h, rng)
        datas += [jw.encode(a, layout, 60 + 8 * k, ri=k, fill=k % 3, huff=("std", "opt", "deep")[k % 3], q16=bool(k % 2)),
                  jw.encode(a, layout, 85, rgb=True, ids=[82, 71, 66], markers=(), qidx=[3, 2, 1], dcidx=[3, 1, 2], acidx=[3, 2, 1]),
                  jw.encode(a, layout, 95, markers=(("adobe", 1),), dht="merged", redefine=True, ri=5)]
    b = io.BytesIO()
    Image.fromarray(jg.image("noise", w, h, rng)).save(b, "JPEG", keep_rgb=True)
    datas.append(b.getvalue())
    got = check(jpeg, dev, datas, "mixed")
    for i, d in enumerate(datas):
        one, st = decode_one_call(jpeg, [d], dev)
        assert st[0] == 0 and np.array_equal(one[0], got[i]), i


@pytest.mark.parametrize("w,h", [(8192, 8), (8, 8192)])
def test_largest_sides(jpeg, dev, w, h):
    rng = np.random.default_rng(w)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    datas = [jw.encode(a, layout, 75, ri=ri) for layout in ("gray", "420") for ri in (0, 7)]
    datas += [jg.encode(a, "gray", quality=75), jg.encode(a, "420", quality=75)]
    check(jpeg, dev, datas, (w, h))


def flat_fixtures():
    """Flat frames (gray and 4:2:0, several sizes, values and qualities), and flat frames with a few edge pixels changed."""
    out = []
    for w, h in ((64, 48), (640, 512), (801, 603), (8, 8)):
        for layout in ("gray", "420"):
            for v, q in ((77, 75), (0, 75), (200, 75), (128, 10), (77, 100)):
                a = np.full((h, w, 3), v, np.uint8)
                out.append(((w, h, layout, v, q, "flat"), jg.encode(a, layout, quality=q)))
            a = np.full((h, w, 3), 77, np.uint8)
            a[0, 0], a[h - 1, w - 1], a[h // 2, 0] = (255, 0, 0), (0, 255, 0), (0, 0, 255)
            out.append(((w, h, layout, 77, 75, "edges"), jg.encode(a, layout, quality=75)))
    return out


def test_worst_case_synchronisation(jpeg, dev):
    """Flat frames: every bit run of the stream is periodic, so a lane that starts out of phase never falls back into step on its own
    and the chain of redone lanes moves one lane per round.  At least one fixture needs all 64 rounds (the bound of the round loop, so
    it is exercised, not assumed), and at least one of those would have left lane 63's MCU count short after 63 rounds."""
    fx = flat_fixtures()
    res = [js.sync(d) for _, d in fx]
    for (what, _), r in zip(fx, res):
        print("sync rounds %2d  %s" % (r["rounds"], what))
        assert r["exact"] and r["rounds"] <= js.LANES, what
    full = [r for r in res if r["rounds"] == js.LANES]
    assert full, "no fixture needs 64 rounds"
    assert any(r["mcu0_63"] + r["mcus63_at63"] < r["nmcu"] for r in full)
    by_size = {}
    for (what, d), r in zip(fx, res):
        by_size.setdefault(what[:2], []).append(d)
    for (w, h), datas in by_size.items():
        check(jpeg, dev, datas, ("flat", w, h))


def guarded_decode(jpeg, dev, good, bad):
    """[good, bad] in one call into an output with guard bytes around it -> (status [2], good frame)."""
    blob, h, w = jpeg.pack([good, bad])
    frame = h * w * 3
    guard = 4096
    buf = torch.full((guard + 2 * frame + guard,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + 2 * frame].view(2, h, w, 3)
    _, st = jpeg.decode_blob(blob, h, w, dev, out=out)
    torch.cuda.synchronize(dev)
    host = buf.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[guard + 2 * frame:] == 0xA5).all()
    return st.cpu().numpy(), host[guard:guard + frame].reshape(h, w, 3)


@pytest.mark.parametrize("kind,flag", [("truncated", ST_TRUNCATED), ("all_ones", ST_BAD_CODE), ("dropped_rst", ST_RESTART),
                                       ("extra_rst", ST_RESTART), ("zrl_past_63", ST_BAD_INDEX), ("truncated_rst", ST_TRUNCATED)])
@pytest.mark.parametrize("layout", ["gray", "420", "440"])
def test_status_flags(jpeg, dev, kind, flag, layout):
    """Each corruption sets its flag (a later bad code may add ST_BAD_CODE, so the flag is tested, not the word); the good frame of the
    same call is exact and nothing is written outside the output."""
    a = jw.textured(64, 48, 5)
    ri = 2 if kind in ("dropped_rst", "extra_rst", "truncated_rst") else 0
    base = jw.encode(a, layout, 75, ri=ri)
    bad = {"truncated": lambda: jg.truncated(base), "truncated_rst": lambda: jg.truncated(base), "all_ones": lambda: jg.altered(base),
           "dropped_rst": lambda: jw.encode(a, layout, 75, ri=ri, drop_rst=2),
           "extra_rst": lambda: jw.encode(a, layout, 75, ri=ri, extra_rst=1),
           "zrl_past_63": lambda: jw.encode(a, layout, 75, zrl_past_63=5)}[kind]()
    good = jw.encode(jw.textured(64, 48, 6), layout, 90, ri=ri)
    st, first = guarded_decode(jpeg, dev, good, bad)
    assert st[0] == 0, st
    assert st[1] & flag, (kind, int(st[1]))
    assert np.array_equal(first, jg.pil_bgr(good))
