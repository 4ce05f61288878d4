"""The device JPEG decoder (csrc/yf_jpeg_kernels.hip via yolo_fastest_amd/jpeg.py) bit for bit against PIL's decode (libjpeg-turbo):
`np.asarray(Image.open(f).convert("RGB"))[:, :, ::-1]`, the bytes DetectDataset._decode and Detect_YOLO._read_bgr return.  Inputs: the
bundled frames, the VOC fixtures and a seeded matrix made here with PIL (tests/jpeg_gen.py); corrupt scans for the status words."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import jpeg_gen as jg  # noqa: E402

GOLDEN_DIR = os.path.join(HERE, "golden", "test_data")
VOC_DIR = os.path.join(HERE, "golden", "voc", "img")


@pytest.fixture(scope="module")
def jpeg():
    from yolo_fastest_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def read_all(d):
    return [open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))]


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


def test_bundled_frames_in_one_call(jpeg, dev):
    datas = read_all(GOLDEN_DIR)
    assert len(datas) == 20
    got, st = decode_one_call(jpeg, datas, dev)
    assert got.shape == (20, 512, 640, 3)
    assert_bitwise(got, st, datas, "bundled")


def test_voc_fixtures(jpeg, dev):
    names = sorted(os.listdir(VOC_DIR))
    datas = read_all(VOC_DIR)
    groups = jpeg.decode_files([os.path.join(VOC_DIR, n) for n in names], dev)
    sizes = sorted(tuple(g.bgr.shape[1:3]) for g in groups)
    assert (600, 800) in sizes                         # the frame whose last MCU row is partly filled (600 = 37.5 rows of 16)
    assert sorted(p for g in groups for p in g.positions) == list(range(len(names)))
    for g in groups:
        got = g.bgr.cpu().numpy()
        assert_bitwise(got, np.zeros(len(g.positions), np.int32), [datas[p] for p in g.positions], "voc")


@pytest.mark.parametrize("w,h", jg.SIZES)
@pytest.mark.parametrize("content", ["noise", "smooth"])
@pytest.mark.parametrize("layout", jg.LAYOUTS)
def test_seeded_matrix(jpeg, dev, layout, content, w, h):
    """quality {10, 75, 100} x optimize {off, on} x restart markers {none, every block, every MCU row}: 18 files in one call."""
    rng = np.random.default_rng(1000 * w + h + 7 * jg.LAYOUTS.index(layout) + (content == "noise"))
    datas = [jg.encode(jg.image(content, w, h, rng), layout, **kw) for kw in jg.settings()]
    got, st = decode_one_call(jpeg, datas, dev)
    assert_bitwise(got, st, datas, (layout, content, w, h))


@pytest.mark.parametrize("layout", jg.LAYOUTS)
def test_quality_100_noise(jpeg, dev, layout):
    """Long codes, ZRL runs and the largest magnitudes; optimised tables make the longest codes."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (512, 640, 3), dtype=np.uint8)
    a[:, 320:] = (a[:, 320:] // 128) * 255                      # bi-level noise: bigger AC magnitudes
    datas = [jg.encode(a, layout, quality=100), jg.encode(a, layout, quality=100, optimize=True)]
    got, st = decode_one_call(jpeg, datas, dev)
    assert_bitwise(got, st, datas, ("q100", layout))


@pytest.mark.parametrize("layout", jg.LAYOUTS)
def test_sharp_checkerboard_quality_100(jpeg, dev, layout):
    """A one-pixel 0 / 255 checkerboard (and a coloured one): the IDCT overshoots past 0 and 255 into the range-limit table."""
    y, x = np.mgrid[0:64, 0:96]
    b = (((x + y) & 1) * 255).astype(np.uint8)
    a = np.stack([b, 255 - b, b], 2)
    datas = [jg.encode(a, layout, quality=100), jg.encode(a, layout, quality=97, optimize=True)]
    got, st = decode_one_call(jpeg, datas, dev)
    assert_bitwise(got, st, datas, ("checkerboard", layout))


def test_a_frame_does_not_depend_on_its_batch(jpeg, dev):
    datas = read_all(GOLDEN_DIR)
    tiled = (datas * 13)[:256]
    got, st = decode_one_call(jpeg, tiled, dev)
    assert not st.any()
    for i, d in enumerate(datas):
        one, s1 = decode_one_call(jpeg, [d], dev)
        assert s1[0] == 0
        for k in range(i, 256, 20):
            assert np.array_equal(got[k], one[0]), (i, k)


def test_graph_capture_replays_the_same_bytes(jpeg, dev):
    from yolo_fastest_amd import _lib
    rng = np.random.default_rng(3)
    datas = [jg.encode(jg.image("noise", 64, 48, rng), "420", quality=80) for _ in range(3)]
    datas.append(jg.encode(jg.image("smooth", 64, 48, rng), "420", quality=80, restart_marker_blocks=1))
    blob, h, w = jpeg.pack(datas)
    d_blob = torch.empty(blob.numel(), dtype=torch.uint8, device=dev)
    d_blob.copy_(blob)
    ws = torch.empty(jpeg.workspace_bytes(blob), dtype=torch.uint8, device=dev)
    out = torch.empty((len(datas), h, w, 3), dtype=torch.uint8, device=dev)
    st = torch.empty((len(datas),), dtype=torch.int32, device=dev)
    lib = _lib.lib()

    def call():
        _lib.check(lib.yf_jpeg_decode_u8(dev.index, ctypes.c_void_p(blob.data_ptr()), ctypes.c_void_p(d_blob.data_ptr()),
                                         ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(out.data_ptr()),
                                         ctypes.c_void_p(st.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    first = out.cpu().numpy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    out.zero_()
    ws.fill_(0x5A)
    st.fill_(-1)
    g.replay()
    torch.cuda.synchronize(dev)
    assert not st.cpu().numpy().any()
    assert np.array_equal(out.cpu().numpy(), first)
    assert_bitwise(first, np.zeros(len(datas), np.int32), datas, "graph")


@pytest.mark.parametrize("kind", ["truncated", "altered", "truncated_restart"])
def test_corrupt_scans_set_status_and_stay_in_bounds(jpeg, dev, kind, tmp_path):
    rng = np.random.default_rng(9)
    base = jg.encode(jg.image("noise", 64, 48, rng), "420", quality=75, **({"restart_marker_rows": 1} if kind == "truncated_restart" else {}))
    bad = jg.altered(base) if kind == "altered" else jg.truncated(base)
    good = jg.encode(jg.image("smooth", 64, 48, rng), "420", quality=75)
    blob, h, w = jpeg.pack([good, bad])
    frame = h * w * 3
    guard = 4096
    buf = torch.full((guard + 2 * frame + guard,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + 2 * frame].view(2, h, w, 3)
    bgr, st = jpeg.decode_blob(blob, h, w, dev, out=out)
    torch.cuda.synchronize(dev)
    host = buf.cpu().numpy()
    st = st.cpu().numpy()
    # the flag of the corruption (a later bad code may add ST_BAD_CODE = 1): truncated ST_TRUNCATED = 4, an all-ones run ST_BAD_CODE;
    # cut inside the restart intervals also ST_RESTART = 8 (markers missing)
    want = {"truncated": 4, "altered": 1, "truncated_restart": 4 | 8}[kind]
    assert st[0] == 0 and st[1] & want == want, st
    assert (host[:guard] == 0xA5).all() and (host[guard + 2 * frame:] == 0xA5).all()
    assert np.array_equal(host[guard:guard + frame].reshape(h, w, 3), jg.pil_bgr(good))
    p = tmp_path / ("%s.jpg" % kind)
    p.write_bytes(bad)
    with pytest.raises(OSError, match="%s.jpg: corrupt or truncated JPEG data" % kind):
        jpeg.decode_files([good, str(p)], dev)


def test_decode_files_groups_by_size(jpeg, dev, tmp_path):
    rng = np.random.default_rng(4)
    items = [jg.encode(jg.image("noise", 17, 33, rng), "420"), jg.encode(jg.image("noise", 64, 48, rng), "gray"),
             jg.encode(jg.image("smooth", 17, 33, rng), "444")]
    p = tmp_path / "x.jpg"
    p.write_bytes(items[1])
    groups = jpeg.decode_files([items[0], str(p), items[2]], dev)
    assert [g.positions for g in groups] == [[0, 2], [1]]
    assert tuple(groups[0].bgr.shape) == (2, 33, 17, 3) and tuple(groups[1].bgr.shape) == (1, 48, 64, 3)
    for g in groups:
        for k, i in enumerate(g.positions):
            assert np.array_equal(g.bgr[k].cpu().numpy(), jg.pil_bgr(items[i]))
    with pytest.raises(ValueError, match="<bytes #1>: progressive"):
        jpeg.decode_files([items[0], jg.encode(jg.image("smooth", 8, 8, rng), "gray", progressive=True)], dev)
