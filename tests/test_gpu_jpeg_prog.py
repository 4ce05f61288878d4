"""Progressive JPEG files through the device decoder (`progressive=True`: yf_jpeg_pack_ex + jpeg_prog_entropy_kernel in
csrc/yf_jpeg_kernels.hip) bit for bit against PIL's decode, and against the device's own decode of the baseline twin (the same
coefficients in a baseline file).  Inputs: the bundled frames and VOC fixtures re-saved by Pillow, a seeded Pillow matrix, and the scan
scripts Pillow never writes from tests/jpeg_write_prog.py; corrupt scans for the status words; both drivers."""
import ctypes
import io
import logging
import os
import random
import re
import shutil
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import jpeg_gen as jg  # noqa: E402
import jpeg_write as jw  # noqa: E402
import jpeg_write_prog as jp  # noqa: E402
import voc_tree  # noqa: E402

GOLDEN_DIR = os.path.join(HERE, "golden", "test_data")
VOC_DIR = os.path.join(HERE, "golden", "voc", "img")
WDIR = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights")
LOG = logging.getLogger("test-gpu-jpeg-prog")
LARGE_LIMIT_S = 120.0                      # test_one_large_frame's own time limit


@pytest.fixture(scope="module")
def jpeg():
    from yolo_fastest_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def resave(d, **kw):
    """The file's pixels saved again by Pillow (mode kept: L or RGB)."""
    from PIL import Image
    im = Image.open(io.BytesIO(d))
    im.load()
    b = io.BytesIO()
    with jg.big_encoder_buffer():
        im.save(b, "JPEG", **kw)
    return b.getvalue()


def is_progressive(d):
    return b"\xff\xc2" in d[:jg.scan_start(d)]


def decode_one_call(jpeg, datas, dev, progressive=True):
    blob, h, w = jpeg.pack(datas, progressive=progressive)
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


def test_bundled_frames_and_voc_fixtures_resaved_progressive(jpeg, dev, tmp_path):
    """One decode_files call over all of them (two frame sizes); PIL's bytes, and the device's bytes for the baseline twins."""
    src = [os.path.join(GOLDEN_DIR, n) for n in sorted(os.listdir(GOLDEN_DIR))] + [os.path.join(VOC_DIR, n) for n in sorted(os.listdir(VOC_DIR))]
    assert len(src) == 23
    prog, twin = [], []
    for k, p in enumerate(src):
        d = open(p, "rb").read()
        kw = dict(quality=90, optimize=True)
        q = tmp_path / ("p%02d.jpg" % k)
        q.write_bytes(resave(d, progressive=True, **kw))
        assert is_progressive(q.read_bytes())
        prog.append(str(q))
        twin.append(resave(d, **kw))
        assert not is_progressive(twin[-1])
    groups = jpeg.decode_files(prog, dev, progressive=True)
    tgroups = jpeg.decode_files(twin, dev)
    assert sorted(p for g in groups for p in g.positions) == list(range(23))
    assert [g.positions for g in groups] == [g.positions for g in tgroups] and len(groups) >= 2
    for g, t in zip(groups, tgroups):
        got = g.bgr.cpu().numpy()
        assert_bitwise(got, np.zeros(len(g.positions), np.int32), [open(prog[p], "rb").read() for p in g.positions], "resaved")
        assert np.array_equal(got, t.bgr.cpu().numpy())
    with pytest.raises(ValueError, match=r"p00.jpg: progressive JPEG \(SOF2\) is not supported"):
        jpeg.decode_files(prog, dev)


@pytest.mark.parametrize("w,h", jg.SIZES)
@pytest.mark.parametrize("content", ["noise", "smooth"])
@pytest.mark.parametrize("layout", jg.LAYOUTS)
def test_seeded_matrix_progressive(jpeg, dev, layout, content, w, h):
    """tests/test_gpu_jpeg.py's matrix with progressive=True: 18 encoder settings in one call, none left out."""
    rng = np.random.default_rng(1000 * w + h + 7 * jg.LAYOUTS.index(layout) + (content == "noise"))
    datas = [jg.encode(jg.image(content, w, h, rng), layout, progressive=True, **kw) for kw in jg.settings()]
    assert len(datas) == 18 and all(is_progressive(d) for d in datas)
    got, st = decode_one_call(jpeg, datas, dev)
    assert_bitwise(got, st, datas, (layout, content, w, h))


def check_writer(jpeg, dev, cases, what):
    """Each case (image, layout, quality, script, keywords): PIL's bytes, and the device's decode of the writer's baseline twin."""
    datas = [jp.encode(a, lay, q, script, **kw) for a, lay, q, script, kw in cases]
    twins = [jp.baseline(a, lay, q) for a, lay, q, script, kw in cases]
    got, st = decode_one_call(jpeg, datas, dev)
    assert_bitwise(got, st, datas, what)
    base, st2 = decode_one_call(jpeg, twins, dev, progressive=False)
    assert not st2.any()
    assert np.array_equal(got, base), what


@pytest.mark.parametrize("w,h", [(17, 9), (33, 17), (321, 257)])
@pytest.mark.parametrize("layout", jw.LAYOUTS)
def test_writer_scripts(jpeg, dev, layout, w, h):
    """Every script of jpeg_write_prog.scripts() in every layout (4:4:0 too), sizes with partial MCU rows and columns, so that the
    non-interleaved scans walk fewer blocks than the padded planes hold; tables merged / redefined, DRI changing between scans, fill
    bytes, a quantisation table that arrives late and is redefined after its latch."""
    nc = 1 if layout == "gray" else 3
    a = jw.textured(w, h, 31 * w + h)
    cases = []
    for name, script in jp.scripts(nc).items():
        if name == "al13" and w > 100:
            continue                                      # 42 scans of a python encoder: the two small sizes carry this script
        n = len(script)
        for kw in ({}, {"ri": 1, "fill": 1}, {"ri": [(5 if i % 2 else 0) for i in range(n)], "dht": "merged", "redefine": True, "marker_fill": 2},
                   {"ri": 7, "late_dqt": True}):
            if w > 100 and kw.get("ri") == 1:
                kw = {"ri": 3, "fill": 2}
            cases.append((a, layout, 90, script, kw))
    check_writer(jpeg, dev, cases, (layout, w, h))


@pytest.mark.parametrize("layout", ["gray", "420", "440"])
def test_restart_intervals_around_the_wave_width(jpeg, dev, layout):
    """63 / 64 / 65 restart intervals per scan (lanes with none, one and two intervals) and an interval longer than the scan."""
    nc = 1 if layout == "gray" else 3
    a = jw.textured(72, 56, 5)                           # gray: 9 x 7 = 63 blocks; 4:2:0: 20 MCUs, 63 luma blocks, 20 chroma blocks
    cases = []
    for script in (jp.pillow_script(nc), jp.scripts(nc)["deep"]):
        for ri in (1, 2, 62, 63, 64, 1000):
            cases.append((a, layout, 85, script, {"ri": ri}))
    b = jw.textured(8 * 13, 8 * 5, 6)                    # 65 blocks
    c = jw.textured(8 * 8, 8 * 8, 7)                     # 64 blocks
    for img in (b, c):
        cases2 = [(img, layout, 85, jp.scripts(nc)["deep"], {"ri": 1})]
        check_writer(jpeg, dev, cases2, ("ri", layout, img.shape))
    check_writer(jpeg, dev, cases, ("ri", layout))


def test_eob_run_of_32767_blocks(jpeg, dev):
    """A gray 2048 x 1024 frame (32768 blocks) whose AC bands are empty but for a few blocks: EOB runs up to the 32767 limit, across rows."""
    y, x = np.mgrid[0:1024, 0:2048]
    a = np.full((1024, 2048), 100, np.uint8)
    a[1016:, 2040:] = ((x[1016:, 2040:] + y[1016:, 2040:]) & 1) * 200        # the last block
    a[512:520, 8:16] = (x[512:520, 8:16] & 1) * 180                          # and one in the middle
    script = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)]
    d = jp.encode(a, "gray", 90, script)
    # the run / size symbols of an EOB14 run with all 14 extra bits set are in the stream: 32767 = (1 << 14) + 16383
    d2 = jp.encode(np.full((1024, 2048), 100, np.uint8), "gray", 90, script)
    got, st = decode_one_call(jpeg, [d, d2], dev)
    assert_bitwise(got, st, [d, d2], "eob run")
    short = jp.encode(a, "gray", 90, script, max_run=5)
    got2, st2 = decode_one_call(jpeg, [short], dev)
    assert st2[0] == 0 and np.array_equal(got2[0], got[0])


def test_al13_on_a_high_contrast_frame(jpeg, dev):
    rng = np.random.default_rng(13)
    a = (rng.integers(0, 2, (40, 56, 3)) * 255).astype(np.uint8)
    cases = [(a, lay, 100, jp.scripts(1 if lay == "gray" else 3)["al13"], {}) for lay in jw.LAYOUTS]
    for c in cases:
        check_writer(jpeg, dev, [c], ("al13", c[1]))


@pytest.mark.parametrize("order", ["baseline_first", "progressive_first"])
def test_baseline_and_progressive_frames_in_one_call(jpeg, dev, order):
    rng = np.random.default_rng(21)
    imgs = [jg.image("noise" if k % 2 else "smooth", 64, 48, rng) for k in range(6)]
    base = [jg.encode(a, "420", quality=80, **({"restart_marker_rows": 1} if k == 2 else {})) for k, a in enumerate(imgs[:3])]
    prog = [jg.encode(a, "420", quality=80, progressive=True) for a in imgs[3:5]] + [jp.encode(imgs[5], "gray", 80, jp.scripts(1)["deep"])]
    datas = base + prog if order == "baseline_first" else prog + base
    got, st = decode_one_call(jpeg, datas, dev)
    assert_bitwise(got, st, datas, order)
    info = [jpeg.scan_info(jpeg.pack(datas, pin=False, progressive=True)[0], k)["scans"] for k in range(6)]
    assert [n > 0 for n in info] == [is_progressive(d) for d in datas]
    # the baseline frames: the same bytes as without the flag
    b0, s0 = decode_one_call(jpeg, base, dev, progressive=False)
    k0 = 0 if order == "baseline_first" else 3
    assert np.array_equal(got[k0:k0 + 3], b0)


def test_256_frames_in_one_call_against_256_single_calls(jpeg, dev):
    datas = [resave(open(os.path.join(GOLDEN_DIR, n), "rb").read(), quality=85, progressive=True) for n in sorted(os.listdir(GOLDEN_DIR))]
    rng = np.random.default_rng(8)
    color = [jg.encode(jg.image("noise", 640, 512, rng), "420", quality=60, progressive=True) for _ in range(4)]
    tiled = ((datas + color) * 11)[:256]
    got, st = decode_one_call(jpeg, tiled, dev)
    assert not st.any()
    for k, d in enumerate(tiled):
        one, s1 = decode_one_call(jpeg, [d], dev)
        assert s1[0] == 0 and np.array_equal(got[k], one[0]), k
    assert_bitwise(got[:24], st[:24], tiled[:24], "256")


def test_graph_capture_replays_the_same_bytes_with_guards_intact(jpeg, dev):
    from yolo_fastest_amd import _lib
    rng = np.random.default_rng(3)
    datas = [jg.encode(jg.image("noise", 64, 48, rng), "420", quality=80, progressive=True) for _ in range(3)]
    datas.append(jg.encode(jg.image("smooth", 64, 48, rng), "420", quality=80, progressive=True, restart_marker_blocks=1))
    datas.append(jg.encode(jg.image("smooth", 64, 48, rng), "420", quality=80))
    blob, h, w = jpeg.pack(datas, progressive=True)
    d_blob = torch.empty(blob.numel(), dtype=torch.uint8, device=dev)
    d_blob.copy_(blob)
    guard = 4096
    nws, nout = jpeg.workspace_bytes(blob), len(datas) * h * w * 3
    ws_buf = torch.full((guard + nws + guard,), 0xA5, dtype=torch.uint8, device=dev)
    out_buf = torch.full((guard + nout + guard,), 0xA5, dtype=torch.uint8, device=dev)
    ws = ws_buf[guard:guard + nws]
    out = out_buf[guard:guard + nout].view(len(datas), h, w, 3)
    assert ws.data_ptr() % 256 == 0
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
    for buf, n in ((ws_buf, nws), (out_buf, nout)):
        host = buf.cpu().numpy()
        assert (host[:guard] == 0xA5).all() and (host[guard + n:] == 0xA5).all()


CORRUPTIONS = {                            # name: (layout, writer keywords, flag that must be set)
    "truncated_ac_first": ("420", {"truncate_scan": 1}, 4),
    "truncated_dc_first": ("420", {"truncate_scan": 0}, 4),
    "truncated_last_refinement": ("420", {"truncate_scan": 9}, 4),
    "truncated_gray_dc_refinement": ("gray", {"truncate_scan": 4}, 4),
    "all_ones_ac_first": ("420", {"ones_scan": 1}, 1),
    "all_ones_ac_refinement": ("420", {"ones_scan": 9}, 1),
    "dropped_rst": ("420", {"ri": 2, "drop_rst": (1, 1)}, 8),
    "extra_rst": ("420", {"ri": 2, "extra_rst": (9, 0)}, 8),
    "truncated_with_restarts": ("gray", {"ri": 2, "truncate_scan": 5}, 4 | 8),
    "run_past_se": ("420", {"run_past_se": 1}, 2),
}


@pytest.mark.parametrize("kind", list(CORRUPTIONS))
def test_corrupt_scans_set_status_and_stay_in_bounds(jpeg, dev, kind, tmp_path):
    layout, kw, want = CORRUPTIONS[kind]
    nc = 1 if layout == "gray" else 3
    a = jw.textured(64, 48, 9)
    bad = jp.encode(a, layout, 90, jp.pillow_script(nc), **kw)
    good = jg.encode(jg.image("smooth", 64, 48, None), "420", quality=75, progressive=True)
    good2 = jp.encode(a, layout, 90, jp.pillow_script(nc))
    blob, h, w = jpeg.pack([good, bad, good2], progressive=True)
    frame, guard = h * w * 3, 4096
    nws = jpeg.workspace_bytes(blob)
    buf = torch.full((guard + 3 * frame + guard,), 0xA5, dtype=torch.uint8, device=dev)
    ws_buf = torch.full((guard + nws + guard,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + 3 * frame].view(3, h, w, 3)
    bgr, st = jpeg.decode_blob(blob, h, w, dev, out=out, workspace=ws_buf[guard:guard + nws])
    torch.cuda.synchronize(dev)
    host, wsh, st = buf.cpu().numpy(), ws_buf.cpu().numpy(), st.cpu().numpy()
    assert st[0] == 0 and st[2] == 0 and st[1] & want == want, st
    assert (host[:guard] == 0xA5).all() and (host[guard + 3 * frame:] == 0xA5).all()
    assert (wsh[:guard] == 0xA5).all() and (wsh[guard + nws:] == 0xA5).all()
    assert np.array_equal(host[guard:guard + frame].reshape(h, w, 3), jg.pil_bgr(good))
    assert np.array_equal(host[guard + 2 * frame:guard + 3 * frame].reshape(h, w, 3), jg.pil_bgr(good2))
    p = tmp_path / ("%s.jpg" % kind)
    p.write_bytes(bad)
    with pytest.raises(OSError, match="%s.jpg: corrupt or truncated JPEG data" % kind):
        jpeg.decode_files([good, str(p), good2], dev, progressive=True)


def _mixed_trees(tmp_path):
    """The VOC fixture trees with every other frame re-saved as a progressive file."""
    trees = voc_tree.make_trees(tmp_path)
    for split in ("train", "val"):
        d = os.path.join(trees[split], "img")
        for k, n in enumerate(sorted(os.listdir(d))):
            if k % 2 == 0:
                p = os.path.join(d, n)
                data = resave(open(p, "rb").read(), quality=92, progressive=True)
                os.unlink(p)
                with open(p, "wb") as f:
                    f.write(data)
    return trees


@pytest.mark.parametrize("cache", [None, "device"])
def test_dataset_progressive_device_decode_equals_host_decode(tmp_path, dev, cache):
    from yolo_fastest_amd.dataset import DetectDataset
    trees = _mixed_trees(tmp_path)

    def ds(**kw):
        return DetectDataset([256, 320, 1], [512, 640, 3], LOG, aug_params=voc_tree.aug_params(trees), max_boxes=64, device=dev, cache=cache, **kw)
    host, devd = ds(), ds(decode="device", progressive=True)
    assert host.img_list == devd.img_list
    rng = np.random.default_rng(2)
    for rep in range(2):
        idx = [int(i) for i in rng.integers(0, len(host), size=12)] + list(range(4))
        random.seed(rep)
        a = host.__getitems__(idx)
        random.seed(rep)
        b = devd.__getitems__(idx)
        assert torch.equal(a.imgs, b.imgs) and torch.equal(a.targets, b.targets)
        for i in idx[-4:]:
            random.seed(100 + i)
            ia, ba = host[i]
            random.seed(100 + i)
            ib, bb = devd[i]
            assert np.array_equal(ia, ib) and np.array_equal(ba, bb)
    # four items of which at least one IS a progressive file: the list's order is os.listdir's (the file system's), so the first four alone
    # can all be baseline files (11 of the 23 are), and then nothing is refused
    from PIL import Image
    prog = [i for i, p in enumerate(host.img_list) if Image.open(p).info.get("progressive")]
    assert 0 < len(prog) < len(host.img_list)
    with pytest.raises(ValueError, match=r"progressive JPEG \(SOF2\) is not supported"):
        ds(decode="device").__getitems__([prog[0]] + [i for i in range(4) if i != prog[0]][:3])


def test_batch_detect_on_a_directory_that_mixes_kinds(dev, tmp_path):
    import yolo_fastest_amd as yf
    from PIL import Image
    src = tmp_path / "src"
    src.mkdir()
    for k, n in enumerate(sorted(os.listdir(GOLDEN_DIR))):
        d = open(os.path.join(GOLDEN_DIR, n), "rb").read()
        (src / n).write_bytes(resave(d, quality=92, progressive=True) if k % 3 else d)

    def run(decode, **kw):
        lines = []

        class H(logging.Handler):
            def emit(self, rec):
                lines.append(rec.getMessage())
        logger = logging.getLogger("yf-jpeg-prog-batch-detect-%s" % decode)
        logger.setLevel(logging.INFO)
        logger.addHandler(H())
        logger.propagate = False
        det = yf.Detect_YOLO(dev, os.path.join(WDIR, "yolo_fastest_256x320_epoch28.pth"), {"io_params": yf.io_params_for(256)}, logger,
                             decode=decode, **kw)
        out = tmp_path / decode
        out.mkdir()
        det.batch_detect(str(src), str(out), batch_size=8, in_flight=2)
        return lines, det.last_labels
    lh, labels_h = run("host")
    ld, labels_d = run("device", progressive=True)
    assert len(lh) == len(ld) == 21
    pat = re.compile(r"^image_name:(\S+) -> (detect finished|no targets), infer time")
    for a, b in zip(lh[:20], ld[:20]):
        assert pat.match(a).groups() == pat.match(b).groups(), (a, b)
    assert labels_h == labels_d and len(labels_d) == 20
    for name in sorted(os.listdir(tmp_path / "host")):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "host" / name)), np.asarray(Image.open(tmp_path / "device" / name))), name
        assert open(tmp_path / "host" / name, "rb").read() == open(tmp_path / "device" / name, "rb").read(), name
    shutil.rmtree(tmp_path / "device")


def test_one_large_frame(jpeg, dev):
    """One textured 4:2:0 frame, Pillow's script, no restart markers: ten serial chains of one lane each.  The size: 2048 x 2048 first;
    8192 x 8192 only if the measured 2048 x 2048 call times 16 stays under a fifth of LARGE_LIMIT_S (120 s), i.e. under 24 s.
    Measured on an MI355X: 2048 x 2048 (an 888 kB file) 1.40 s in one call, times 16 = 22.4 s < 24 s, so the size used was
    8192 x 8192 (a 14.1 MB file): 23.5 s in one call, the whole test well inside its limit.  (An earlier build took 1.97 s at
    2048 x 2048 and stayed there; both sizes are checked for every byte when they run.)"""
    def one(n):
        a = jw.textured(n, n, 4)
        d = jg.encode(a, "420", quality=90, progressive=True)
        blob, h, w = jpeg.pack([d], progressive=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        bgr, st = jpeg.decode_blob(blob, h, w, dev)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        assert int(st.cpu()[0]) == 0
        assert np.array_equal(bgr[0].cpu().numpy(), jg.pil_bgr(d))
        return dt, len(d)
    t_start = time.perf_counter()
    one(64)                                               # first-call costs stay out of the timing
    dt, nbytes = one(2048)
    print("large frame: 2048 x 2048, %d file bytes, one call %.1f ms" % (nbytes, dt * 1e3))
    if dt * 16 < LARGE_LIMIT_S / 5:
        dt2, nbytes2 = one(8192)
        print("large frame: 8192 x 8192, %d file bytes, one call %.1f ms" % (nbytes2, dt2 * 1e3))
    assert time.perf_counter() - t_start < LARGE_LIMIT_S
