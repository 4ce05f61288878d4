"""jpeg.encode_frames / encode_batch (csrc/yf_jpeg_enc_kernels.hip) against the installed Pillow, byte for byte: every case of
tests/test_cpu_jpeg_enc.py, both channel orders, gray, batches of 1, 2, 64 and 257 frames, decode -> encode on the bundled files, the
overflow protocol and graph capture.  Nothing here compares the device with itself."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_cpu_jpeg_enc as cases  # noqa: E402
from test_cpu_jpeg_enc import DATA, FILES, PATTERNS, QUALITIES, SIZES, SUBS, pattern, pil_bytes  # noqa: E402


@pytest.fixture(scope="module")
def jpeg():
    from yolo_fastest_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def up(dev, *arrays):
    return torch.from_numpy(np.stack(arrays)).to(dev)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("size", SIZES)
def test_every_padding_case_with_every_subsampling(jpeg, dev, size, sub):
    k = SIZES.index(size) + SUBS.index(sub)
    for j, q in enumerate((QUALITIES[k % 8], QUALITIES[(k + 3) % 8], 95)):
        a = pattern("noise", size[0], size[1], 3, seed=k + j)
        want = pil_bytes(a, q, sub)
        assert jpeg.encode_frames(up(dev, a), q, sub, order="rgb") == [want], (size, sub, q)
        assert jpeg.encode_frames(up(dev, np.ascontiguousarray(a[:, :, ::-1])), q, sub, order="bgr") == [want], (size, sub, q)


@pytest.mark.parametrize("pat", PATTERNS)
@pytest.mark.parametrize("quality", QUALITIES)
def test_patterns_at_every_quality(jpeg, dev, pat, quality):
    for (h, w), sub in (((37, 53), SUBS[quality % 3]), ((16, 17), SUBS[(quality + 1) % 3]), ((64, 48), "4:2:0")):
        a = pattern(pat, h, w, 3, seed=quality)
        assert jpeg.encode_frames(up(dev, a), quality, sub, order="rgb") == [pil_bytes(a, quality, sub)], (pat, quality, h, w, sub)
    g = pattern(pat, 37, 53, 1, seed=quality)
    assert jpeg.encode_frames(up(dev, g), quality) == [pil_bytes(g, quality)]


@pytest.mark.parametrize("size", SIZES)
def test_gray_at_every_size(jpeg, dev, size):
    for q, pat in ((95, "noise"), (100, "checker"), (50, "hramp")):
        g = pattern(pat, size[0], size[1], 1, seed=size[0])
        assert jpeg.encode_frames(up(dev, g), q) == [pil_bytes(g, q)], (size, q, pat)


def test_bundled_frames_plain_and_drawn_on_in_one_batch(jpeg, dev):
    from yolo_fastest_amd.plot import plot_one_box
    frames = [cases.frame(n) for n in FILES]
    drawn = []
    for k, a in enumerate(frames):
        b = a.copy()
        plot_one_box([40 + 9 * k, 60 + 7 * k, 300 + 5 * k, 280 + 3 * k], b, label="cloud 0.%02d" % k, color=[106, 90, 205], line_thickness=3)
        drawn.append(b)
    both = frames + drawn
    got = jpeg.encode_frames(up(dev, *both), 95, "4:2:0", order="rgb")
    assert got == [pil_bytes(a, 95) for a in both]


def test_decode_then_encode_on_the_bundled_files(jpeg, dev):
    paths = [os.path.join(DATA, n) for n in FILES]
    groups = jpeg.decode_files(paths, dev)
    assert len(groups) == 1 and groups[0].positions == list(range(len(FILES)))
    got = jpeg.encode_frames(groups[0].bgr)                       # the defaults: quality 95, 4:2:0, BGR as the decoder hands out
    assert got == [pil_bytes(np.asarray(Image.open(p).convert("RGB")), 95) for p in paths]


@pytest.mark.parametrize("n", [1, 2, 64, 257])
def test_a_frames_bytes_do_not_depend_on_its_batch(jpeg, dev, n):
    rng = np.random.default_rng(n)
    base = [pattern("noise", 40, 56, 3, seed=s) for s in range(5)] + [pattern(p, 40, 56, 3) for p in PATTERNS[1:]]
    want = [pil_bytes(a, 90, "4:2:0") for a in base]
    pick = [int(i) for i in rng.integers(0, len(base), n)]
    got = jpeg.encode_frames(up(dev, *[base[i] for i in pick]), 90, "4:2:0", order="rgb")
    assert got == [want[i] for i in pick]
    gray = [pattern("noise", 33, 47, 1, seed=s) for s in range(4)]
    pick = [int(i) for i in rng.integers(0, 4, n)]
    assert jpeg.encode_frames(up(dev, *[gray[i] for i in pick]), 75) == [pil_bytes(gray[i], 75) for i in pick]


def test_overflow_sets_the_flag_and_the_needed_length_and_touches_nothing(jpeg, dev):
    big = pattern("noise", 64, 64, 3)                            # tests/test_cpu_jpeg_enc.py: outgrows 64 * 64 * 3 + 1024 at quality 100
    small = pattern("flat128", 64, 64, 3)
    want = [pil_bytes(big, 100, "4:4:4"), pil_bytes(small, 100, "4:4:4"), pil_bytes(big, 100, "4:4:4")]
    assert len(want[0]) > 64 * 64 * 3 + 1024 > len(want[1])
    frames = up(dev, big, small, big)
    stride = 64 * 64 * 3 + 1024
    out = torch.full((4, stride), 0xA5, dtype=torch.uint8, device=dev)   # a fourth slot behind the last frame's
    buf, lengths, status = jpeg.encode_batch(frames, 100, "4:4:4", order="rgb", out=out[:3])
    torch.cuda.synchronize()
    assert status.tolist() == [1, 0, 1] and lengths.tolist() == [len(w) for w in want]
    host = out.cpu().numpy()
    assert (host[0] == 0xA5).all() and (host[2] == 0xA5).all() and (host[3] == 0xA5).all()
    assert host[1, :len(want[1])].tobytes() == want[1] and (host[1, len(want[1]):] == 0xA5).all()
    # the smallest stride that fits and the largest that does not
    for stride, st in ((len(want[0]), 0), (len(want[0]) - 1, 1)):
        out = torch.full((2, stride), 0x5A, dtype=torch.uint8, device=dev)
        _, lengths, status = jpeg.encode_batch(frames[:1], 100, "4:4:4", order="rgb", out=out[:1], stride=stride)
        assert status.tolist() == [st] and lengths.tolist() == [len(want[0])]
        host = out.cpu().numpy()
        assert (host[1] == 0x5A).all()
        assert host[0].tobytes() == want[0] if st == 0 else (host[0] == 0x5A).all()
    assert jpeg.encode_frames(frames, 100, "4:4:4", order="rgb") == want          # one repeat with the needed size
    assert jpeg.encode_frames(frames, 100, "4:4:4", order="rgb", stride=700) == want


def test_what_is_not_built_is_refused_before_any_launch(jpeg, dev):
    a = up(dev, pattern("noise", 8, 8, 3))
    for kw in (dict(quality=0), dict(quality=101), dict(quality=95.0), dict(subsampling="4:1:1"), dict(subsampling=2), dict(optimize=True),
               dict(progressive=True), dict(order="gbr")):
        with pytest.raises(ValueError):
            jpeg.encode_frames(a, **kw)
    for bad in (a.float(), a.cpu(), a[..., :2], a[0, 0], torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=dev),
                torch.zeros((1, 8, 8193), dtype=torch.uint8, device=dev), torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            jpeg.encode_frames(bad)


def test_encode_batch_is_capturable_and_replays_on_new_pixels(jpeg, dev):
    h, w, n = 48, 72, 3
    first = [pattern("noise", h, w, 3, seed=s) for s in range(n)]
    second = [pattern("noise", h, w, 3, seed=100 + s) for s in range(n - 1)] + [pattern("checker", h, w, 3)]
    frames = up(dev, *first)
    s = jpeg.enc_setup(h, w, 3, 95, "4:2:0")
    stride = h * w * 3 + 1024
    _, _, _ = jpeg.encode_batch(frames, order="rgb", setup=s)     # warm-up outside the capture (module load)
    ws = torch.empty(jpeg.enc_workspace_bytes(s, n), dtype=torch.uint8, device=dev)
    out = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    lengths = torch.zeros((n,), dtype=torch.int32, device=dev)
    status = torch.zeros((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        jpeg.encode_batch(frames, order="rgb", setup=s, workspace=ws, out=out, lengths=lengths, status=status)
    for arrays in (first, second, first):
        frames.copy_(torch.from_numpy(np.stack(arrays)))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert status.tolist() == [0] * n
        assert jpeg.gather_files(out, lengths.tolist()) == [pil_bytes(a, 95) for a in arrays]
