"""DetectDataset's opt-in mosaic on the host (dataset.py: draw_mosaic): the yardstick (tests/mosaic_ref.py over
tests/warp_ref.py) against Pillow on materialised canvases, the neutral warp, the kernel's per-pixel canvas rule, the draw order, the
labels against yolov5's restated arithmetic, the unchanged defaults, the constructor's refusals, and the C entry.  No GPU needed.
Pixels compare bit for bit; labels compare exactly (float64, the same operations)."""
import ctypes
import logging
import math
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mosaic_ref  # noqa: E402
import voc_tree  # noqa: E402
import warp_ref  # noqa: E402
from yolo_fastest_amd import _lib  # noqa: E402
from yolo_fastest_amd.dataset import DetectDataset, mosaic_placement  # noqa: E402

LOG = logging.getLogger("test-dataset-mosaic")
ACTIVE = dict(degrees=10.0, translate=0.1, scale=1.3, shear=2.0, perspective=0.0005, flipud=0.5)
SIZES = [(37, 45, 1), (37, 45, 3), (16, 20, 1)]


@pytest.fixture()
def trees(tmp_path):
    return voc_tree.make_trees(tmp_path)


def _ds(trees, max_boxes=64, flag=True, augment=True, shape=(256, 320, 1), **keys):
    ap = voc_tree.aug_params(trees)
    ap.update(keys)
    kw = dict(mosaic=True) if flag else {}
    ds = DetectDataset(list(shape), [512, 640, 3], LOG, aug_params=ap, max_boxes=max_boxes, device="cpu", augment=augment, **kw)
    ds.img_list.sort()                               # os.listdir's order varies by machine: the seeds below meet the same items everywhere
    return ds


def _index(ds, stem):
    return [os.path.splitext(os.path.basename(p))[0] for p in ds.img_list].index(stem)


def _tiles(rng, H, W, C):
    """Four tiles: random, a ramp, random, constant 255 (so that a seam towards 114 and one between tiles both show)."""
    shape = (H, W) if C == 1 else (H, W, C)
    ramp = np.broadcast_to((np.arange(W) * 255 // (W - 1)).astype(np.uint8).reshape((1, W) + (1,) * (len(shape) - 2)), shape)
    return [rng.integers(0, 256, size=shape, dtype=np.uint8), np.ascontiguousarray(ramp), rng.integers(0, 256, size=shape, dtype=np.uint8),
            np.full(shape, 255, np.uint8)]


def _matrix(H, W, persp, degrees, gain, shear, shift):
    """yolov5's M = T S R P C for the mosaic: C moves the canvas centre (W, H) to the origin, T is in units of the output."""
    C = np.eye(3); C[0, 2], C[1, 2] = -W, -H
    P = np.eye(3); P[2, 0], P[2, 1] = (0.12 / W, -0.08 / H) if persp else (0.0, 0.0)
    a = math.radians(degrees)
    R = np.eye(3); R[:2, :2] = [[gain * math.cos(a), gain * math.sin(a)], [-gain * math.sin(a), gain * math.cos(a)]]
    S = np.eye(3); S[0, 1], S[1, 0] = math.tan(math.radians(shear[0])), math.tan(math.radians(shear[1]))
    T = np.eye(3); T[0, 2], T[1, 2] = (0.5 + shift[0]) * W, (0.5 + shift[1]) * H
    return T @ S @ R @ P @ C


def _warps(H, W):
    """-> [(name, coeffs, perspective)]: neutral, affine, perspective, gain 0.5 (canvas border and fill visible), gain 1.5."""
    out = [("neutral", mosaic_ref.neutral_coeffs(H, W), False)]
    for name, persp, deg, gain, shear, shift in (("affine", False, 10.0, 1.1, (5.0, -3.0), (0.04, -0.03)),
                                                 ("perspective", True, -7.5, 0.8, (0.0, 2.0), (-0.05, 0.02)),
                                                 ("gain0.5", False, 3.0, 0.5, (0.0, 0.0), (0.1, -0.1)),
                                                 ("gain1.5", True, -4.0, 1.5, (1.0, 1.0), (0.0, 0.05))):
        c = warp_ref.coeffs_of(_matrix(H, W, persp, deg, gain, shear, shift))
        if not persp:
            c[6:] = 0.0
        out.append((name, c, persp))
    return out


def _centres(H, W):
    """Both extremes of each draw range (int(uniform(a, b)) lies in a .. b; b itself only by rounding), (W, H), and off-centre."""
    lo_x, hi_x, lo_y, hi_y = W // 2, 2 * W - W // 2, H // 2, 2 * H - H // 2
    return [(lo_x, lo_y), (hi_x, hi_y), (lo_x, hi_y), (hi_x, lo_y), (W, H), (W - 3, H + 5), (W + 7, H - 2)]


# ---- 1. the yardstick against Pillow ----
@pytest.mark.parametrize("size", SIZES)
def test_yardstick_equals_pillow_on_canvases(size):
    H, W, C = size
    tiles = _tiles(np.random.default_rng(H + C), H, W, C)
    n = 0
    for xc, yc in _centres(H, W):
        canvas = mosaic_ref.canvas_u8(tiles, xc, yc)
        assert canvas.shape[:2] == (2 * H, 2 * W)
        for name, c, persp in _warps(H, W):
            got = warp_ref.transform_u8(canvas, c, persp, size=(H, W))
            want = warp_ref.pil_transform_u8(canvas, c, persp, size=(H, W))
            assert got.shape == want.shape == (H, W) + canvas.shape[2:]
            assert np.array_equal(got, want), (xc, yc, name, int((got != want).sum()))
            if name == "gain0.5":
                assert (want == mosaic_ref.FILL).any()                          # the border beyond the canvas is in view
            for k, fl, fu in ((0, False, False), (3, True, False), (7, False, True)):
                a = mosaic_ref.compose_u8(tiles, xc, yc, c, persp, k, fl, fu, transform=warp_ref.transform_u8)
                b = mosaic_ref.compose_u8(tiles, xc, yc, c, persp, k, fl, fu)
                assert np.array_equal(a, b)
            n += 1
    assert n == 35


# ---- 2. the neutral warp is the central crop ----
def test_neutral_warp_is_the_central_crop_at_an_even_size():
    H, W = 16, 20
    tiles = _tiles(np.random.default_rng(1), H, W, 1)
    M = _matrix(H, W, False, 0.0, 1.0, (0.0, 0.0), (0.0, 0.0))
    c = warp_ref.coeffs_of(M)
    assert np.array_equal(c, mosaic_ref.neutral_coeffs(H, W))
    for xc, yc in _centres(H, W):
        canvas = mosaic_ref.canvas_u8(tiles, xc, yc)
        for transform in (warp_ref.transform_u8, warp_ref.pil_transform_u8):
            got = transform(canvas, c, False, size=(H, W))
            assert np.array_equal(got, canvas[H // 2:H // 2 + H, W // 2:W // 2 + W])


# ---- 3. the kernel's per-pixel rule is the canvas ----
def test_per_pixel_rule_reproduces_the_canvas_for_every_centre_in_range():
    H, W = 16, 20
    tiles = _tiles(np.random.default_rng(2), H, W, 1)
    cy, cx = np.meshgrid(np.arange(2 * H), np.arange(2 * W), indexing="ij")
    for yc in range(H // 2, 2 * H - H // 2 + 1):
        for xc in range(W // 2, 2 * W - W // 2 + 1):
            canvas = mosaic_ref.canvas_u8(tiles, xc, yc)
            # vectorised: the quadrant's rectangle and pads per pixel
            got = np.full_like(canvas, mosaic_ref.FILL)
            for q in range(4):
                (x1a, y1a, x2a, y2a), (x1b, y1b, x2b, y2b) = mosaic_ref.placement(q, xc, yc, H, W)
                assert (x1a, y1a, x2a, y2a, x1b, y1b, x2b, y2b) == mosaic_placement(q, xc, yc, H, W)
                assert x2a - x1a == x2b - x1b and y2a - y1a == y2b - y1b and 0 <= x1b <= x2b <= W and 0 <= y1b <= y2b <= H
                mine = ((cx >= xc) == bool(q & 1)) & ((cy >= yc) == bool(q & 2))
                inside = mine & (cx >= x1a) & (cx < x2a) & (cy >= y1a) & (cy < y2a)
                padw, padh = x1a - x1b, y1a - y1b
                got[inside] = tiles[q][(cy - padh)[inside], (cx - padw)[inside]]
            assert np.array_equal(got, canvas), (xc, yc)
    # and pixel by pixel through mosaic_ref.canvas_px, at the corner centres and an inner one
    for xc, yc in ((W // 2, H // 2), (2 * W - W // 2, 2 * H - H // 2), (W + 3, H - 5)):
        canvas = mosaic_ref.canvas_u8(tiles, xc, yc)
        assert all(canvas[y, x] == mosaic_ref.canvas_px(tiles, xc, yc, x, y) for y in range(2 * H) for x in range(2 * W))


# ---- 4. the draw order ----
def _replay(ds, i, p):
    """The documented sequence by hand -> (hit, xc, yc, tiles, canvas coeffs or frame coeffs, k, fliplr, flipud)."""
    H, W = ds.input_shape[:2]
    xc = yc = tiles = None
    hit = random.random() < p                                                      # 1.
    if hit:
        yc = int(random.uniform(H // 2, 2 * H - H // 2))                           # 2. yc first
        xc = int(random.uniform(W // 2, 2 * W - W // 2))
        tiles = [i] + random.choices(range(len(ds)), k=3)                          # 3.
        random.shuffle(tiles)
        coeffs = ds._draw_warp(mosaic=True)[2]                                     # 4. always
    else:
        coeffs = ds._draw_warp()[2] if ds.geometric else None                      # draw_mix's step 1
    k = 0
    if random.random() < ds.gussian_filter:                                        # 5.
        k = 7 if random.random() < 0.4 else 3
    fl = random.random() < ds.fliplr
    fu = ds.flipud > 0 and random.random() < ds.flipud
    return hit, xc, yc, tiles, coeffs, k, fl, fu


@pytest.mark.parametrize("keys", [{}, ACTIVE], ids=["neutral", "geometric"])
@pytest.mark.parametrize("p", [1.0, 0.5])
def test_draw_order(trees, keys, p):
    ds = _ds(trees, mosaic=p, **keys)
    H, W = ds.input_shape[:2]
    assert ds.geometric == bool(keys) and ds.mosaic == p
    hits = 0
    for i in range(len(ds)):
        random.seed(70 + i)
        rec = ds.draw_mosaic(i)
        end = random.getstate()
        random.seed(70 + i)
        hit, xc, yc, tiles, coeffs, k, fl, fu = _replay(ds, i, p)
        assert random.getstate() == end
        assert len(rec) == 9 and (rec[0], rec[1], rec[3]) == (k, fl, fu) and rec[5:8] == (None, None, None)
        hits += hit
        if hit:
            assert rec[4] is None and rec[8][:3] == (xc, yc, tiles) and np.array_equal(rec[8][3], coeffs)
            assert W // 2 <= xc <= 2 * W - W // 2 and H // 2 <= yc <= 2 * H - H // 2 and i in tiles and len(tiles) == 4
            if not keys:
                assert np.array_equal(coeffs, mosaic_ref.neutral_coeffs(H, W))     # eight draws over empty ranges: the central crop
        else:
            assert rec[8] is None and ((coeffs is None and rec[4] is None) or np.array_equal(rec[4], coeffs))
        for fn, n in ((ds.draw_mix, 8), (ds.draw_ex, 5), (ds.draw, 3)):             # the older entries: the same draws, their own lengths
            random.seed(70 + i)
            short = fn(i)
            assert random.getstate() == end and len(short) == n and np.array_equal(short[2], rec[2])
    assert hits == len(ds) if p == 1.0 else 0 < hits < len(ds)


# ---- 5. labels ----
def _want_targets(ds, rec, M, gain):
    xc, yc, tiles, _ = rec[8]
    H, W = ds.input_shape[:2]
    rows = mosaic_ref.mosaic_labels([ds._labels(t) for t in tiles], xc, yc, H, W, M, gain)
    return rows, mosaic_ref.targets_of(rows, rec[1], rec[3], ds.max_boxes)


@pytest.mark.parametrize("keys", [{}, ACTIVE], ids=["neutral", "geometric"])
def test_labels_equal_yolov5s_arithmetic(trees, monkeypatch, keys):
    ds = _ds(trees, max_boxes=16, mosaic=1.0, **keys)
    crowd, empty = _index(ds, "syn_crowd"), _index(ds, "syn_empty")
    real, seen = ds._draw_warp, []

    def spy(mosaic=False):
        seen.append((mosaic, real(mosaic=mosaic)))
        return seen[-1][1]
    monkeypatch.setattr(ds, "_draw_warp", spy)
    truncated = with_empty = kept = 0
    flips = set()
    for n_th, i in enumerate(list(range(len(ds))) + [crowd] * 6 + [empty] * 6):
        del seen[:]
        random.seed(500 + n_th)
        rec = ds.draw_mosaic(i)
        assert len(seen) == 1 and seen[0][0] is True
        M, gain, coeffs = seen[0][1]
        assert np.array_equal(coeffs, rec[8][3])
        rows, want = _want_targets(ds, rec, M, gain)
        assert np.array_equal(rec[2], want), i
        n = min(len(rows), 16)
        assert (rec[2][:n, 5] == 255.0).all() and not rec[2][n:].any()
        if n:
            b = rec[2][:n]
            assert (b[:, 0] - b[:, 2] / 2 > -1e-12).all() and (b[:, 0] + b[:, 2] / 2 < 1 + 1e-12).all()      # inside the output
            assert (b[:, 2] * ds.input_shape[1] > 2).all() and (b[:, 3] * ds.input_shape[0] > 2).all()
        truncated += len(rows) > 16
        with_empty += empty in rec[8][2]
        kept += n
        flips.add((rec[1], rec[3]))
    assert truncated > 0 and with_empty > 0 and kept > 0
    assert len(flips) == (4 if keys else 2)
    assert len(ds._labels(empty)) == 0 and len(ds._labels(crowd)) > 64


def test_more_rows_than_max_boxes_drops_the_last_and_an_empty_tile_adds_none(trees, monkeypatch):
    ds = _ds(trees, max_boxes=8, mosaic=1.0)
    crowd, empty = _index(ds, "syn_crowd"), _index(ds, "syn_empty")
    H, W = ds.input_shape[:2]
    monkeypatch.setattr(ds, "fliplr", 0.0)
    monkeypatch.setattr(random, "shuffle", lambda x: None)                         # the item stays top-left
    monkeypatch.setattr(random, "uniform", lambda a, b: (a + b) / 2)               # centre (W, H): every tile whole; neutral warp
    M = _matrix(H, W, False, 0.0, 1.0, (0.0, 0.0), (0.0, 0.0))
    for others in ([crowd, crowd, crowd], [empty, crowd, empty], [empty, empty, empty]):
        monkeypatch.setattr(random, "choices", lambda pop, k, others=others: list(others))
        for item in (crowd, empty, 0):
            rec = ds.draw_mosaic(item)
            assert rec[8][:3] == (W, H, [item] + others)
            rows, want = _want_targets(ds, rec, M, 1.0)
            assert np.array_equal(rec[2], want)
            # tile by tile: an empty tile contributes nothing, the others their rows in tile order
            per = [mosaic_ref.mosaic_labels([ds._labels(t) if q == j else [] for j in range(4)], W, H, H, W, M, 1.0)
                   for q, t in enumerate(rec[8][2])]
            assert np.array_equal(np.concatenate(per), rows)
            assert all(len(per[q]) == 0 for q, t in enumerate(rec[8][2]) if t == empty)
            if len(rows) > 8:
                assert np.array_equal(rec[2][:, :4], rows[:8, 1:5]) and (rec[2][:, 5] == 255.0).all()
            else:
                assert not rec[2][len(rows):].any()
    # all four tiles empty: all-zero boxes
    monkeypatch.setattr(random, "choices", lambda pop, k: [empty] * 3)
    assert not ds.draw_mosaic(empty)[2].any()


# ---- 6. the defaults are unchanged ----
@pytest.mark.parametrize("keys", [{}, ACTIVE], ids=["neutral", "geometric"])
def test_without_the_flag_or_with_probability_zero_nothing_changes(trees, keys):
    base = _ds(trees, flag=False, **keys)                                          # voc_tree's params carry no "mosaic" key: today's
    assert "mosaic" not in base.aug_params
    unread, zero, absent = _ds(trees, flag=False, mosaic=0.9, **keys), _ds(trees, mosaic=0.0, **keys), _ds(trees, **keys)
    assert unread.mosaic == 0.0 and zero.mosaic == 0.0 and absent.mosaic == 0.0
    for ds in (unread, zero, absent):
        random.seed(9)
        want = [base.draw_mix(i) for i in range(len(base))]                        # a whole epoch, one stream
        end = random.getstate()
        random.seed(9)
        got = [ds.draw_mosaic(i) for i in range(len(ds))]
        assert random.getstate() == end
        for g, w in zip(got, want):
            assert len(g) == 9 and g[8] is None and g[:2] == w[:2] and g[3] == w[3] and g[5:8] == w[5:8]
            assert np.array_equal(g[2], w[2]) and ((g[4] is None and w[4] is None) or np.array_equal(g[4], w[4]))
        random.seed(9)
        assert all(np.array_equal(ds.draw(i)[2], w[2]) for i, w in enumerate(want)) and random.getstate() == end


def _warp_labels_as_it_was(labels, M, gain, H, W):
    """_warp_labels before it was split around _warp_boxes, restated: normalised rows in, normalised kept rows out."""
    x1, x2 = (labels[:, 1] - labels[:, 3] / 2) * W, (labels[:, 1] + labels[:, 3] / 2) * W
    y1, y2 = (labels[:, 2] - labels[:, 4] / 2) * H, (labels[:, 2] + labels[:, 4] / 2) * H
    n = len(labels)
    xy = np.ones((n * 4, 3))
    xy[:, 0] = np.stack([x1, x2, x1, x2], 1).reshape(-1)
    xy[:, 1] = np.stack([y1, y2, y2, y1], 1).reshape(-1)
    xy = xy @ M.T
    xy = (xy[:, :2] / xy[:, 2:3]).reshape(n, 4, 2)
    nx1, nx2 = xy[:, :, 0].min(1).clip(0, W), xy[:, :, 0].max(1).clip(0, W)
    ny1, ny2 = xy[:, :, 1].min(1).clip(0, H), xy[:, :, 1].max(1).clip(0, H)
    w1, h1 = (x2 - x1) * gain, (y2 - y1) * gain
    w2, h2 = nx2 - nx1, ny2 - ny1
    ar = np.maximum(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16))
    keep = (w2 > 2) & (h2 > 2) & (w2 * h2 / (w1 * h1 + 1e-16) > 0.1) & (ar < 20)
    out = labels.copy()
    out[:, 1], out[:, 2], out[:, 3], out[:, 4] = (nx1 + nx2) / 2 / W, (ny1 + ny2) / 2 / H, w2 / W, h2 / H
    return out[keep]


def test_warp_labels_keeps_its_values_around_the_pixel_core(trees):
    """_warp_labels, now a wrapper of the pixel-coordinate core _warp_boxes, returns what the unsplit function returned, and what the
    mosaic arithmetic gives for a single tile with zero pads."""
    ds = _ds(trees, flag=False, **ACTIVE)
    H, W = ds.input_shape[:2]
    random.seed(4)
    rows_seen = dropped = 0
    for i in list(range(len(ds))) * 3:
        lab = ds._labels(i)
        M, gain, _ = ds._draw_warp()
        if not len(lab):
            continue
        got = ds._warp_labels(lab, M, gain)
        assert np.array_equal(got, _warp_labels_as_it_was(lab, M, gain, H, W))
        # a frame's rows through the mosaic arithmetic with a zero pad (tile BR at centre (0, 0)): the same boxes, the canvas clip idle
        assert np.array_equal(mosaic_ref.mosaic_labels([[], [], [], lab], 0, 0, H, W, M, gain), got)
        rows_seen += len(got)
        dropped += len(lab) - len(got)
    assert rows_seen > 0 and dropped > 0


# ---- 7. refusals ----
@pytest.mark.parametrize("p", [-0.1, 1.5])
def test_constructor_refuses_a_probability_outside_0_1_only_with_the_flag(trees, p):
    with pytest.raises(ValueError, match="mosaic"):
        _ds(trees, mosaic=p)
    assert _ds(trees, flag=False, mosaic=p).mosaic == 0.0
    assert _ds(trees, mosaic=1.0).mosaic == 1.0
    assert _ds(trees, mosaic=1.0, augment=False).draw_mosaic(0)[8] is None         # no augmentation: no draw at all


def test_constructor_refuses_mosaic_with_mixup(trees):
    ap = dict(voc_tree.aug_params(trees), mosaic=0.5, mixup=0.5)

    def mk(keys=None, **kw):
        return DetectDataset([256, 320, 1], [512, 640, 3], LOG, aug_params=dict(ap, **(keys or {})), device="cpu", **kw)
    with pytest.raises(ValueError, match="mosaic.*mixup"):
        mk(mosaic=True, mixup=True)
    assert mk(mosaic=True).mosaic == 0.5 and mk(mixup=True).mixup == 0.5           # each alone
    both = mk(mosaic=True, mixup=True, keys=dict(mixup=0.0))                       # one probability zero: allowed
    assert both.mosaic == 0.5 and both.mixup == 0.0
    both = mk(mosaic=True, mixup=True, keys=dict(mosaic=0.0))
    assert both.mosaic == 0.0 and both.mixup == 0.5


# ---- 8. the C entry ----
def test_library_exports_the_mosaic_entry_and_lib_declares_it():
    assert "yf_augment_mosaic_u8" in _lib.EXPORTS
    lib = _lib.lib()
    fn = lib.yf_augment_mosaic_u8
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert lib.yf_abi_version() == _lib.ABI_VERSION == 1
    with open(os.path.join(os.path.dirname(HERE), "include", "yolo_fastest_hip.h")) as f:
        assert "int yf_augment_mosaic_u8(int device, const uint8_t *d_frames, int n_frames, int N, int h, int w, int c," in f.read()


def test_mosaic_entry_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)                      # never read: every call below is refused before a launch
    good = dict(d_frames=ptr, n_frames=4, N=2, h=16, w=20, c=1, d_tiles=ptr, d_centre=ptr, d_params=ptr, d_warp=ptr, d_u8=ptr, d_x=ptr)

    def call(**change):
        a = dict(good, **change)
        return lib.yf_augment_mosaic_u8(0, a["d_frames"], a["n_frames"], a["N"], a["h"], a["w"], a["c"], a["d_tiles"], a["d_centre"],
                                        a["d_params"], a["d_warp"], a["d_u8"], a["d_x"], None)
    bad = [dict(d_frames=None), dict(d_tiles=None), dict(d_centre=None), dict(d_params=None), dict(d_warp=None), dict(d_u8=None, d_x=None),
           dict(N=0), dict(N=-1), dict(n_frames=0), dict(n_frames=-3), dict(c=2), dict(c=0), dict(c=4), dict(h=0), dict(h=-1), dict(h=16385),
           dict(w=0), dict(w=-1), dict(w=16385)]
    for change in bad:
        assert call(**change) == _lib.YF_E_INVALID, change
        assert b"yf_augment_mosaic_u8" in lib.yf_last_error_string()
    with pytest.raises(_lib.YFError, match="yf_augment_mosaic_u8"):
        _lib.check(call(c=2))
