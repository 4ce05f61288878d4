"""DetectDataset's opt-in mixup on the host (dataset.py: draw_mix): the blend's reference (tests/mix_ref.py) against
yolov5's literal expression, the draw order, the merged labels, the batch's draws, the constructor's range check, and the argument checks
of yf_augment_mix_u8, which return before the GPU is touched.  No GPU needed."""
import ctypes
import logging
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mix_ref  # noqa: E402
import voc_tree  # noqa: E402
from yolo_fastest_amd import _lib  # noqa: E402
from yolo_fastest_amd.dataset import DetectDataset  # noqa: E402

LOG = logging.getLogger("test-dataset-mixup")
ACTIVE = dict(degrees=10.0, translate=0.1, scale=1.3, shear=2.0, perspective=0.0005, flipud=0.5)
R127 = 0.4809054919537687          # 127 * r + 127 * (1 - r) rounds to just below 127: the byte is 126


@pytest.fixture()
def trees(tmp_path):
    return voc_tree.make_trees(tmp_path)


def _ds(trees, max_boxes=64, absent=(), flag=True, augment=True, **keys):
    ap = voc_tree.aug_params(trees)
    for k in absent:
        del ap[k]
    ap.update(keys)
    kw = dict(mixup=True) if flag else {}
    return DetectDataset([256, 320, 1], [512, 640, 3], LOG, aug_params=ap, max_boxes=max_boxes, device="cpu", augment=augment, **kw)


def _index(ds, stem):
    return [os.path.splitext(os.path.basename(p))[0] for p in ds.img_list].index(stem)


def _bundled(ds, n):
    """The n-th bundled frame (every one has objects), wherever os.listdir put it."""
    return _index(ds, voc_tree.bundled_stems()[n])


def _rows(ds, i):
    """The reference's normalised rows of item i as draw() lays them out, (xc, yc, w, h, cls, 255), all of them, no draws made."""
    plain = ds._labels(i)
    if not len(plain):
        return np.zeros((0, 6))
    return np.concatenate([plain[:, 1:5], plain[:, 0:1], np.full((len(plain), 1), 255.0)], 1)


# ---- 1. the reference of the blend ----
def test_mix_ref_is_yolov5s_expression():
    rng = np.random.default_rng(0)
    rnd = random.Random(0)
    for shape in ((37, 45), (16, 20, 3)):
        im, im2 = rng.integers(0, 256, size=shape, dtype=np.uint8), rng.integers(0, 256, size=shape, dtype=np.uint8)
        for r in (0.0, 1.0, 0.5, R127, 2.0 ** -60, rnd.betavariate(32.0, 32.0)):
            want = (im * r + im2 * (1 - r)).astype(np.uint8)                       # utils/augmentations.py: mixup
            assert np.array_equal(mix_ref.mix_u8(im, im2, r), want)
            # per byte in Python floats (IEEE double, one rounding per operation), truncated
            flat = [int(float(a) * r + float(b) * (1.0 - r)) for a, b in zip(im.reshape(-1).tolist(), im2.reshape(-1).tolist())]
            assert want.reshape(-1).tolist() == flat
            assert np.array_equal(mix_ref.compose_u8(im, None, im2, None, r, 0, False, False), want)
    a = np.full((4, 4), 127, np.uint8)
    assert (mix_ref.mix_u8(a, a, R127) == 126).all()
    assert (mix_ref.mix_u8(a, a, 0.5) == 127).all()
    assert np.array_equal(mix_ref.compose_u8(a, None, None, None, None, 0, False, False), a)   # no partner: no blend


# ---- 2. flag unset / probability zero: nothing changes ----
def test_without_the_flag_or_with_probability_zero_nothing_changes(trees):
    off0, off9 = _ds(trees, flag=False, mixup=0.0, **ACTIVE), _ds(trees, flag=False, mixup=0.9, **ACTIVE)
    on0, on_absent = _ds(trees, mixup=0.0, **ACTIVE), _ds(trees, absent=("mixup",), **ACTIVE)
    assert off9.mixup == 0.0 and on0.mixup == 0.0 and on_absent.mixup == 0.0
    for i in range(len(off0)):
        recs, states = [], []
        for ds in (off0, off9, on0, on_absent):
            random.seed(i)
            recs.append(ds.draw_mix(i))
            states.append(random.getstate())
        for rec, st in zip(recs[1:], states[1:]):
            assert st == states[0]
            assert rec[:2] == recs[0][:2] and rec[3] == recs[0][3] and np.array_equal(rec[2], recs[0][2]) and np.array_equal(rec[4], recs[0][4])
            assert rec[5:] == (None, None, None)
        random.seed(i)
        ex = off9.draw_ex(i)
        assert len(ex) == 5 and np.array_equal(ex[2], recs[0][2]) and random.getstate() == states[0]


# ---- 3. the draw order ----
@pytest.mark.parametrize("keys", [{}, ACTIVE], ids=["neutral", "geometric"])
def test_draw_order_at_probability_one(trees, keys):
    ds = _ds(trees, mixup=1.0, **keys)
    assert ds.geometric == bool(keys)
    for i in range(len(ds)):
        random.seed(50 + i)
        k, flip, boxes, flipud, coeffs, partner, pcoeffs, r = ds.draw_mix(i)
        end = random.getstate()
        random.seed(50 + i)
        c1 = ds._draw_warp()[2] if ds.geometric else None                       # 1. the item's eight
        assert random.random() < 1.0                                               # 2. the hit
        j = random.randint(0, len(ds) - 1)                                         # 3. the partner
        c2 = ds._draw_warp()[2] if ds.geometric else None                       # 4. the partner's eight
        rr = random.betavariate(32.0, 32.0)                                        # 5. the ratio
        kk = 0
        if random.random() < ds.gussian_filter:                                    # 6. blur?, which blur, fliplr?, [flipud?]
            kk = 7 if random.random() < 0.4 else 3
        fl = random.random() < ds.fliplr
        fu = ds.flipud > 0 and random.random() < ds.flipud
        assert random.getstate() == end
        assert (k, flip, flipud, partner, r) == (kk, fl, fu, j, rr) and 0.0 < r < 1.0
        if ds.geometric:
            assert np.array_equal(coeffs, c1) and np.array_equal(pcoeffs, c2) and not np.array_equal(c1, c2)
        else:
            assert coeffs is None and pcoeffs is None
        random.seed(50 + i)
        ex = ds.draw_ex(i)
        assert random.getstate() == end and len(ex) == 5 and np.array_equal(ex[2], boxes)       # draw_ex: the merged boxes
        random.seed(50 + i)
        d = ds.draw(i)
        assert random.getstate() == end and len(d) == 3 and np.array_equal(d[2], boxes)


def test_a_miss_draws_one_value_and_nothing_else(trees):
    ds, base = _ds(trees, mixup=0.5), _ds(trees, flag=False)
    hits = 0
    for i in range(len(ds)):
        random.seed(i)
        rec = ds.draw_mix(i)
        end = random.getstate()
        random.seed(i)
        hit = random.random() < 0.5
        hits += hit
        assert hit == (rec[5] is not None)
        if not hit:
            want = base.draw_mix(i)                                                # the plain draws, after the one value
            assert random.getstate() == end and rec[:2] == want[:2] and np.array_equal(rec[2], want[2]) and rec[5:] == (None, None, None)
    assert 0 < hits < len(ds)


# ---- 4. labels ----
def _pin(monkeypatch, ds, partner, fliplr, flipud=0.0):
    monkeypatch.setattr(random, "randint", lambda a, b: partner)
    monkeypatch.setattr(ds, "fliplr", fliplr)
    monkeypatch.setattr(ds, "flipud", flipud)


@pytest.mark.parametrize("fliplr,flipud", [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)])
def test_partner_rows_follow_the_items_and_flips_act_on_all(trees, monkeypatch, fliplr, flipud):
    ds = _ds(trees, max_boxes=256, mixup=1.0)
    crowd, empty = _index(ds, "syn_crowd"), _index(ds, "syn_empty")
    b = [_bundled(ds, n) for n in range(6)]
    pairs = [(b[0], b[1]), (b[3], b[3]), (b[2], crowd), (crowd, b[5]), (empty, b[4]), (b[4], empty), (empty, empty)]   # (b[3], b[3]): j == index
    for i, j in pairs:
        _pin(monkeypatch, ds, j, fliplr, flipud)
        random.seed(i)
        k, flip, boxes, ud, coeffs, partner, pcoeffs, r = ds.draw_mix(i)
        assert partner == j and flip == bool(fliplr) and ud == bool(flipud) and coeffs is None and pcoeffs is None
        want = np.concatenate([_rows(ds, i), _rows(ds, j)])
        if flip:
            want[:, 0] = 1 - want[:, 0]
        if ud:
            want[:, 1] = 1 - want[:, 1]
        n = len(want)
        assert n == len(_rows(ds, i)) + len(_rows(ds, j)) and n <= 256
        assert np.array_equal(boxes[:n], want) and not boxes[n:].any()
    assert len(_rows(ds, empty)) == 0 and len(_rows(ds, crowd)) > 64


def test_truncation_keeps_the_items_rows_first(trees, monkeypatch):
    probe = _ds(trees, flag=False)
    crowd = _index(probe, "syn_crowd")
    item = _bundled(probe, 2)
    own = len(_rows(probe, item))
    assert own > 0
    ds = _ds(trees, max_boxes=own + 3, mixup=1.0)
    _pin(monkeypatch, ds, crowd, 0.0)
    boxes = ds.draw_mix(item)[2]
    assert np.array_equal(boxes[:own], _rows(ds, item)) and np.array_equal(boxes[own:], _rows(ds, crowd)[:3])
    _pin(monkeypatch, ds, item, 0.0)                                                  # the crowd as the item: only its rows survive
    boxes = ds.draw_mix(crowd)[2]
    assert np.array_equal(boxes, _rows(ds, crowd)[:own + 3])


def test_partner_rows_get_the_partners_own_warp(trees, monkeypatch):
    ds = _ds(trees, max_boxes=256, mixup=1.0, **ACTIVE)
    crowd, empty = _index(ds, "syn_crowd"), _index(ds, "syn_empty")
    real, seen = ds._draw_warp, []

    def spy():
        seen.append(real())
        return seen[-1]
    monkeypatch.setattr(ds, "_draw_warp", spy)
    b = [_bundled(ds, n) for n in range(5)]
    for i, j in [(b[0], b[1]), (b[3], b[3]), (b[2], crowd), (empty, b[4]), (b[4], empty)]:
        _pin(monkeypatch, ds, j, 0.0)
        del seen[:]
        random.seed(7 + i)
        k, flip, boxes, ud, coeffs, partner, pcoeffs, r = ds.draw_mix(i)
        assert len(seen) == 2 and np.array_equal(coeffs, seen[0][2]) and np.array_equal(pcoeffs, seen[1][2])
        parts = []
        for item, (M, gain, _) in zip((i, j), seen):
            lab = ds._labels(item)
            if len(lab):
                lab = ds._warp_labels(lab, M, gain)
                parts.append(np.concatenate([lab[:, 1:5], lab[:, 0:1], np.full((len(lab), 1), 255.0)], 1))
        want = np.concatenate(parts) if parts else np.zeros((0, 6))
        n = len(want)
        assert np.array_equal(boxes[:n], want) and not boxes[n:].any()
        if i == j:                                                                 # the same rows under two different warps
            assert len(parts) == 2 and not np.array_equal(parts[0], parts[1])


# ---- 5. the batch makes the items' draws in order ----
@pytest.mark.parametrize("p", [1.0, 0.5])
def test_getitems_makes_the_items_draws_in_order(trees, monkeypatch, p):
    ds = _ds(trees, mixup=p, **ACTIVE)
    got = {}

    def fake(indices, params, out_u8=False):
        got["indices"], got["params"] = list(indices), list(params)
        return torch.zeros((len(indices), 1, 256, 320))
    monkeypatch.setattr(ds, "_need_gpu", lambda: None)
    monkeypatch.setattr(ds, "augment_images", fake)
    idx = [5, 0, 22, 5, 17, 9, 21]
    random.seed(3)
    batch = ds.__getitems__(idx)
    end = random.getstate()
    random.seed(3)
    recs = [ds.draw_mix(i) for i in idx]
    assert random.getstate() == end and got["indices"] == idx
    assert torch.equal(batch.targets, torch.from_numpy(np.stack([r[2] for r in recs])))
    hits = 0
    for rec, prm in zip(recs, got["params"]):
        k, flip, _, ud, coeffs, partner, pcoeffs, r = rec
        assert len(prm) == 7 and prm[:3] == (k, flip, ud) and np.array_equal(prm[3], coeffs)
        assert prm[4] == partner and prm[6] == r and ((pcoeffs is None and prm[5] is None) or np.array_equal(prm[5], pcoeffs))
        hits += partner is not None
    assert hits == len(idx) if p == 1.0 else 0 < hits < len(idx)
    # one item through __getitem__: the same record reaches augment_images
    monkeypatch.setattr(ds, "augment_images", lambda indices, params, out_u8=False: got.update(one=params[0]) or torch.zeros((1, 256, 320, 1), dtype=torch.uint8))
    random.seed(3)
    _, boxes = ds[idx[0]]
    assert np.array_equal(boxes, recs[0][2]) and got["one"][4] == recs[0][5] and got["one"][6] == recs[0][7]


# ---- 6. the constructor ----
@pytest.mark.parametrize("p", [-0.1, 1.5])
def test_constructor_refuses_a_probability_outside_0_1_only_with_the_flag(trees, p):
    with pytest.raises(ValueError, match="mixup"):
        _ds(trees, mixup=p)
    assert _ds(trees, flag=False, mixup=p).mixup == 0.0
    assert _ds(trees, mixup=0.0).mixup == 0.0 and _ds(trees, mixup=1.0).mixup == 1.0
    assert _ds(trees, mixup=1.0, augment=False).draw_mix(0)[5:] == (None, None, None)      # no augmentation: no draw at all


# ---- 7. the C entry refuses bad arguments before the GPU is touched ----
def test_mix_entry_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)                      # never read: every call below is refused before a launch
    good = dict(d_frames=ptr, n_frames=4, N=2, h=16, w=20, c=1, d_first=ptr, d_second=ptr, d_params=ptr, d_warp=ptr, d_ratio=ptr, d_u8=ptr,
                d_x=ptr)

    def call(**change):
        a = dict(good, **change)
        return lib.yf_augment_mix_u8(0, a["d_frames"], a["n_frames"], a["N"], a["h"], a["w"], a["c"], a["d_first"], a["d_second"], a["d_params"],
                                     a["d_warp"], a["d_ratio"], a["d_u8"], a["d_x"], None)
    bad = [dict(d_frames=None), dict(d_first=None), dict(d_second=None), dict(d_params=None), dict(d_warp=None), dict(d_ratio=None),
           dict(d_u8=None, d_x=None), dict(N=0), dict(N=-1), dict(n_frames=0), dict(n_frames=-3), dict(c=2), dict(c=0), dict(c=4),
           dict(h=0), dict(h=-1), dict(h=16385), dict(w=0), dict(w=-1), dict(w=16385)]
    for change in bad:
        assert call(**change) == _lib.YF_E_INVALID, change
        assert b"yf_augment_mix_u8" in lib.yf_last_error_string()
    with pytest.raises(_lib.YFError, match="yf_augment_mix_u8"):
        _lib.check(call(c=2))
