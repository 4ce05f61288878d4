"""DetectDataset's geometric augment_params on the host (dataset.py: draw_ex, _draw_warp, _warp_labels): labels and random draws only, no
GPU.  Neutral or absent keys leave the `random` stream and the boxes the reference's (golden_dataset.npz); active keys add eight
random.uniform draws per item (+ one random.random for flipud); warped labels against a separate restatement of yolov5's arithmetic."""
import logging
import math
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voc_tree  # noqa: E402

LOG = logging.getLogger("test-dataset-geometric")
GEOMETRIC = ("degrees", "translate", "scale", "shear", "perspective", "flipud")
ACTIVE = dict(degrees=10.0, translate=0.1, scale=1.3, shear=2.0, perspective=0.0005)


def _ds(trees, channels=1, max_boxes=64, **keys):
    from yolo_fastest_amd.dataset import DetectDataset
    ap = voc_tree.aug_params(trees)
    for k in keys.pop("absent", ()):
        del ap[k]
    ap.update(keys)
    return DetectDataset([256, 320, channels], [512, 640, 3], LOG, aug_params=ap, max_boxes=max_boxes, device="cpu")


@pytest.fixture()
def trees(tmp_path):
    return voc_tree.make_trees(tmp_path)


class Counting:
    """Counts the calls of random.random and random.uniform (uniform calls random.random itself: those are not counted twice)."""
    def __init__(self, monkeypatch):
        self.random = self.uniform = 0
        real_random, real_uniform = random.random, random.uniform

        def rnd():
            self.random += 1
            return real_random()

        def uni(a, b):
            self.uniform += 1
            return a + (b - a) * real_random()
        monkeypatch.setattr(random, "random", rnd)
        monkeypatch.setattr(random, "uniform", uni)


@pytest.mark.parametrize("absent", [(), GEOMETRIC, ("degrees", "flipud")])
@pytest.mark.parametrize("key", ["c1_s0", "c1_s1", "c1_s2", "c3_s0"])
def test_neutral_or_absent_keys_are_the_reference(golden, trees, key, absent):
    """The reference's own items (recorded from its DetectDataset): k, flip and boxes, item after item from one seed -- so the draws
    are its draws -- and the stream ends where a run of the plain (blur?, which blur, flip?) draws ends."""
    g = golden("golden_dataset")
    ds = _ds(trees, 1 if key.startswith("c1") else 3, absent=absent)
    assert not ds.geometric
    names = [os.path.splitext(os.path.basename(p))[0] for p in ds.img_list]
    random.seed(int(key[-1]))
    for j, stem in enumerate(g[key + "_names"]):
        k, flip, boxes, flipud, coeffs = ds.draw_ex(names.index(str(stem)))
        assert (k, flip, flipud, coeffs) == (int(g[key + "_k"][j]), bool(g[key + "_flip"][j]), False, None)
        if not g[key + "_raised"][j]:
            assert np.array_equal(boxes, g[key + "_boxes"][j])
    end = random.getstate()
    random.seed(int(key[-1]))
    for _ in g[key + "_names"]:
        if random.random() < ds.gussian_filter:
            random.random()
        random.random()
    assert random.getstate() == end


def test_draw_is_draw_ex_without_the_geometric_part(trees):
    ds = _ds(trees, flipud=0.5, **ACTIVE)
    for i in range(len(ds)):
        random.seed(i)
        k, flip, boxes = ds.draw(i)
        random.seed(i)
        ex = ds.draw_ex(i)
        assert (k, flip) == ex[:2] and np.array_equal(boxes, ex[2]) and len(ex) == 5 and ex[4].shape == (8,) and ex[4].dtype == np.float64


@pytest.mark.parametrize("keys,uniforms,randoms", [
    (dict(), 0, 0), (dict(flipud=0.5), 0, 1), (dict(degrees=5.0), 8, 0), (dict(scale=0.7), 8, 0), (dict(translate=0.1, flipud=1.0), 8, 1),
    (dict(shear=1.0), 8, 0), (dict(perspective=0.0003, flipud=0.2), 8, 1), (dict(flipud=0.5, **ACTIVE), 8, 1)])
def test_active_keys_consume_eight_draws_and_one_for_flipud(trees, monkeypatch, keys, uniforms, randoms):
    base, ds = _ds(trees), _ds(trees, **keys)
    c = Counting(monkeypatch)
    for i in range(len(ds)):
        random.seed(100 + i)
        c.random = c.uniform = 0
        base.draw(i)
        plain = c.random
        assert c.uniform == 0
        random.seed(100 + i)
        c.random = c.uniform = 0
        k, flip, _, flipud, coeffs = ds.draw_ex(i)
        assert c.uniform == uniforms and (coeffs is None) == (uniforms == 0)
        # the blur and fliplr draws come after the eight, so they see other values: count them by what they decided
        assert c.random == (2 if k else 1) + 1 + randoms
        if not uniforms:
            assert c.random == plain + randoms
    # a dataset that does not augment draws nothing at all
    from yolo_fastest_amd.dataset import DetectDataset
    off = DetectDataset([256, 320, 1], [512, 640, 3], LOG, aug_params=dict(voc_tree.aug_params(trees), flipud=0.5, **ACTIVE), augment=False,
                        device="cpu")
    c.random = c.uniform = 0
    assert off.draw_ex(0)[3:] == (False, None) and c.random == 0 and c.uniform == 0


def test_draw_order_and_matrix(trees, monkeypatch):
    """The eight draws in order -- perspective x, y, angle, gain, shear x, y, translate x, y -- before the blur draw; flipud after fliplr;
    M = T S R P C rebuilt from the recorded values; the coefficients are inv(M) / inv(M)[2, 2]; an affine frame ends in exact zeros."""
    seen = []
    real_random = random.random

    def uni(a, b):
        v = a + (b - a) * real_random()
        seen.append(("u", a, b, v))
        return v

    def rnd():
        v = real_random()
        seen.append(("r", v))
        return v
    monkeypatch.setattr(random, "uniform", uni)
    monkeypatch.setattr(random, "random", rnd)
    for persp in (0.0005, 0.0):
        ds = _ds(trees, flipud=0.5, **dict(ACTIVE, perspective=persp))
        del seen[:]
        random.seed(3)
        k, flip, _, flipud, coeffs = ds.draw_ex(0)
        assert [s[0] for s in seen[:8]] == ["u"] * 8 and all(s[0] == "r" for s in seen[8:])
        g = abs(1.3 - 1)
        assert [(s[1], s[2]) for s in seen[:8]] == [(-persp, persp)] * 2 + [(-10.0, 10.0), (1 - g, 1 + g)] + [(-2.0, 2.0)] * 2 + [(0.4, 0.6)] * 2
        assert flip == (seen[-2][1] < 0.5) and flipud == (seen[-1][1] < 0.5) and len(seen) == 8 + (2 if k else 1) + 2
        px, py, ang, s, shx, shy, tx, ty = [v[3] for v in seen[:8]]
        W, H = 320, 256
        C = np.array([[1, 0, -W / 2], [0, 1, -H / 2], [0, 0, 1.0]])
        P = np.array([[1, 0, 0], [0, 1, 0], [px, py, 1.0]])
        a = math.radians(ang)
        R = np.array([[s * math.cos(a), s * math.sin(a), 0], [-s * math.sin(a), s * math.cos(a), 0], [0, 0, 1.0]])
        S = np.array([[1, math.tan(math.radians(shx)), 0], [math.tan(math.radians(shy)), 1, 0], [0, 0, 1.0]])
        T = np.array([[1, 0, tx * W], [0, 1, ty * H], [0, 0, 1.0]])
        inv = np.linalg.inv(T @ S @ R @ P @ C)
        want = (inv / inv[2, 2]).reshape(9)[:8]
        if persp == 0:
            assert coeffs[6] == 0.0 and coeffs[7] == 0.0
            assert np.allclose(coeffs[:6], want[:6], rtol=1e-12, atol=1e-12)
        else:
            assert np.allclose(coeffs, want, rtol=1e-12, atol=1e-15) and coeffs[6] != 0.0
        assert all(coeffs[6] * x + coeffs[7] * y + 1 > 0 for x in (0, W) for y in (0, H))


def _warp_boxes(xywh, M, s, W, H):
    """yolov5's random_perspective + box_candidates for normalised (xc, yc, w, h) rows, box by box in plain Python floats."""
    out = []
    for xc, yc, w, h in xywh:
        x1, y1, x2, y2 = (xc - w / 2) * W, (yc - h / 2) * H, (xc + w / 2) * W, (yc + h / 2) * H
        pts = []
        for x, y in ((x1, y1), (x2, y2), (x1, y2), (x2, y1)):
            u, v, d = (M[r][0] * x + M[r][1] * y + M[r][2] for r in range(3))
            pts.append((u / d, v / d))
        nx1, nx2 = min(max(min(p[0] for p in pts), 0), W), min(max(max(p[0] for p in pts), 0), W)
        ny1, ny2 = min(max(min(p[1] for p in pts), 0), H), min(max(max(p[1] for p in pts), 0), H)
        w2, h2 = nx2 - nx1, ny2 - ny1
        ok = w2 > 2 and h2 > 2 and w2 * h2 / ((x2 - x1) * s * (y2 - y1) * s + 1e-16) > 0.1 and max(w2 / (h2 + 1e-16), h2 / (w2 + 1e-16)) < 20
        out.append(((nx1 + nx2) / 2 / W, (ny1 + ny2) / 2 / H, w2 / W, h2 / H) if ok else None)
    return out


def test_warped_labels_equal_the_restatement(trees, monkeypatch):
    plain = _ds(trees, max_boxes=128)
    ds = _ds(trees, max_boxes=128, flipud=0.5, **ACTIVE)
    kept = dropped = 0
    rec = {}
    real = ds._draw_warp

    def spy():
        rec["M"], rec["s"], rec["c"] = real()
        return rec["M"], rec["s"], rec["c"]
    monkeypatch.setattr(ds, "_draw_warp", spy)
    monkeypatch.setattr(plain, "augment", False)
    for i in range(len(ds)):
        for seed in range(4):
            random.seed(seed)
            k, flip, boxes, flipud, coeffs = ds.draw_ex(i)
            before = plain.draw(i)[2]
            nb = int((before[:, 5] == 255.0).sum())
            want = []
            for row, w in zip(before[:nb], _warp_boxes(before[:nb, :4], rec["M"].tolist(), rec["s"], 320, 256)):
                if w is None:
                    dropped += 1
                    continue
                kept += 1
                x, y = (1 - w[0] if flip else w[0]), (1 - w[1] if flipud else w[1])
                want.append([x, y, w[2], w[3], row[4], 255.0])
            n = len(want)
            assert np.allclose(boxes[:n], np.array(want).reshape(n, 6), rtol=1e-12, atol=1e-12)
            assert not boxes[n:].any()
            assert np.array_equal(coeffs, rec["c"])
    assert kept > 100


def test_a_box_pushed_out_of_the_frame_is_dropped_and_the_rest_compacted(trees, monkeypatch):
    """A pure shift of 0.3 W to the right (a hand-made matrix in place of the draw): boxes right of 0.7 leave the frame and the boxes
    after them in file order move up; a box cut by the border is clipped."""
    ds = _ds(trees, max_boxes=128, translate=0.3)
    M = np.array([[1, 0, 0.3 * 320], [0, 1, 0], [0, 0, 1.0]])
    monkeypatch.setattr(ds, "_draw_warp", lambda: (M, 1.0, np.array([1, 0, -0.3 * 320, 0, 1, 0, 0, 0.0])))
    monkeypatch.setattr(ds, "fliplr", 0.0)
    monkeypatch.setattr(ds, "gussian_filter", 0.0)
    plain = _ds(trees, max_boxes=128, fliplr=0.0, gussian_filter=0.0)
    gone = holes = clipped = 0
    for i in range(len(ds)):
        before = plain.draw(i)[2]
        nb = int((before[:, 5] == 255.0).sum())
        boxes = ds.draw_ex(i)[2]
        out_of_frame = before[:nb, 0] - before[:nb, 2] / 2 + 0.3 >= 1 - 2 / 320          # what is left of it is at most 2 pixels wide
        want = [w for w in _warp_boxes(before[:nb, :4], M.tolist(), 1.0, 320, 256)]
        assert all((w is None) or not o for w, o in zip(want, out_of_frame))
        keep = [j for j, w in enumerate(want) if w is not None]
        gone += nb - len(keep)
        holes += int(any(j > m for m, j in enumerate(keep)))                                  # a kept box that moved up
        n = len(keep)
        assert int((boxes[:, 5] == 255.0).sum()) == n and not boxes[n:].any()
        assert np.array_equal(boxes[:n, 4], before[keep, 4])
        assert np.allclose(boxes[:n, :4], np.array([want[j] for j in keep]).reshape(n, 4), rtol=1e-12, atol=1e-12)
        assert (boxes[:n, 0] + boxes[:n, 2] / 2 <= 1 + 1e-12).all()
        clipped += int((np.abs(boxes[:n, 2] - before[keep, 2]) > 1e-9).sum())
    assert gone > 0 and holes > 0 and clipped > 0


@pytest.mark.parametrize("keys", [dict(scale=0.0), dict(scale=2.0), dict(scale=-0.5), dict(scale=2.5), dict(degrees=-1.0), dict(shear=-0.1),
                                  dict(perspective=-0.001), dict(translate=-0.1), dict(translate=1.0), dict(translate=1.5),
                                  dict(degrees=float("nan"))])
def test_constructor_refuses_out_of_range_values(trees, keys):
    with pytest.raises(ValueError, match=next(iter(keys))):
        _ds(trees, **keys)


def test_constructor_accepts_the_ends_of_the_ranges(trees):
    assert not _ds(trees, scale=1.0, degrees=0.0, shear=0.0, perspective=0.0, translate=0.0).geometric
    assert _ds(trees, scale=0.001, translate=0.999).geometric and _ds(trees, scale=1.999).geometric


def test_a_perspective_that_always_folds_is_refused_at_the_draw(trees, monkeypatch):
    """Documented choice: a folding draw is redrawn (all eight values); 100 in a row raise."""
    ds = _ds(trees, perspective=0.0005)
    monkeypatch.setattr(ds, "perspective", 1.0)
    monkeypatch.setattr(random, "uniform", lambda a, b: b)
    with pytest.raises(ValueError, match="perspective"):
        ds.draw_ex(0)


def test_mixup_stays_ignored(trees):
    a, b = _ds(trees, mixup=0.0), _ds(trees, mixup=0.9)
    for i in range(len(a)):
        random.seed(i)
        x = a.draw_ex(i)
        s = random.getstate()
        random.seed(i)
        y = b.draw_ex(i)
        assert s == random.getstate() and x[:2] == y[:2] and np.array_equal(x[2], y[2])
