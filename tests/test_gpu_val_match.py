"""`Validation(..., match="device")`: val_match_kernel behind yf_val_match against the host matching it restates
(`Validation._match_image`, itself pinned to the reference's goldens by tests/test_cpu_host.py), and `get_mAP` in both modes.

  * kernel: records (confidence bits, class, hit) and their order equal, bit for bit, what `_match_image` appends image by image -- on
    detections from the GPU NMS of tests/val_cases.py inputs and on hand-written `det` arrays where the geometry has to be exact.  No
    tolerance: the IoU is fp32 add / mul / div / compare in the same order.
  * get_mAP on the VOC fixture tree: match lists (keys and flags), target_num, log lines and mAP equal in both modes, also with a record
    buffer that has to grow in the middle of the run."""
import ctypes
import logging
import os
import sys

import numpy as np
import pytest
import torch

from tests import val_cases as vc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import voc_tree  # noqa: E402

WEIGHTS = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_256x320_epoch28.pth")
SENTINEL = 0x5A5A5A5A
NAMES = ["carrier", "defender", "destroyer"]


@pytest.fixture(scope="module")
def yf():
    import yolo_fastest_amd
    return yolo_fastest_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(yf, dev):
    io = yf.io_params_for(256)
    m = yf.YoloFastest(io).to(dev).eval()
    m.load_state_dict(torch.load(WEIGHTS, map_location=dev))
    return m, io


def _host_validation(thres=0.5):
    from yolo_fastest_amd import validation as V
    params = {"train_params": {"batch_size": 4, "IOU_val_thre": thres},
              "io_params": {"input_shape": (256, 320, 1), "num_cls": 3, "class_names": NAMES, "conf_thre": 0.5, "nms_thre": 0.2}}
    frames = [(np.zeros((2, 2, 1), np.float32), np.zeros((64, 6), np.float32))] * 4   # the loader is not used
    return V.Validation(params, logging.getLogger("t"), frames, "cpu", None)


def _expected(det, counts, targets, thres=0.5):
    """`_match_image` image by image -> (int32 [total, 3] records in image, slot order, the keys it stored).  `det` is class-ascending,
    so an image's records are its classes' lists one after the other."""
    val = _host_validation(thres)
    kmax = det.shape[1]
    rows, keys = [], []
    for i, count in enumerate(counts):
        n = min(max(int(count), 0), kmax)
        val.clear()
        val._match_image(det[i, :n] if n else None, targets[i])
        hits = [m for c in range(3) for m in val.match_list[c]]
        assert len(hits) == n
        for k in range(n):
            rows.append((int(det[i, k, 4:5].view(torch.int32)), int(det[i, k, 6]), int(hits[k][1])))
            keys.append(hits[k][0])
    return np.array(rows, np.int32).reshape(-1, 3), keys


def _match(dev, det, counts, targets, thres=0.5, cap=None, rec=None, cursor=None, turn=0):
    """yf_val_match through the C ABI -> (records int32 [rows, 3] on the host, the whole buffer; the cursor it wrote)."""
    from yolo_fastest_amd import _lib
    N, kmax = det.shape[0], det.shape[1]
    T = targets.shape[1]
    d_det = det.to(dev).contiguous()
    d_cnt = torch.as_tensor(counts, dtype=torch.int32).to(dev)
    d_tg = targets.to(dev).contiguous() if T else torch.zeros(6, dtype=torch.float32, device=dev)
    if rec is None:
        rec = torch.full((max(N * kmax, 1) + 4, 3), SENTINEL, dtype=torch.int32, device=dev)
    if cursor is None:
        cursor = torch.zeros(2, dtype=torch.int64, device=dev)
    cap = rec.shape[0] if cap is None else cap
    assert 0 <= cap <= rec.shape[0]
    rc = _lib.lib().yf_val_match(dev.index, d_det.data_ptr(), d_cnt.data_ptr(), N, kmax, d_tg.data_ptr(), T, float(thres),
                                 cursor[turn:].data_ptr(), cursor[1 - turn:].data_ptr(), rec.data_ptr(), cap,
                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, _lib.lib().yf_last_error_string()
    torch.cuda.synchronize(dev)
    return rec.cpu().numpy(), int(cursor[1 - turn])


def _check(dev, det, counts, targets, thres=0.5):
    """one call into a sentinel-filled buffer: the records, the cursor, and nothing written behind them.  -> the expected records"""
    from yolo_fastest_amd import validation as V
    want, keys = _expected(det, counts, targets, thres)
    got, nxt = _match(dev, det, counts, targets, thres)
    assert nxt == len(want)
    assert np.array_equal(got[:nxt], want), np.nonzero((got[:nxt] != want).any(1))[0][:8]
    assert (got[nxt:] == SENTINEL).all()
    assert V._conf_keys(torch.from_numpy(got[:nxt, 0].copy()).view(torch.float32)) == keys
    return want


def _targets_from(det, counts, T, seed, drop_class=None):
    """targets [N, T, 6] of seeded subsets of each image's detections, jittered by up to 4 px, some of them twice (several targets of one
    class over one detection), a few boxes no detection is near, shuffled; rows that do not exist (marker 1 or 0) in between."""
    rng = np.random.default_rng(seed)
    N = det.shape[0]
    out = np.zeros((N, T, 6), np.float32)
    for i in range(N):
        rows = []
        n = min(int(counts[i]), det.shape[1])
        if n:
            pick = rng.choice(n, min(n, max(1, T // 3)), replace=False)
            for k in pick:
                for rep in range(1 + int(rng.integers(0, 3) == 0)):
                    rows.append(np.concatenate([det[i, k, :4].numpy() + rng.uniform(-4, 4, 4), [float(det[i, k, 6]), 255.0]]))
        for _ in range(3):
            x, y = rng.uniform(0, 500), rng.uniform(0, 400)
            rows.append(np.array([x, y, x + rng.uniform(20, 200), y + rng.uniform(20, 200), float(rng.integers(0, 3)), 255.0]))
        rows = [r for r in rows if drop_class is None or r[4] != drop_class]
        rng.shuffle(rows)
        rows = rows[:T]
        slots = np.sort(rng.choice(T, len(rows), replace=False))
        out[i, slots] = np.array(rows, np.float32).reshape(-1, 6)
        free = np.setdiff1d(np.arange(T), slots)
        out[i, free[::2], 5] = 1.0                     # marker 1 does not exist either (validate.py:47: > 1)
        out[i, free[::2], :4] = (0, 0, 640, 512)
    return torch.from_numpy(out)


def _nms(model, dev, case, frames):
    from yolo_fastest_amd import validation as V
    det, cnt, _ = V._nms_device(case.pred[frames].to(dev), case.C, case.conf_thres, case.nms_thres, None, model[0])
    return det.cpu(), cnt.cpu().tolist()


def test_nms_survivors_against_jittered_targets(model, dev):
    """N = 4 (both `ties` cases) and N = 5 (the scattered pass ladder: 0, 1, 64, 65 and 256 passing rows) through the GPU NMS, T = 64 and
    130; class 1 has detections and no targets in the second batch; the frame without detections has targets."""
    ties = vc.cases("ties")
    runs = [_nms(model, dev, c, [0, 1]) for c in ties]
    det, cnt = torch.cat([d for d, _ in runs]), [n for _, c in runs for n in c]
    assert det.shape[0] == 4 and min(cnt) > 8
    want = _check(dev, det, cnt, _targets_from(det, cnt, 64, 1))
    assert 0 < want[:, 2].sum() < len(want)
    want = _check(dev, det, cnt, _targets_from(det, cnt, 130, 2, drop_class=1.0))
    assert (want[:, 1] == 1).any() and not want[want[:, 1] == 1, 2].any() and want[:, 2].any()
    ladder = next(c for c in vc.cases("pass_1200") if c.name.endswith("scattered"))
    det, cnt = _nms(model, dev, ladder, [0, 1, 2, 3, 4])
    assert cnt[0] == 0 and cnt[1] == 1 and max(cnt) > 8
    for T, seed in ((64, 3), (130, 4), (65, 5)):
        tg = _targets_from(det, cnt, T, seed)
        assert int((tg[0, :, 5] > 1).sum()) == 3
        want = _check(dev, det, cnt, tg)
        assert 0 < want[:, 2].sum() < len(want)


def _det(rows, kmax=None):
    """hand-written detections: rows[i] = [(x1, y1, x2, y2, conf, cls), ...] per image, class-ascending -> float32 [N, kmax, 7], counts"""
    kmax = kmax or max(1, max(len(r) for r in rows))
    det = torch.full((len(rows), kmax, 7), -7.0)
    for i, r in enumerate(rows):
        for k, (x1, y1, x2, y2, conf, cls) in enumerate(r[:kmax]):
            det[i, k] = torch.tensor([x1, y1, x2, y2, conf, 0.9, cls])
    return det, [len(r) for r in rows]


BOX = (10.0, 10.0, 50.0, 50.0)


@pytest.mark.parametrize("T", [0, 1, 64, 65, 130])
def test_target_chunks_and_the_place_of_the_only_match(dev, T):
    """lanes are targets, 64 at a time: the only target a detection can take at index 0, 63, 64 and T - 1; every other slot holds a
    target of the wrong class over the same box or of the right class far away.  Image 1: the same targets with marker 1 (none exists);
    image 2: no detections."""
    det, cnt = _det([[BOX + (0.9, 0.0), BOX + (0.8, 1.0)], [BOX + (0.9, 0.0), BOX + (0.8, 1.0)], []])
    places = sorted({p for p in (0, 63, 64, T - 1) if 0 <= p < T}) or [None]
    for place in places:
        tg = torch.zeros((3, T, 6))
        for t in range(T):
            tg[:, t] = torch.tensor(BOX + (2.0, 255.0)) if t % 2 else torch.tensor((300.0, 300.0, 340.0, 340.0, 0.0, 255.0))
        if place is not None:
            tg[:, place] = torch.tensor((12.0, 9.0, 51.0, 50.0, 0.0, 255.0))
        tg[1, :, 5] = 1.0
        want = _check(dev, det, cnt, tg)
        assert want[:, 2].tolist() == [int(place is not None), 0, 0, 0], (T, place)


def test_lowest_index_wins_and_a_taken_target_is_gone(dev):
    """detection A is over targets 2, 5 and 70 (one class): it takes 2.  B is over 2 alone: false positive.  C is exactly 5: true positive.
    D, of another class, is exactly A's box: no target of its class."""
    det, cnt = _det([[(0, 0, 99, 105, 0.9, 1.0), (0, 0, 99, 55, 0.8, 1.0), (0, 0, 99, 119, 0.7, 1.0), (0, 0, 99, 105, 0.95, 2.0)]] * 3)
    tg = torch.zeros((3, 130, 6))
    tg[:, 2] = torch.tensor((0.0, 0.0, 99.0, 99.0, 1.0, 255.0))
    tg[:, 5] = torch.tensor((0.0, 0.0, 99.0, 119.0, 1.0, 255.0))
    tg[:, 70] = torch.tensor((0.0, 0.0, 119.0, 99.0, 1.0, 255.0))
    tg[1, 2, 5] = 0.0                                  # image 1 without target 2: A takes 5, B still has nothing, C is left with 70
    tg[2, :, 4] = 0.0                                  # image 2: every target of class 0
    want = _check(dev, det, cnt, tg)
    assert want[:, 2].tolist() == [1, 0, 1, 0] + [1, 0, 1, 0] + [0, 0, 0, 0]


def test_iou_at_the_threshold(dev):
    """pairs whose fp32 IoU is exactly 0.5, the value below and the value above (val_cases.IOU_PAIRS): only `above` is a match"""
    rows, tg = [], torch.zeros((3, 64, 6))
    for i, kind in enumerate(vc.IOU_PAIR_ORDER):
        W1, H1, W2, H2 = vc.IOU_PAIRS[0.5][kind]
        rows.append([(0.0, 0.0, W1 - 1.0, H1 - 1.0, 0.9, 0.0)])
        tg[i, 7] = torch.tensor((0.0, 0.0, W2 - 1.0, H2 - 1.0, 0.0, 255.0))
    det, cnt = _det(rows)
    want = _check(dev, det, cnt, tg)
    assert want[:, 2].tolist() == [0, 0, 1]
    want = _check(dev, det, cnt, tg, thres=float(np.nextafter(np.float32(0.5), np.float32(0))))   # one fp32 step lower: `equal` matches too
    assert want[:, 2].tolist() == [1, 0, 1]


def test_nan_and_infinite_corners(dev):
    """torch.max / min / clamp hand NaN on: a NaN corner gives a NaN IoU, which is above nothing; infinite corners as the arithmetic has it"""
    nan, inf = float("nan"), float("inf")
    one = [(nan, 10, 50, 50, 0.9, 0.0), (10, 10, 50, nan, 0.85, 0.0), (10, 10, inf, 50, 0.8, 0.0), (-inf, 10, inf, 50, 0.7, 0.0),
           (-inf, -inf, inf, inf, 0.65, 0.0), (10, 10, 50, 50, 0.6, 0.0), (inf, 10, inf, 50, 0.55, 1.0), (10, 10, 50, 50, 0.5, 1.0)]
    det, cnt = _det([one, one, one])
    tg = torch.zeros((3, 65, 6))
    tg[:, 0] = torch.tensor(BOX + (0.0, 255.0))
    tg[:, 64] = torch.tensor(BOX + (1.0, 255.0))
    tg[1, 0, 2] = inf                                   # an infinite target: inf / (inf + inf - inf) where a box reaches it, else area / inf = 0
    tg[2, 0, 0] = nan                                   # a NaN target: nothing can take it
    want = _check(dev, det, cnt, tg)
    assert want[:, 2].tolist() == [0, 0, 0, 0, 0, 1, 0, 1] + [0, 0, 0, 0, 0, 0, 0, 1] + [0, 0, 0, 0, 0, 0, 0, 1]


def test_kmax_below_the_count_and_garbage_counts(dev):
    """counts as yf_val_nms_ex leaves them when an image has more survivors than K_max (the true number), and garbage: an image
    contributes min(max(count, 0), K_max) records and the next image starts right behind them"""
    rows = [[(10.0 * k, 0.0, 10.0 * k + 30, 30.0, 0.9 - 0.01 * k, 0.0) for k in range(4)] for _ in range(5)]
    det, _ = _det(rows)
    cnt = [9, 2, -3, 2 ** 31 - 1, 4]
    tg = torch.zeros((5, 64, 6))
    for k in range(4):
        tg[:, 3 * k] = torch.tensor((10.0 * k + 1, 0.0, 10.0 * k + 30, 31.0, 0.0, 255.0))
    want = _check(dev, det, cnt, tg)
    assert len(want) == 4 + 2 + 0 + 4 + 4 and want[:, 2].all()


def test_capacity_and_a_shared_cursor(dev):
    """cap below the total: nothing at or behind record `cap` is written and the cursor still counts every detection.  Two calls in a row,
    the second reading the cursor the first wrote: one list, in call order."""
    rng = np.random.default_rng(11)
    boxes = torch.from_numpy(vc._boxes(rng, (3, 40), 3))
    det = torch.zeros((3, 40, 7))
    det[..., :2], det[..., 2:4] = boxes[..., :2], boxes[..., :2] + boxes[..., 2:4]
    det[..., 4] = torch.sort(boxes[..., 4], descending=True)[0]
    det[..., 6] = torch.sort(torch.from_numpy(rng.integers(0, 3, (3, 40))).float())[0]
    cnt = [40, 17, 33]
    tg = _targets_from(det, cnt, 64, 12)
    want, _ = _expected(det, cnt, tg)
    total = len(want)
    assert total == 90 and 0 < want[:, 2].sum() < total
    for cap in (total - 3, 41, 0):
        got, nxt = _match(dev, det, cnt, tg, cap=cap)
        assert nxt == total
        assert np.array_equal(got[:cap], want[:cap]) and (got[cap:] == SENTINEL).all(), cap
    rec = torch.full((2 * total + 5, 3), SENTINEL, dtype=torch.int32, device=dev)
    cursor = torch.zeros(2, dtype=torch.int64, device=dev)
    _, first = _match(dev, det, cnt, tg, rec=rec, cursor=cursor, turn=0)
    tg2 = _targets_from(det, cnt, 64, 13)
    got, second = _match(dev, det[[2, 0]], [cnt[2], cnt[0]], tg2[[2, 0]], rec=rec, cursor=cursor, turn=1)
    want2, _ = _expected(det[[2, 0]], [cnt[2], cnt[0]], tg2[[2, 0]])
    assert (first, second) == (total, total + len(want2)) and cursor.tolist() == [second, first]
    assert np.array_equal(got[:second], np.concatenate([want, want2])) and (got[second:] == SENTINEL).all()


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.fixture(scope="module")
def map_runs(yf, model, dev, golden, tmp_path_factory):
    """get_mAP over the VOC fixture tree (20 frames, batch 4, shuffled under one seed): host mode once, shared"""
    from yolo_fastest_amd import validation as V
    from yolo_fastest_amd.dataset import DetectDataset
    m, io = model
    trees = voc_tree.make_trees(tmp_path_factory.mktemp("voc"))
    params = {"train_params": {"batch_size": 4, "IOU_val_thre": 0.5}, "io_params": dict(io, class_names=NAMES)}

    def run(match, capacity=None):
        log = logging.getLogger("test-gpu-val-match-%s-%s" % (match, capacity))
        log.setLevel(logging.INFO)
        log.propagate = False
        lines = _Lines()
        log.addHandler(lines)
        losses = [V.YOLOLossV3(io["anchors"][i], io["num_cls"], io["input_shape"], dev) for i in range(2)]
        ds = DetectDataset([256, 320, 1], [512, 640, 3], log, aug_params=voc_tree.aug_params(trees), max_boxes=64, device=dev, val=True,
                           augment=False)
        torch.manual_seed(0)
        val = V.Validation(params, log, ds, dev, losses, match=match)
        if capacity is not None:
            val._record_capacity = capacity
        del lines.lines[:]
        mAP = float(val.get_mAP(m, 3))
        return {"mAP": mAP, "match_list": val.match_list, "target_num": val.target_num.tolist(), "lines": lines.lines}
    return run, run("host")


@pytest.mark.parametrize("capacity", [None, 8])
def test_get_map_is_the_same_in_both_modes(map_runs, golden, capacity):
    """capacity 8: the record buffer is smaller than the first batch's bound, so it grows while the run goes on"""
    run, host = map_runs
    gd = golden("golden_dataset")
    got = run("device", capacity)
    assert got["target_num"] == host["target_num"] == gd["target_num"].tolist()
    for c in range(3):
        assert got["match_list"][c] == host["match_list"][c], c
        assert all(type(k) is str and type(h) is bool for k, h in got["match_list"][c])
    assert [len(got["match_list"][c]) for c in range(3)] == gd["match_n"].tolist()
    assert [sum(t for _, t in got["match_list"][c]) for c in range(3)] == gd["match_tp"].tolist()
    assert got["lines"] == host["lines"] and len(got["lines"]) == 6 and got["lines"][4].startswith("mean AP")
    assert got["mAP"] == host["mAP"]
    assert abs(got["mAP"] - float(gd["mAP"])) < 2e-3, (got["mAP"], float(gd["mAP"]))   # tests/test_gpu_dataset.py's bound for this value
