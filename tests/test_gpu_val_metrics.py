"""yolov5-style validation scoring on the device: val_match_iouv_kernel behind yf_val_match_iouv against the direct definition
(tests/val_metrics_ref.py, itself held to a literal process_batch by tests/test_cpu_val_metrics.py), `Validation.get_metrics` in both
matching modes, and `train(..., val_metrics=True)`.

  * kernel: records (obj_conf bits, class_conf bits, class, hit mask) and their order bit for bit.  No tolerance: the IoU is fp32
    sub / mul / add / div / compare in one stated order, and the winner of a target is a minimum, which no execution order can change.
  * get_metrics on the VOC fixture tree: the same dict (`ap` bitwise) and the same log lines with match="host" and match="device", also
    with a record buffer that has to grow in the middle of the run.
  * train: YOLO-Fastest_best.pth is the checkpoint of the epoch with the best logged fitness; without val_metrics nothing new appears."""
import copy
import ctypes
import logging
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

from tests import val_metrics_ref as ref

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


def _match(dev, det, counts, targets, thr, cap=None, rec=None, cursor=None, turn=0):
    """yf_val_match_iouv through the C ABI -> (the whole record buffer int32 [rows, 4] on the host, the cursor it wrote)"""
    from yolo_fastest_amd import _lib
    N, kmax, T = det.shape[0], det.shape[1], targets.shape[1]
    d_det = torch.from_numpy(np.ascontiguousarray(det, np.float32)).to(dev)
    d_cnt = torch.as_tensor(counts, dtype=torch.int32).to(dev)
    d_tg = torch.from_numpy(np.ascontiguousarray(targets, np.float32)).to(dev) if T else torch.zeros(6, dtype=torch.float32, device=dev)
    if rec is None:
        rec = torch.full((max(N * kmax, 1) + 4, 4), SENTINEL, dtype=torch.int32, device=dev)
    if cursor is None:
        cursor = torch.zeros(2, dtype=torch.int64, device=dev)
    cap = rec.shape[0] if cap is None else cap
    assert 0 <= cap <= rec.shape[0]
    c_thr = (ctypes.c_double * len(thr))(*[float(v) for v in thr])
    rc = _lib.lib().yf_val_match_iouv(dev.index, d_det.data_ptr(), d_cnt.data_ptr(), N, kmax, d_tg.data_ptr(), T, c_thr, len(thr),
                                      cursor[turn:].data_ptr(), cursor[1 - turn:].data_ptr(), rec.data_ptr(), cap,
                                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, _lib.lib().yf_last_error_string()
    torch.cuda.synchronize(dev)
    return rec.cpu().numpy(), int(cursor[1 - turn])


@pytest.mark.parametrize("name", [c[0] for c in ref.CASES])
def test_records_equal_the_direct_definition(dev, name):
    """one call into a sentinel-filled buffer: the records, the cursor, and nothing written behind them (val_metrics_ref.CASES: n around
    the workgroup width, T around a wave and at the cap, contested targets across waves, thresholds one fp32 step either side of an IoU,
    ties, class mismatch, markers, NaN and infinity, clamped counts, 1 and 16 thresholds)"""
    _, (det, counts, tg), thr = next(c for c in ref.CASES if c[0] == name)
    want = ref.direct_records(det, counts, tg, thr)
    got, nxt = _match(dev, det, counts, tg, thr)
    assert nxt == len(want)
    assert np.array_equal(got[:nxt], want), np.nonzero((got[:nxt] != want).any(1))[0][:8]
    assert (got[nxt:] == SENTINEL).all()


def test_capacity_and_a_shared_cursor(dev):
    """cap below the total: nothing at or behind record `cap` is written and the cursor still counts every detection.  Two calls in a row,
    the second reading the cursor the first wrote: one list, in call order."""
    det, cnt, tg = ref.random_batch(21, [300, 17, 33], 64)
    want = ref.direct_records(det, cnt, tg, ref.IOUV)
    total = len(want)
    assert total == 350 and 0 < (want[:, 3] != 0).sum() < total
    for cap in (total - 3, 257, 0):
        got, nxt = _match(dev, det, cnt, tg, ref.IOUV, cap=cap)
        assert nxt == total
        assert np.array_equal(got[:cap], want[:cap]) and (got[cap:] == SENTINEL).all(), cap
    rec = torch.full((2 * total + 5, 4), SENTINEL, dtype=torch.int32, device=dev)
    cursor = torch.zeros(2, dtype=torch.int64, device=dev)
    _, first = _match(dev, det, cnt, tg, ref.IOUV, rec=rec, cursor=cursor, turn=0)
    det2, cnt2, tg2 = ref.random_batch(22, [33, 300], 65, kmax=300)
    got, second = _match(dev, det2, cnt2, tg2, ref.IOUV[:3], rec=rec, cursor=cursor, turn=1)
    want2 = ref.direct_records(det2, cnt2, tg2, ref.IOUV[:3])
    assert (first, second) == (total, total + len(want2)) and cursor.tolist() == [second, first]
    assert np.array_equal(got[:second], np.concatenate([want, want2])) and (got[second:] == SENTINEL).all()


def test_refusals_leave_the_buffers_alone(dev):
    """every YF_E_INVALID of the header with real device buffers behind the pointers: records and cursor keep their sentinels"""
    from yolo_fastest_amd import _lib
    lib = _lib.lib()
    det, cnt, tg = ref.random_batch(23, [5, 3], 4)
    d_det, d_cnt, d_tg = torch.from_numpy(det).to(dev), torch.as_tensor(cnt, dtype=torch.int32).to(dev), torch.from_numpy(tg).to(dev)
    rec = torch.full((16, 4), SENTINEL, dtype=torch.int32, device=dev)
    cursor = torch.full((2,), SENTINEL, dtype=torch.int64, device=dev)
    good = dict(det=d_det.data_ptr(), counts=d_cnt.data_ptr(), N=2, K=5, targets=d_tg.data_ptr(), T=4, thr=[0.5, 0.75], nthr=None,
                base=cursor.data_ptr(), next=cursor[1:].data_ptr(), rec=rec.data_ptr(), cap=16)
    nan, inf = float("nan"), float("inf")
    bad = [{k: None} for k in ("det", "counts", "targets", "base", "next", "rec")] + [
        dict(thr=None, nthr=2), dict(N=0), dict(N=-1), dict(K=0), dict(K=-3), dict(T=-1), dict(cap=-1), dict(T=ref.MAX_T + 1),
        dict(next=cursor.data_ptr()), dict(thr=[], nthr=0), dict(nthr=-1), dict(thr=[0.5] * 17), dict(thr=[0.5, nan]), dict(thr=[inf]),
        dict(thr=[-inf]), dict(thr=[1e300])]
    for kw in bad:
        a = dict(good, **kw)
        thr = None if a["thr"] is None else (ctypes.c_double * max(len(a["thr"]), 1))(*a["thr"])
        nthr = len(a["thr"]) if a["nthr"] is None else a["nthr"]
        rc = lib.yf_val_match_iouv(dev.index, a["det"], a["counts"], a["N"], a["K"], a["targets"], a["T"], thr, nthr, a["base"], a["next"],
                                   a["rec"], a["cap"], ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == _lib.YF_E_INVALID and b"yf_val_match_iouv" in lib.yf_last_error_string(), kw
    torch.cuda.synchronize(dev)
    assert bool((rec == SENTINEL).all()) and bool((cursor == SENTINEL).all())


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _logger(name):
    log = logging.getLogger(name)
    log.setLevel(logging.INFO)
    log.propagate = False
    lines = _Lines()
    log.handlers[:] = [lines]
    return log, lines.lines


@pytest.fixture(scope="module")
def metric_runs(yf, dev, tmp_path_factory):
    """get_metrics over the VOC fixture tree (20 frames, batch 4, shuffled under one seed) with the shipped weights: host mode once, shared"""
    from yolo_fastest_amd import validation as V
    from yolo_fastest_amd.dataset import DetectDataset
    io = yf.io_params_for(256)
    m = yf.YoloFastest(io).to(dev).eval()
    m.load_state_dict(torch.load(WEIGHTS, map_location=dev))
    trees = voc_tree.make_trees(tmp_path_factory.mktemp("voc"))
    params = {"train_params": {"batch_size": 4, "IOU_val_thre": 0.5}, "io_params": dict(io, class_names=NAMES)}

    def run(match, capacity=None):
        log, lines = _logger("test-gpu-val-metrics-%s-%s" % (match, capacity))
        losses = [V.YOLOLossV3(io["anchors"][i], io["num_cls"], io["input_shape"], dev) for i in range(2)]
        ds = DetectDataset([256, 320, 1], [512, 640, 3], log, aug_params=voc_tree.aug_params(trees), max_boxes=64, device=dev, val=True,
                           augment=False)
        val = V.Validation(params, log, ds, dev, losses, match=match)
        if capacity is not None:
            val._record_capacity = capacity
        del lines[:]
        torch.manual_seed(0)
        out = val.get_metrics(m, 3)
        return out, list(lines)
    return run, run("host")


@pytest.mark.parametrize("capacity", [None, 8])
def test_get_metrics_is_the_same_in_both_modes(metric_runs, golden, capacity):
    """capacity 8: the record buffer is smaller than the first batch's bound, so it grows while the run goes on"""
    run, (host, host_lines) = metric_runs
    got, lines = run("device", capacity)
    assert sorted(got) == sorted(host) == ["ap", "fitness", "labels", "mAP50", "mAP50_95", "precision", "recall"]
    assert got["ap"].shape == (3, 10) and got["ap"].dtype == np.float64 and got["ap"].tobytes() == host["ap"].tobytes()
    assert got["labels"].tolist() == host["labels"].tolist() == [int(v) for v in golden("golden_dataset")["target_num"]]
    for k in ("precision", "recall", "mAP50", "mAP50_95", "fitness"):
        assert type(got[k]) is float and got[k] == host[k], k
    assert lines == host_lines and len(lines) == 5 and lines[1].split()[:3] == ["all", "20", str(int(got["labels"].sum()))]
    assert 0 < got["mAP50_95"] < got["mAP50"] <= 1 and got["fitness"] == 0.1 * got["mAP50"] + 0.9 * got["mAP50_95"]
    assert got["ap"][:, 0].min() > 0                                                   # every class is found


class _TB:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, name, value, step):
        self.scalars.append((name, value, step))


@pytest.fixture(scope="module")
def trained(yf, dev, tmp_path_factory):
    """train() for 7 epochs at batch 4 on the fixture tree, with and without val_metrics, same seeds"""
    from yolo_fastest_amd import training
    from yolo_fastest_amd.dataset import DetectDataset
    root = tmp_path_factory.mktemp("train")
    trees = voc_tree.make_trees(root / "voc")
    out = {}
    for tag, kw in (("metrics", dict(val_metrics=True)), ("plain", {})):
        log, lines = _logger("test-gpu-val-metrics-train-" + tag)
        params = copy.deepcopy(yf.config_params)
        params["io_params"]["save_path"] = str(root / tag)
        params["augment_params"] = voc_tree.aug_params(trees)
        params["train_params"].update(total_epochs=7, batch_size=4, pretrained_pth=WEIGHTS)
        shape = list(params["io_params"]["input_shape"])
        tr = DetectDataset(shape, [512, 640, 3], log, aug_params=voc_tree.aug_params(trees), max_boxes=64, device=dev, cache="device")
        va = DetectDataset(shape, [512, 640, 3], log, aug_params=voc_tree.aug_params(trees), max_boxes=64, device=dev, val=True, augment=False)
        tb = _TB()
        torch.manual_seed(0)
        random.seed(0)
        np.random.seed(0)
        training.train(params, dev, tb, train_dataset=tr, val_dataset=va, logger=log, **kw)
        out[tag] = (str(root / tag), tb.scalars, list(lines))
    return out


def test_best_checkpoint_is_the_epoch_of_the_best_logged_fitness(trained):
    from yolo_fastest_amd import metrics
    path, scalars, lines = trained["metrics"]
    logged = {name: {step: v for n, v, step in scalars if n == name} for name in
              ("metrics/precision", "metrics/recall", "metrics/mAP_0.5", "metrics/mAP_0.5:0.95")}
    assert all(sorted(v) == [5, 6] for v in logged.values())                           # the epochs get_mAP runs on: epoch > 4
    fit = {e: metrics.fitness(logged["metrics/mAP_0.5"][e], logged["metrics/mAP_0.5:0.95"][e]) for e in (5, 6)}
    best_epoch = 5 if fit[5] >= fit[6] else 6                                          # strictly better only: a tie stays with the earlier
    best = torch.load(os.path.join(path, "YOLO-Fastest_best.pth"), map_location="cpu")
    want = torch.load(os.path.join(path, "YOLO-Fastest_epoch_%d.pth" % best_epoch), map_location="cpu")
    assert list(best) == list(want) and all(torch.equal(best[k], want[k]) for k in want)
    other = torch.load(os.path.join(path, "YOLO-Fastest_epoch_%d.pth" % (11 - best_epoch)), map_location="cpu")
    assert not all(torch.equal(best[k], other[k]) for k in want)
    headers = [i for i, ln in enumerate(lines) if ln.split()[:2] == ["Class", "Images"]]
    assert len(headers) == 2 and all(lines[i - 1].startswith("———") and lines[i + 1].split()[0] == "all" for i in headers)   # behind get_mAP's


def test_without_val_metrics_nothing_new_is_written_or_logged(trained):
    path, scalars, lines = trained["plain"]
    _, _, with_lines = trained["metrics"]
    assert not os.path.exists(os.path.join(path, "YOLO-Fastest_best.pth"))
    assert sorted(f for f in os.listdir(path)) == sorted("YOLO-Fastest_epoch_%d.pth" % e for e in range(7))
    assert not [n for n, _, _ in scalars if n.startswith("metrics/")]
    assert not [ln for ln in lines if ln.split()[:2] == ["Class", "Images"]]

    def table(ln):
        return ln.split()[:1] in (["Class"], ["all"]) or (ln.split()[:1] in ([n] for n in NAMES) and len(ln.split()) == 7)

    def shape(run):                             # every line but the timing ones, digits masked: two trainings need not agree to the bit
        return [re.sub(r"[0-9.]+", "#", ln) for ln in run if "example/sec" not in ln]
    kept, plain = shape(with_lines), shape(lines)
    assert [ln for ln in kept if not table(ln)] == plain and len(kept) == len(plain) + 2 * (2 + len(NAMES))
