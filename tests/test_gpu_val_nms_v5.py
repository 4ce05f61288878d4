"""yolov5's NMS on the device: val_nms_v5_kernel behind yf_val_nms_v5 against the numpy rule (tests/val_nms_v5_ref.py, itself held to a
transcription of yolov5's code by tests/test_cpu_val_nms_v5.py), then `Validation.get_metrics(nms="yolov5")` and
`train(..., val_nms="yolov5")`.

  * kernel: d_det and d_counts bit for bit, and every slot the entry must not write still holding its sentinel.  No tolerance: the rule is
    fp32 mul / add / sub / div / compare in one stated order, the ranking is a total order (score, then candidate index), and the walk is
    sequential by definition.
  * the workspace tier's size comes from the budget the header documents (YF_VAL_NMS_V5_LDS_BUDGET), not from the path the code takes.
  * get_metrics(nms="yolov5") on the VOC fixture tree: the same dict (`ap` bitwise) and log lines in both matching modes, its detections
    those of the rule on the decoded predictions read back; nms="reference" is get_metrics() as it was."""
import copy
import ctypes
import logging
import os
import random
import sys

import numpy as np
import pytest
import torch

from tests import val_nms_v5_ref as ref
from yolo_fastest_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import voc_tree  # noqa: E402

WEIGHTS = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_256x320_epoch28.pth")
SENTINEL = -7777.0
NAMES = ["carrier", "defender", "destroyer"]
CASES = ref.build_cases(_lib.YF_VAL_NMS_V5_LDS_BUDGET, _lib.YF_VAL_NMS_V5_LDS_STATIC)


@pytest.fixture(scope="module")
def yf():
    import yolo_fastest_amd
    return yolo_fastest_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nms(dev, pred, kmax, conf_thres, iou_thres, multi_label, agnostic, max_det, max_nms):
    """yf_val_nms_v5 through the C ABI into sentinel-filled buffers -> (det [N, kmax + 1, 7] with one guard row per image at the end of
    the whole buffer, counts [N]) on the host"""
    lib = _lib.lib()
    N, M, C = pred.shape[0], pred.shape[1], pred.shape[2] - 5
    d_pred = torch.from_numpy(pred).to(dev)
    det = torch.full((N * kmax + 4, 7), SENTINEL, dtype=torch.float32, device=dev)
    cnt = torch.full((N + 2,), -9, dtype=torch.int32, device=dev)
    need = lib.yf_val_nms_v5_work_bytes(N, M, C, int(multi_label))
    assert need == N * 9 * max(64, 1 << (((M * C if multi_label and C > 1 else M) - 1).bit_length()))
    work = torch.zeros(need // 8 + 1, dtype=torch.int64, device=dev)
    rc = lib.yf_val_nms_v5(dev.index, d_pred.data_ptr(), N, M, C, conf_thres, iou_thres, int(multi_label), int(agnostic), max_det, max_nms,
                           kmax, work.data_ptr(), need, det.data_ptr(), cnt.data_ptr(),
                           ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, lib.yf_last_error_string()
    torch.cuda.synchronize(dev)
    det, cnt = det.cpu().numpy(), cnt.cpu().numpy()
    assert (det[N * kmax:] == SENTINEL).all() and (cnt[N:] == -9).all()                # nothing behind the buffers
    return det[:N * kmax].reshape(N, kmax, 7), cnt[:N]


def _bits(a):
    """float32 -> its bits, every NaN as one pattern: WHICH NaN an `inf - inf` yields is the processor's choice (x86 sets the sign bit,
    the GPU does not), and the rule only says that it is one"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.int32(0x7FC00000), a.view(np.int32))


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_detections_equal_the_rule(dev, name):
    _, pred, args, kmax = next(c for c in CASES if c[0] == name)
    want, want_counts = ref.rule_batch(pred, kmax, SENTINEL, **args)
    got, counts = _nms(dev, pred, kmax, **args)
    assert counts.tolist() == want_counts.tolist()
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:8]


def test_refusals_leave_the_buffers_alone(dev):
    """every YF_E_INVALID of the header with real device buffers behind the pointers: det and counts keep their sentinels"""
    lib = _lib.lib()
    pred = torch.from_numpy(ref.random_image(np.random.default_rng(3), 40, 3, low=0.6)).to(dev)
    det = torch.full((300, 7), SENTINEL, dtype=torch.float32, device=dev)
    cnt = torch.full((1,), -9, dtype=torch.int32, device=dev)
    need = lib.yf_val_nms_v5_work_bytes(1, 40, 3, 1)
    work = torch.zeros(need // 8, dtype=torch.int64, device=dev)
    good = dict(pred=pred.data_ptr(), N=1, M=40, C=3, conf=0.25, iou=0.45, multi=1, agnostic=0, max_det=300, max_nms=30000, K=300,
                work=work.data_ptr(), work_bytes=need, det=det.data_ptr(), counts=cnt.data_ptr())
    nan = float("nan")
    bad = [{k: None} for k in ("pred", "work", "det", "counts")] + [
        dict(N=0), dict(M=0), dict(C=0), dict(M=46341, C=46341), dict(conf=nan), dict(conf=-1e-9), dict(iou=nan), dict(max_det=0),
        dict(max_nms=0), dict(K=0), dict(work_bytes=need - 1)]
    for kw in bad:
        a = dict(good, **kw)
        rc = lib.yf_val_nms_v5(dev.index, a["pred"], a["N"], a["M"], a["C"], a["conf"], a["iou"], a["multi"], a["agnostic"], a["max_det"],
                               a["max_nms"], a["K"], a["work"], a["work_bytes"], a["det"], a["counts"],
                               ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == _lib.YF_E_INVALID and b"yf_val_nms_v5" in lib.yf_last_error_string(), kw
    torch.cuda.synchronize(dev)
    assert bool((det == SENTINEL).all()) and bool((cnt == -9).all())


def test_non_max_suppression_v5_returns_yolov5s_rows(dev):
    """[n, 6] per image, conf = obj * cls as a float32 product, an empty [0, 6] tensor where nothing is kept"""
    from yolo_fastest_amd import validation as V
    _, pred, args, _ = next(c for c in CASES if c[0] == "three_images_with_different_counts")
    out = V.non_max_suppression_v5(torch.from_numpy(pred).to(dev), args["conf_thres"], args["iou_thres"], multi_label=True)
    assert len(out) == 3 and out[1].shape == (0, 6) and out[1].dtype == torch.float32 and out[1].device.type == "cuda"
    for got, p in zip(out, pred):
        want = ref.to_yolov5(ref.rule(p, **args))
        assert got.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        V.non_max_suppression_v5(torch.from_numpy(pred).to(dev), conf_thres=1.5)


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
    """get_metrics over the VOC fixture tree (20 frames, batch 4, shuffled under one seed) with the shipped 256x320 weights"""
    from yolo_fastest_amd import validation as V
    from yolo_fastest_amd.dataset import DetectDataset
    io = yf.io_params_for(256)
    m = yf.YoloFastest(io).to(dev).eval()
    m.load_state_dict(torch.load(WEIGHTS, map_location=dev))
    trees = voc_tree.make_trees(tmp_path_factory.mktemp("voc"))
    params = {"train_params": {"batch_size": 4, "IOU_val_thre": 0.5}, "io_params": dict(io, class_names=NAMES)}

    def run(match, **kw):
        log, lines = _logger("test-gpu-val-nms-v5-%s" % match)
        losses = [V.YOLOLossV3(io["anchors"][i], io["num_cls"], io["input_shape"], dev) for i in range(2)]
        ds = DetectDataset([256, 320, 1], [512, 640, 3], log, aug_params=voc_tree.aug_params(trees), max_boxes=64, device=dev, val=True,
                           augment=False)
        val = V.Validation(params, log, ds, dev, losses, match=match)
        del lines[:]
        torch.manual_seed(0)
        out = val.get_metrics(m, 3, **kw)
        return out, list(lines), val
    return run, m


def _same(a, b):
    assert sorted(a) == sorted(b) == ["ap", "fitness", "labels", "mAP50", "mAP50_95", "precision", "recall"]
    assert a["ap"].shape == b["ap"].shape and a["ap"].tobytes() == b["ap"].tobytes() and a["labels"].tolist() == b["labels"].tolist()
    for k in ("precision", "recall", "mAP50", "mAP50_95", "fitness"):
        assert type(a[k]) is float and a[k] == b[k], k


def test_get_metrics_with_yolov5s_nms_in_both_modes_and_its_detections(metric_runs, dev):
    from yolo_fastest_amd import validation as V
    run, m = metric_runs
    host, host_lines, _ = run("host", nms="yolov5")
    got, lines, val = run("device", nms="yolov5")
    _same(got, host)
    assert lines == host_lines and len(lines) == 5 and lines[1].split()[:2] == ["all", "20"]
    assert 0 < got["mAP50_95"] < got["mAP50"] <= 1 and got["ap"][:, 0].min() > 0
    # the same pass by hand: the loader's batches under the same seed, forward and decode on the device, the rule on what is read back
    total = 0
    torch.manual_seed(0)
    with torch.no_grad():
        for imgs, _ in val.dataloader:
            pred = m(imgs.to(dev).float())
            output = torch.cat([val.model_loss[i](p) for i, p in enumerate(pred)], 1)
            dets = V.non_max_suppression_v5(output, 0.001, 0.6, agnostic=False, multi_label=True, max_det=300, max_nms=30000)
            for d, p in zip(dets, output.cpu().numpy()):
                want = ref.to_yolov5(ref.rule(p, 0.001, 0.6, multi_label=True, agnostic=False, max_det=300, max_nms=30000))
                assert d.cpu().numpy().tobytes() == want.tobytes()
                total += len(want)
    assert total == val.metrics_detections > 20
    _, _, val5 = run("device", nms="yolov5", max_det=5)                               # max_det reaches the entry
    assert 0 < val5.metrics_detections <= 20 * 5 and val5.metrics_detections < total


def test_the_reference_nms_is_get_metrics_as_it_was(metric_runs):
    run, _ = metric_runs
    plain, plain_lines, val = run("device")
    named, named_lines, val2 = run("device", nms="reference", max_det=1)              # max_det is not read with "reference"
    _same(plain, named)
    assert plain_lines == named_lines and val.metrics_detections == val2.metrics_detections
    other, _, val3 = run("device", nms="yolov5")
    assert val3.metrics_detections != val.metrics_detections                           # (the two rules keep different detections)


def test_train_with_yolov5s_nms_writes_the_best_checkpoint(yf, dev, tmp_path):
    from yolo_fastest_amd import training
    from yolo_fastest_amd.dataset import DetectDataset
    trees = voc_tree.make_trees(tmp_path / "voc")
    log, lines = _logger("test-gpu-val-nms-v5-train")
    params = copy.deepcopy(yf.config_params)
    params["io_params"]["save_path"] = str(tmp_path / "out")
    params["augment_params"] = voc_tree.aug_params(trees)
    params["train_params"].update(total_epochs=7, batch_size=4, pretrained_pth=WEIGHTS)
    shape = list(params["io_params"]["input_shape"])
    tr = DetectDataset(shape, [512, 640, 3], log, aug_params=voc_tree.aug_params(trees), max_boxes=64, device=dev, cache="device")
    va = DetectDataset(shape, [512, 640, 3], log, aug_params=voc_tree.aug_params(trees), max_boxes=64, device=dev, val=True, augment=False)
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    training.train(params, dev, None, train_dataset=tr, val_dataset=va, logger=log, val_metrics=True, val_nms="yolov5")
    best = torch.load(os.path.join(str(tmp_path / "out"), "YOLO-Fastest_best.pth"), map_location="cpu")
    epochs = [torch.load(os.path.join(str(tmp_path / "out"), "YOLO-Fastest_epoch_%d.pth" % e), map_location="cpu") for e in (5, 6)]
    assert any(list(best) == list(w) and all(torch.equal(best[k], w[k]) for k in w) for w in epochs)
    assert len([ln for ln in lines if ln.split()[:2] == ["Class", "Images"]]) == 2
