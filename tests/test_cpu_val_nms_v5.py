"""Host side of yolov5's NMS on the device (yf_val_nms_v5): the numpy rule the kernel is held to against a transcription of yolov5's own
code (tests/val_nms_v5_ref.py), the C ABI's two new symbols (declared, bound, exported, refusing bad arguments before anything touches
a GPU), and the Python arguments that raise."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest

from tests import val_nms_v5_ref as ref
from yolo_fastest_amd import _lib, training, validation as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_equals_yolov5s_code_where_scores_are_distinct():
    """300 seeded images, every mode and a spread of thresholds and caps.  The test's own condition first: the candidates' scores are
    distinct (on equal scores yolov5's order is its unstable sort's; the rule's index order is this library's definition)."""
    rng = np.random.default_rng(61)
    kept = cut_det = cut_nms = suppressed = 0
    for i in range(300):
        M, C = int(rng.integers(1, 70)), int(rng.choice([1, 2, 3, 20]))
        multi, agnostic = bool(i & 1), bool(i & 2)
        conf = float(rng.choice([0.001, 0.1, 0.25]))
        iou = float(rng.choice([0.3, 0.45, 0.6]))
        max_det = int(rng.choice([300, 300, 5]))
        max_nms = int(rng.choice([30000, 30000, 12]))
        pred = ref.random_image(rng, M, C)
        if i % 7 == 0:
            pred[rng.integers(0, M), 4] = 0.0                     # a row below every threshold
        while not ref.scores_distinct(pred, conf, multi):
            pred[:, 4:] = rng.uniform(0, 1, (M, 1 + C))
        n_cand = len(ref.candidates(pred, conf, multi))
        want = ref.yolov5_literal(pred, conf, iou, agnostic, multi, max_det, max_nms)
        got7 = ref.rule(pred, conf, iou, multi, agnostic, max_det, max_nms)
        got = ref.to_yolov5(got7)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (i, M, C, multi, agnostic, conf, iou, max_det, max_nms)
        kept += len(got)
        cut_det += len(got) == max_det
        cut_nms += n_cand > max_nms
        suppressed += min(n_cand, max_nms) - len(got)
    assert kept > 2000 and suppressed > 2000 and cut_det > 20 and cut_nms > 20     # the images are not trivial


def test_the_vectorised_walk_is_the_scalar_iou():
    """`rule`'s inner loop is one numpy expression per kept rank; `iou_pair` is the same float32 operations on scalars"""
    rng = np.random.default_rng(62)
    pred = ref.random_image(rng, 40, 3)
    pred[7, :4] = pred[3, :4]                                     # IoU 1 within a class pair
    pred[9, 2:4] = 0                                              # zero area
    pred[11, 0] = np.nan
    rows, classes = list(range(40)), [int(v) for v in rng.integers(0, 3, 40)]
    _, b, area = ref.offset_boxes(pred, rows, classes, False)
    for i in range(0, 40, 3):
        with np.errstate(all="ignore"):
            dx = ref.std_min(b[i, 2], b[:, 2]) - ref.std_max(b[i, 0], b[:, 0])
            dy = ref.std_min(b[i, 3], b[:, 3]) - ref.std_max(b[i, 1], b[:, 1])
            inter = ref.std_max(np.float32(0), dx) * ref.std_max(np.float32(0), dy)
            iou = inter / (area[i] + area - inter)
        for q in range(40):
            assert np.array_equal(iou[q], ref.iou_pair(b[i], b[q]), equal_nan=True), (i, q)
    assert ref.iou_pair(b[3], b[7]) == 1 or classes[3] != classes[7]
    assert np.isnan(ref.iou_pair(b[9], b[9]))                     # 0 / 0


def test_the_case_table_has_what_it_is_there_for():
    """the kernel cases of tests/test_gpu_val_nms_v5.py, by the rule alone: each edge case does what its name says"""
    budget, static = _lib.YF_VAL_NMS_V5_LDS_BUDGET, _lib.YF_VAL_NMS_V5_LDS_STATIC
    by = {c[0]: c for c in ref.build_cases(budget, static)}

    def counts(name):
        _, pred, args, kmax = by[name]
        return ref.rule_batch(pred, kmax, -1.0, **args)[1].tolist()
    assert counts("zero_candidates") == [0] and counts("M1_C1_multi1") == [1]
    assert counts("obj_at_conf_thres_and_its_neighbours") == [1]
    assert counts("score_at_conf_thres_obj_above") == [2] and counts("score_at_conf_thres_obj_above_single_label") == [2]
    assert counts("two_classes_of_one_row_identical_boxes") == [2] and counts("two_classes_of_one_row_identical_boxes_agnostic") == [1]
    _, pred, args, _ = by["argmax_of_products_is_not_argmax_of_class_scores"]
    d = ref.rule(pred[0], **args)
    assert len(d) == 1 and d[0, 6] == 0 and pred[0, 0, 5:].argmax() == 1
    multi = ref.rule(by["equal_scores_across_rows_and_within_one_multi"][1][0], **by["equal_scores_across_rows_and_within_one_multi"][2])
    assert multi[:2, 6].tolist() == [0, 1] and (multi[:2, :4] == multi[0, :4]).all()          # one row, equal scores: class order
    assert [counts(n) for n in ("iou_is_the_threshold", "threshold_one_step_down", "threshold_one_step_up")] == [[2], [1], [2]]
    assert counts("zero_area_boxes") == [14]                                                  # 0 / 0 suppresses nothing
    assert [counts("max_nms_%d_a_survivor_just_beyond" % n) for n in (1, 8, 30000)] == [[1], [2], [3]]
    assert counts("K_max_below_the_count")[0] > by["K_max_below_the_count"][3] == 3
    three = counts("three_images_with_different_counts")
    assert three[1] == 0 and len(set(three)) == 3
    _, pred, args, _ = by["coordinates_of_1e4_offset_does_not_separate"]
    alone = 0                                                                                 # each class on its own: no other class to meet
    for c in range(3):
        one = pred[0].copy()
        one[:, 5:] = 0
        one[:, 5 + c] = pred[0][:, 5 + c]
        alone += len(ref.rule(one, **dict(args, max_det=10 ** 6)))
    assert len(ref.rule(pred[0], **dict(args, max_det=10 ** 6))) < alone                      # boxes of different classes met
    limit = ref.lds_tier_limit(budget, static)
    assert 9 * limit + static <= budget < 9 * 2 * limit + static
    for name, bound in (("workspace_tier_all_rows_candidates", limit + 1), ("workspace_tier_max_nms_cuts", limit + 1),
                        ("workspace_tier_single_label", limit + 1), ("last_lds_tier_size", limit)):
        _, pred, args, _ = by[name]
        assert (pred.shape[1] * (pred.shape[2] - 5) if args["multi_label"] else pred.shape[1]) == bound
        assert len(ref.candidates(pred[0], args["conf_thres"], args["multi_label"])) == bound     # all rows are candidates


def test_header_bindings_and_exports_carry_both_symbols():
    hdr = open(os.path.join(ROOT, "include", "yolo_fastest_hip.h")).read()
    m = re.search(r"^int yf_val_nms_v5\(([^;]*)\);", hdr, re.M)
    assert m and re.sub(r"\s+", " ", m.group(1)) == (
        "int device, const float *d_pred, int N, int M, int num_classes, double conf_thres, double iou_thres, "
        "int multi_label, int agnostic, int max_det, int max_nms, int K_max, "
        "void *d_work, size_t work_bytes, float *d_det, int32_t *d_counts, void *stream")
    m = re.search(r"^size_t yf_val_nms_v5_work_bytes\(([^;]*)\);", hdr, re.M)
    assert m and re.sub(r"\s+", " ", m.group(1)) == "int N, int M, int num_classes, int multi_label"
    assert "yf_val_nms_v5" in _lib.EXPORTS and len(_lib._SIGS["yf_val_nms_v5"][1]) == 17
    assert "yf_val_nms_v5_work_bytes" in _lib.EXPORTS and _lib._SIGS["yf_val_nms_v5_work_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    lib = _lib.lib()
    assert hasattr(lib, "yf_val_nms_v5") and hasattr(lib, "yf_val_nms_v5_work_bytes") and lib.yf_abi_version() == 1 == _lib.ABI_VERSION
    assert re.search(r"#define\s+YF_ABI_VERSION\s+1\b", hdr)
    for name in ("YF_VAL_NMS_V5_LDS_BUDGET", "YF_VAL_NMS_V5_LDS_STATIC"):     # the constants the tier is documented by
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == getattr(_lib, name)
    assert "parity with a real torchvision build is" in re.sub(r"\s*\n \*\s*", " ", hdr)


def _pad(n):
    p = 64
    while p < n:
        p <<= 1
    return p


def test_work_bytes():
    """N images x (keys + liveness bytes) of the candidate bound padded to a power of two; 0 for arguments the entry refuses"""
    lib = _lib.lib()
    for N, M, C, multi in ((1, 1, 1, 0), (3, 65, 20, 1), (3, 65, 20, 0), (2, 1025, 1, 1), (1, 16385, 1, 0), (1, 3277, 5, 1),
                           (1, 2 ** 31 - 1, 1, 1), (1, 46340, 46340, 1)):
        assert lib.yf_val_nms_v5_work_bytes(N, M, C, multi) == N * 9 * _pad(M * C if multi and C > 1 else M), (N, M, C, multi)
    for N, M, C in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 5, 5), (1, 46341, 46341), (1, 2 ** 31 - 1, 2)):
        assert lib.yf_val_nms_v5_work_bytes(N, M, C, 1) == 0 and lib.yf_val_nms_v5_work_bytes(N, M, C, 0) == 0


def test_val_nms_v5_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_int64 * 8)()                      # host memory: a call that got past the checks would fail, not be refused
    p = ctypes.addressof(buf)
    good = dict(device=0, pred=p, N=2, M=40, C=3, conf=0.25, iou=0.45, multi=1, agnostic=0, max_det=300, max_nms=30000, K=300, work=p,
                work_bytes=2 * 9 * 128, det=p, counts=p)
    assert lib.yf_val_nms_v5_work_bytes(2, 40, 3, 1) == good["work_bytes"]

    def call(**kw):
        a = dict(good, **kw)
        return lib.yf_val_nms_v5(a["device"], a["pred"], a["N"], a["M"], a["C"], a["conf"], a["iou"], a["multi"], a["agnostic"], a["max_det"],
                                 a["max_nms"], a["K"], a["work"], a["work_bytes"], a["det"], a["counts"], None)
    for name in ("pred", "work", "det", "counts"):
        assert call(**{name: None}) == _lib.YF_E_INVALID, name
        assert b"yf_val_nms_v5" in lib.yf_last_error_string() and b"null pointer" in lib.yf_last_error_string()
    nan = float("nan")
    for kw in (dict(N=0), dict(N=-1), dict(M=0), dict(M=-7), dict(C=0), dict(C=-1), dict(M=46341, C=46341, work_bytes=1 << 62),
               dict(M=2 ** 31 - 1, C=2, work_bytes=1 << 62), dict(conf=nan), dict(conf=-0.001), dict(conf=-float("inf")), dict(iou=nan),
               dict(max_det=0), dict(max_det=-1), dict(max_nms=0), dict(max_nms=-5), dict(K=0), dict(K=-1),
               dict(work_bytes=good["work_bytes"] - 1), dict(work_bytes=0), dict(multi=0, work_bytes=2 * 9 * 64 - 1)):
        assert call(**kw) == _lib.YF_E_INVALID, kw
        assert b"yf_val_nms_v5" in lib.yf_last_error_string(), kw


def _validation():
    params = {"train_params": {"batch_size": 2, "IOU_val_thre": 0.5},
              "io_params": {"input_shape": (100, 100, 1), "num_cls": 3, "class_names": ["a", "b", "c"], "conf_thre": 0.5, "nms_thre": 0.2}}
    log = logging.getLogger("test-cpu-val-nms-v5")
    log.propagate = False
    return V.Validation(params, log, [0, 1], "cpu", [lambda p: p], match="host")      # (the items are never read)


def test_get_metrics_and_train_refuse_what_they_do_not_know():
    class Model:
        def eval(self):
            raise AssertionError("refused before the model is touched")
    val = _validation()
    for bad in ("bogus", "v5", None, "YOLOV5"):
        with pytest.raises(ValueError, match="nms must be"):
            val.get_metrics(Model(), 0, nms=bad)
    with pytest.raises(ValueError, match="max_det"):
        val.get_metrics(Model(), 0, nms="yolov5", max_det=0)
    assert V.NMS_KINDS == ("reference", "yolov5")
    params = {"io_params": {}, "train_params": {}}
    with pytest.raises(ValueError, match="val_metrics=True"):
        training.train(params, "cpu", train_dataset=[0], val_nms="yolov5")
    with pytest.raises(ValueError, match="val_nms must be"):
        training.train(params, "cpu", train_dataset=[0], val_metrics=True, val_nms="bogus")


def test_non_max_suppression_v5_has_yolov5s_arguments_and_needs_device_tensors():
    import inspect
    import torch
    sig = inspect.signature(V.non_max_suppression_v5)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [
        ("conf_thres", 0.25), ("iou_thres", 0.45), ("agnostic", False), ("multi_label", False), ("max_det", 300), ("max_nms", 30000),
        ("model", None)]
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        V.non_max_suppression_v5(torch.zeros(1, 4, 8))
