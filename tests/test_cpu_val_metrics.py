"""Host side of yolov5-style validation scoring: the matching rule against a literal transcription of yolov5's process_batch, metrics.py
against hand values and a loop form (tests/val_metrics_ref.py), `Validation.get_metrics(match="host")` on hand-built detections through a
stub model, and the C ABI's new entry (declared, bound, exported, refusing bad arguments before anything touches a GPU)."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest
import torch

from tests import val_metrics_ref as ref
from yolo_fastest_amd import _lib, metrics, validation as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _masks(correct):
    return (correct.astype(np.int64) << np.arange(correct.shape[1])).sum(1)


def test_direct_definition_equals_process_batch_where_no_iou_ties():
    """300 seeded images.  The test's own condition first: no detection has two same-class targets at one fp32 IoU that reaches the lowest
    threshold (below every threshold a tie cannot show in either form; at or above one, yolov5's result is its sort's)."""
    rng = np.random.default_rng(2024)
    hits = 0
    for i in range(300):
        det, tg = ref.random_image(rng, int(rng.integers(0, 60)), int(rng.integers(0, 24)))
        assert not ref.tied(det, tg, ref.IOUV[0]), i
        want = _masks(process := ref.process_batch_literal(det, tg, ref.IOUV))
        assert np.array_equal(ref.direct_hits(det, tg, ref.IOUV), want), i
        assert np.array_equal(V.match_iouv_image(det, tg, ref.IOUV), want), i
        hits += int(process.sum())
    assert hits > 3000                                       # the images are not trivially empty


@pytest.mark.parametrize("name", [c[0] for c in ref.CASES])
def test_host_matching_equals_the_direct_definition_on_the_kernel_cases(name):
    """validation.match_iouv_image (the vectorised form match="host" runs) on the cases the kernel is held to, ties and NaN included"""
    _, (det, counts, tg), thr = next(c for c in ref.CASES if c[0] == name)
    for i, count in enumerate(counts):
        n = min(max(int(count), 0), det.shape[1])
        assert np.array_equal(V.match_iouv_image(det[i, :n], tg[i], thr), ref.direct_hits(det[i, :n], tg[i], thr)), i


def test_the_case_table_has_the_hits_it_is_there_for():
    by = {c[0]: c for c in ref.CASES}
    full = (1 << 10) - 1

    def hits(name):
        _, (det, counts, tg), thr = by[name]
        return ref.direct_records(det, counts, tg, thr)[:, 3]
    for name in ("three_contest_winner_has_lowest_iou", "three_contest_winner_has_highest_iou"):
        h = hits(name)
        assert h[3] == full and h[70] == 0 and h[200] == 0 and not h[[k for k in range(ref.W) if k != 3]].any(), name
    h = hits("two_contest_across_waves_targets_at_0_and_T_minus_1")
    assert h[1] == 0x1FF and h[255] == 0x200 and h[64] == full and h[130] == 0   # 255 wins only at 0.95, where slot 1's 0.925 fails
    h = hits("special_values").reshape(4, -1)
    assert h[0, 0] == full and h[0, 1] == 0                   # the second detection's best is the same target 1: the lower slot has it
    assert h[0, 2] == 0 and h[0, 8] == 0 and h[0, 9] == 0     # wrong class; markers 1 and 0
    assert not h[0, 3:8].any() and h[0, 10] == full           # NaN / infinite corners
    assert h[2, 0] == full and not h[3].any()                 # a NaN target hands over to its duplicate; no targets at all
    assert [int(hits(n)[0]) for n in ("iou_is_the_threshold", "threshold_one_step_up", "threshold_one_step_down", "the_three_together")] \
        == [1, 0, 1, 0b011]
    assert len(hits("negative_and_huge_counts")) == 6 + 2 + 0 + 6 + 4 and len(hits("kmax_below_a_count")) == 20 + 12 + 20
    for name, c in by.items():
        if name.startswith(("n_", "T_")) and name not in ("T_0", "T_1"):
            h = hits(name)
            assert 0 < (h != 0).sum() < len(h) and len(set(h.tolist())) > 3, name


def test_compute_ap_hand_values():
    """a perfect ranking of 7: the envelope is 1 up to recall 1, where the 101-point rule reads the 0 sentinel: 99 intervals of 0.01 plus
    half of one.  TP FP TP FP with 2 labels: recall .5 .5 1 1, precision 1 .5 2/3 .5."""
    k = np.arange(1, 8)
    assert metrics.compute_ap(k / (7 + 1e-16), np.ones(7))[0] == 0.995
    ap, mpre, mrec = metrics.compute_ap(np.array([1, 1, 2, 2]) / (2 + 1e-16), np.array([1, 1 / 2, 2 / 3, 2 / 4]))
    assert ap == 0.8283333333333331
    assert mrec.tolist() == [0, 0.5, 0.5, 1, 1, 1] and mpre.tolist() == [1, 1, 2 / 3, 2 / 3, 0.5, 0]
    assert metrics.fitness(0.5, 0.25) == 0.1 * 0.5 + 0.9 * 0.25


def test_a_class_without_detections_or_without_labels_has_a_zero_row():
    tp = np.array([[1, 1], [0, 0], [1, 0], [1, 1]], bool)
    conf = np.array([0.9, 0.8, 0.7, 0.6])
    with np.errstate(all="raise"):
        p, r, f1, ap = metrics.ap_per_class(tp, conf, np.array([0, 0, 0, 2]), np.array([2, 3, 0, 0]))      # class 1: no detections; 2: no labels
        assert ap.shape == (4, 2) and ap[0, 0] > 0.8 and not ap[1:].any() and not p[1:].any() and not r[1:].any() and not f1[1:].any()
        for out in metrics.ap_per_class(np.zeros((0, 2), bool), np.zeros(0), np.zeros(0, int), np.array([2, 3, 0])):   # nothing detected
            assert not out.any()
        for out in metrics.ap_per_class(tp, conf, np.array([0, 0, 0, 2]), np.zeros(3, int)):                  # nothing labelled
            assert not out.any()


def _flags(seed, n, nthr=10, ncls=3, ties=False):
    rng = np.random.default_rng(seed)
    conf = rng.uniform(0.001, 1, n).astype(np.float32).astype(np.float64)
    if ties:
        conf = np.round(conf, 1)                               # eleven values: long runs of equal confidences
    level = rng.uniform(size=n)
    tp = level[:, None] > np.linspace(0.3, 0.9, nthr)[None]    # a detection right at threshold j is right at every lower one
    cls = rng.integers(0, ncls, n)
    labels = np.array([tp[cls == c, 0].sum() for c in range(ncls)]) + rng.integers(1, 6, ncls)     # no more true positives than labels
    return tp, conf, cls, labels


@pytest.mark.parametrize("seed,n,ties", [(0, 200, False), (1, 37, False), (2, 300, True), (3, 1, False)])
def test_ap_per_class_against_the_loop_form(seed, n, ties):
    tp, conf, cls, labels = _flags(seed, n, ties=ties)
    labels[1] = 0 if seed == 1 else labels[1]
    got, want = metrics.ap_per_class(tp, conf, cls, labels), ref.ap_per_class_loops(tp, conf, cls, labels)
    for g, w, what in zip(got, want, ("p", "r", "f1", "ap")):
        assert g.shape == w.shape and np.abs(g - w).max() <= 1e-12, (what, np.abs(g - w).max())
    assert got[3][labels > 0].any() or n == 1


def test_tied_confidences_keep_slot_order():
    """TP then FP at one confidence is not FP then TP: with a stable ranking the order given decides, and reversing it changes the AP"""
    tp = np.array([[1], [0], [1], [0]], bool)
    conf, cls, labels = np.full(4, 0.5), np.zeros(4, int), np.array([2])
    a = metrics.ap_per_class(tp, conf, cls, labels)[3][0, 0]
    b = metrics.ap_per_class(tp[::-1], conf, cls, labels)[3][0, 0]
    assert a == 0.8283333333333331 and b == ref.ap_per_class_loops(tp[::-1], conf, cls, labels)[3][0, 0] and b < 0.6
    tp, conf, cls, labels = _flags(5, 120, ties=True)
    order = np.argsort(-conf, kind="stable")
    got = metrics.ap_per_class(tp, conf, cls, labels)[3]
    assert np.array_equal(got, metrics.ap_per_class(tp[order], conf[order], cls[order], labels)[3])          # already ranked: nothing moves


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_get_metrics_host_mode_on_hand_built_detections(monkeypatch):
    """`get_metrics(match="host")` with the forward, the decode and the NMS stubbed out (they need a GPU): two batches of two images whose
    detections and targets are written here.  Class 0: three labels, found with IoU 1, 0.92 and not at all; class 1: one label, found at
    IoU 0.72 by the second-ranked of two detections; class 2: no labels, one detection."""
    names = ["carrier", "defender", "destroyer"]
    params = {"train_params": {"batch_size": 2, "IOU_val_thre": 0.5},
              "io_params": {"input_shape": (100, 100, 1), "num_cls": 3, "class_names": names, "conf_thre": 0.5, "nms_thre": 0.2}}

    def boxes(*rows):
        t = np.zeros((64, 6), np.float32)
        for i, (x1, y1, x2, y2, c) in enumerate(rows):
            t[i] = ((x1 + x2) / 200, (y1 + y2) / 200, (x2 - x1) / 100, (y2 - y1) / 100, c, 255)   # normalised centre form, as the data set's
        return t
    items = [(np.zeros((100, 100, 1), np.float32), boxes((10, 10, 50, 50, 0), (60, 60, 90, 90, 1))),
             (np.zeros((100, 100, 1), np.float32), boxes((20, 20, 60, 60, 0))),
             (np.zeros((100, 100, 1), np.float32), boxes((0, 0, 40, 40, 0))),
             (np.zeros((100, 100, 1), np.float32), boxes())]
    dets = [[(10, 10, 50, 50, 0.9, 1.0, 0), (60, 60, 90, 81.6, 0.5, 1.0, 1), (0, 0, 5, 5, 0.8, 1.0, 1)],
            [(20, 20, 60, 56.8, 0.8, 0.5, 0)], None, [(5, 5, 30, 30, 0.3, 1.0, 2)]]
    log = logging.getLogger("test-cpu-val-metrics")
    log.setLevel(logging.INFO)
    log.propagate = False
    lines = _Lines()
    log.addHandler(lines)
    val = V.Validation(params, log, items, "cpu", [lambda p: p], match="host")
    val.dataloader = [V.collate_fn(items[:2]), V.collate_fn(items[2:])]                            # in order, no shuffling
    calls = []

    def nms(output, num_cls, conf_thres, nms_thres, model):
        calls.append((conf_thres, nms_thres))
        at = 2 * (len(calls) - 1)
        return [None if d is None else torch.tensor(d, dtype=torch.float32) for d in dets[at:at + 2]]
    monkeypatch.setattr(V, "non_max_suppression", nms)

    class Model:
        def eval(self): pass
        def __call__(self, imgs): return [imgs.reshape(imgs.shape[0], 1, -1)]
    out = val.get_metrics(Model(), 7)
    assert calls == [(0.001, 0.6)] * 2 and out["labels"].tolist() == [3, 1, 0]
    half = metrics.compute_ap(np.array([0.0, 1.0]) / (1 + 1e-16), np.array([0.0, 0.5]))[0]                  # class 1: FP (0.8), then the TP (0.5)
    two = metrics.compute_ap(np.array([1.0, 2.0]) / (3 + 1e-16), np.ones(2))[0]                    # class 0: two of three, no FP
    one = metrics.compute_ap(np.array([1.0, 1.0]) / (3 + 1e-16), np.array([1.0, 0.5]))[0]          # ... and at 0.95 only the first
    want = np.zeros((3, 10))
    want[0, :9], want[0, 9] = two, one                                                             # IoU 0.92: passes 0.5 .. 0.9
    want[1, :5] = half                                                                             # IoU 0.72: passes 0.5 .. 0.7
    assert np.array_equal(out["ap"], want)
    assert out["mAP50"] == (two + half) / 2 and out["mAP50_95"] == (want[0].mean() + want[1].mean()) / 2
    assert out["fitness"] == 0.1 * out["mAP50"] + 0.9 * out["mAP50_95"]
    assert 0 < out["precision"] <= 1 and 0 < out["recall"] < 1
    row = "%20s" + "%11i" * 2 + "%11.3g" * 4
    assert lines.lines[0] == ("%20s" + "%11s" * 6) % ("Class", "Images", "Labels", "P", "R", "mAP@.5", "mAP@.5:.95")
    assert lines.lines[1] == row % ("all", 4, 4, out["precision"], out["recall"], out["mAP50"], out["mAP50_95"])
    assert len(lines.lines) == 5 and lines.lines[4] == row % ("destroyer", 4, 0, 0, 0, 0, 0)
    assert lines.lines[2].split()[:3] == ["carrier", "4", "3"] and float(lines.lines[2].split()[5]) == float("%.3g" % two)
    assert val.match_list == [[], [], []] and not val.target_num.any()                             # get_mAP's state is not touched
    for bad in ([], [0.5] * 17, [0.5, float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            val.get_metrics(Model(), 7, iouv=bad)


def test_header_bindings_and_exports_carry_the_new_entry():
    hdr = open(os.path.join(ROOT, "include", "yolo_fastest_hip.h")).read()
    m = re.search(r"^int yf_val_match_iouv\(([^;]*)\);", hdr, re.M)
    assert m and re.sub(r"\s+", " ", m.group(1)) == (
        "int device, const float *d_det, const int32_t *d_counts, int N, int K_max, const float *d_targets, int T, "
        "const double *iou_thresholds, int num_thresholds, const int64_t *d_base, int64_t *d_next, int32_t *d_records, int64_t cap, void *stream")
    assert "yf_val_match_iouv" in _lib.EXPORTS and len(_lib._SIGS["yf_val_match_iouv"][1]) == 14
    lib = _lib.lib()
    assert hasattr(lib, "yf_val_match_iouv") and lib.yf_abi_version() == 1 == _lib.ABI_VERSION
    assert re.search(r"#define\s+YF_ABI_VERSION\s+1\b", hdr)


def test_val_match_iouv_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_int64 * 8)()                      # host memory: a call that got past the checks would fail, not be refused
    p = ctypes.addressof(buf)
    good = dict(device=0, det=p, counts=p, N=2, K=4, targets=p, T=3, thr=[0.5, 0.75], nthr=None, base=p, next=p + 8, rec=p, cap=16)

    def call(**kw):
        a = dict(good, **kw)
        thr = None if a["thr"] is None else (ctypes.c_double * max(len(a["thr"]), 1))(*a["thr"])
        nthr = len(a["thr"]) if a["nthr"] is None else a["nthr"]
        return lib.yf_val_match_iouv(a["device"], a["det"], a["counts"], a["N"], a["K"], a["targets"], a["T"], thr, nthr, a["base"], a["next"],
                                     a["rec"], a["cap"], None)
    for name in ("det", "counts", "targets", "base", "next", "rec"):
        assert call(**{name: None}) == _lib.YF_E_INVALID, name
        assert b"null pointer" in lib.yf_last_error_string()
    assert call(thr=None, nthr=2) == _lib.YF_E_INVALID and b"null pointer" in lib.yf_last_error_string()
    nan, inf = float("nan"), float("inf")
    for kw in (dict(N=0), dict(N=-1), dict(K=0), dict(K=-3), dict(T=-1), dict(cap=-1), dict(T=513), dict(next=p), dict(thr=[], nthr=0),
               dict(nthr=-1), dict(thr=[0.5] * 17), dict(thr=[0.5, nan]), dict(thr=[inf]), dict(thr=[0.5, -inf, 0.6]), dict(thr=[1e300])):
        assert call(**kw) == _lib.YF_E_INVALID, kw
        assert b"yf_val_match_iouv" in lib.yf_last_error_string()
