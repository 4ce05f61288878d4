"""References for yf_val_nms_v5 (yolov5's non_max_suppression, include/yolo_fastest_hip.h states the rule), neither importing the package:
  * `rule`: the header's rule for one image in numpy float32, step by step: candidates row by row and class by class, the ranking as a
    sort on (score descending, candidate index ascending), the greedy walk rank by rank.  The walk's inner loop over the later ranks is
    one numpy expression per rank -- elementwise float32, the same operations in the same order as a scalar loop; `iou_pair` is that
    scalar form, and tests/test_cpu_val_nms_v5.py holds the two together;
  * `yolov5_literal`: the same the way yolov5 v6.1 / v7.0 writes it with torch CPU ops (boolean masks, nonzero, max, argsort, the class
    offset, then an `nms` that restates torchvision's CPU kernel with a Python loop over the ranks).  torch's argsort is unstable on equal
    scores, so the two are compared on images whose candidate scores are distinct;
  * `random_image`: seeded rows with clustered boxes, so that the suppression has work."""
import numpy as np
import torch

F32 = np.float32
MAX_WH = 7680


def std_min(a, b):
    """std::min(a, b) = (b < a) ? b : a, elementwise"""
    return np.where(b < a, b, a)


def std_max(a, b):
    """std::max(a, b) = (a < b) ? b : a, elementwise"""
    return np.where(a < b, b, a)


def candidates(pred, conf_thres, multi_label):
    """-> list of (score float32, candidate index, row, class) in candidate-index order"""
    pred = np.asarray(pred, F32)
    M, C = pred.shape[0], pred.shape[1] - 5
    ct = F32(conf_thres)
    multi = bool(multi_label) and C > 1
    out = []
    for m in range(M):
        obj = pred[m, 4]
        if not obj > ct:                                         # strict; a NaN fails
            continue
        with np.errstate(all="ignore"):
            s = pred[m, 5:] * obj                                # float32 products
        if multi:
            for j in range(C):
                if s[j] > ct:
                    out.append((s[j], m * C + j, m, j))
        else:
            if np.isnan(s).any():                                # torch.max hands a NaN on, and NaN > conf_thres fails
                continue
            j = 0
            for k in range(1, C):
                if s[k] > s[j]:                                  # the first index of the largest
                    j = k
            if s[j] > ct:
                out.append((s[j], m, m, j))
    return out


def offset_boxes(pred, rows, classes, agnostic):
    """-> (corners float32 [n, 4], the boxes the suppression sees float32 [n, 4], their areas float32 [n])"""
    p = np.asarray(pred, F32)[np.asarray(rows, np.int64)].reshape(-1, pred.shape[1])
    with np.errstate(all="ignore"):
        half_w, half_h = p[:, 2] / F32(2), p[:, 3] / F32(2)
        xyxy = np.stack((p[:, 0] - half_w, p[:, 1] - half_h, p[:, 0] + half_w, p[:, 1] + half_h), 1).astype(F32)
        c = np.zeros(len(p), F32) if agnostic else np.asarray(classes, np.int64).astype(F32) * F32(MAX_WH)
        b = (xyxy + c[:, None]).astype(F32)
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return xyxy, b, area.astype(F32)


def iou_pair(bi, bq):
    """the suppression's IoU of a kept box against a later one, scalar float32: bi, bq float32 [4] as the suppression sees them"""
    bi, bq = np.asarray(bi, F32), np.asarray(bq, F32)
    with np.errstate(all="ignore"):
        area_i = F32(F32(bi[2] - bi[0]) * F32(bi[3] - bi[1]))
        area_q = F32(F32(bq[2] - bq[0]) * F32(bq[3] - bq[1]))
        dx = F32((bq[2] if bq[2] < bi[2] else bi[2]) - (bq[0] if bi[0] < bq[0] else bi[0]))
        dy = F32((bq[3] if bq[3] < bi[3] else bi[3]) - (bq[1] if bi[1] < bq[1] else bi[1]))
        w = dx if F32(0) < dx else F32(0)
        h = dy if F32(0) < dy else F32(0)
        inter = F32(w * h)
        return F32(inter / F32(F32(area_i + area_q) - inter))


def rule(pred, conf_thres, iou_thres, multi_label=False, agnostic=False, max_det=300, max_nms=30000):
    """one image: pred float32 [M, 5 + C] -> the kept records float32 [n, 7] = (x1, y1, x2, y2, obj, cls_j, j) in rank order, n <= max_det"""
    pred = np.asarray(pred, F32)
    cand = candidates(pred, conf_thres, multi_label)
    cand.sort(key=lambda c: (-float(c[0]), c[1]))                # score descending (all positive), then candidate index
    cand = cand[:max_nms]
    n = len(cand)
    rows, classes = [c[2] for c in cand], [c[3] for c in cand]
    xyxy, b, area = offset_boxes(pred, rows, classes, agnostic)
    it = F32(iou_thres)
    alive = np.ones(n, bool)
    keep = []
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) >= max_det:
            break
        q = slice(i + 1, n)
        with np.errstate(all="ignore"):
            dx = std_min(b[i, 2], b[q, 2]) - std_max(b[i, 0], b[q, 0])
            dy = std_min(b[i, 3], b[q, 3]) - std_max(b[i, 1], b[q, 1])
            inter = std_max(F32(0), dx) * std_max(F32(0), dy)
            iou = inter / (area[i] + area[q] - inter)            # no epsilon: 0 / 0 is NaN and suppresses nothing
            alive[q] &= ~(iou > it)
    out = np.zeros((len(keep), 7), F32)
    for k, i in enumerate(keep):
        m, j = rows[i], classes[i]
        out[k] = (xyxy[i, 0], xyxy[i, 1], xyxy[i, 2], xyxy[i, 3], pred[m, 4], pred[m, 5 + j], F32(j))
    return out


def rule_batch(pred, kmax, sentinel, **kw):
    """pred [N, M, 5 + C] -> (det float32 [N, kmax, 7] with `sentinel` in every slot the entry does not write, counts int32 [N])"""
    pred = np.asarray(pred, F32)
    det = np.full((pred.shape[0], kmax, 7), sentinel, F32)
    counts = np.zeros(pred.shape[0], np.int32)
    for i, p in enumerate(pred):
        d = rule(p, **kw)
        counts[i] = len(d)
        det[i, :min(len(d), kmax)] = d[:kmax]
    return det, counts


def to_yolov5(det7):
    """records [n, 7] -> yolov5's rows [n, 6] = (x1, y1, x2, y2, conf = obj * cls, cls)"""
    det7 = np.asarray(det7, F32).reshape(-1, 7)
    with np.errstate(all="ignore"):
        return np.concatenate((det7[:, :4], (det7[:, 4] * det7[:, 5])[:, None], det7[:, 6:7]), 1).astype(F32)


def _xywh2xyxy(x):
    y = x.clone()
    y[:, 0] = x[:, 0] - x[:, 2] / 2
    y[:, 1] = x[:, 1] - x[:, 3] / 2
    y[:, 2] = x[:, 0] + x[:, 2] / 2
    y[:, 3] = x[:, 1] + x[:, 3] / 2
    return y


def _tv_nms(dets, scores, iou_threshold):
    """torchvision/csrc/ops/cpu/nms_kernel.cpp: ranks in score order, a kept rank suppresses the later ones over the threshold.  Its inner
    loop over the later ranks is one tensor expression here; std::max / std::min are written as the comparisons they are."""
    if dets.numel() == 0:
        return torch.empty(0, dtype=torch.long)
    x1, y1, x2, y2 = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3]
    areas = (x2 - x1) * (y2 - y1)
    order = scores.sort(stable=True, descending=True)[1]
    n = dets.shape[0]
    suppressed = torch.zeros(n, dtype=torch.bool)
    thr = torch.tensor(iou_threshold, dtype=torch.float32)
    zero = torch.zeros((), dtype=torch.float32)
    keep = []
    for _i in range(n):
        i = order[_i]
        if suppressed[i]:
            continue
        keep.append(int(i))
        js = order[_i + 1:]
        xx1 = torch.where(x1[i] < x1[js], x1[js], x1[i])
        yy1 = torch.where(y1[i] < y1[js], y1[js], y1[i])
        xx2 = torch.where(x2[js] < x2[i], x2[js], x2[i])
        yy2 = torch.where(y2[js] < y2[i], y2[js], y2[i])
        w, h = xx2 - xx1, yy2 - yy1
        inter = torch.where(zero < w, w, zero) * torch.where(zero < h, h, zero)
        ovr = inter / (areas[i] + areas[js] - inter)
        suppressed[js] |= ovr > thr
    return torch.tensor(keep, dtype=torch.long)


def yolov5_literal(pred, conf_thres=0.25, iou_thres=0.45, agnostic=False, multi_label=False, max_det=300, max_nms=30000):
    """utils/general.py::non_max_suppression for one image (classes=None, labels=(), no merge, no time limit) -> float32 [n, 6]"""
    x = torch.from_numpy(np.array(pred, np.float32))
    nc = x.shape[1] - 5
    xc = x[:, 4] > conf_thres
    multi_label &= nc > 1
    x = x[xc]
    if not x.shape[0]:
        return np.zeros((0, 6), np.float32)
    x[:, 5:] *= x[:, 4:5]                                        # conf = obj_conf * cls_conf
    box = _xywh2xyxy(x[:, :4])
    if multi_label:
        i, j = (x[:, 5:] > conf_thres).nonzero(as_tuple=False).T
        x = torch.cat((box[i], x[i, 5 + j, None], j[:, None].float()), 1)
    else:
        conf, j = x[:, 5:].max(1, keepdim=True)
        x = torch.cat((box, conf, j.float()), 1)[conf.view(-1) > conf_thres]
    if not x.shape[0]:
        return np.zeros((0, 6), np.float32)
    x = x[x[:, 4].argsort(descending=True)[:max_nms]]
    c = x[:, 5:6] * (0 if agnostic else MAX_WH)
    boxes, scores = x[:, :4] + c, x[:, 4]
    i = _tv_nms(boxes, scores, iou_thres)
    i = i[:max_det]
    return x[i].numpy()


def random_image(rng, M, C, clusters=4, low=0.0):
    """rows float32 [M, 5 + C]: centres around `clusters` spots of a 320 x 256 frame, sizes 8 .. 120, obj and class scores uniform in
    (low, 1)"""
    p = np.zeros((M, 5 + C), F32)
    spots = rng.uniform((20, 20), (300, 236), (clusters, 2))
    which = rng.integers(0, clusters, M)
    p[:, :2] = spots[which] + rng.normal(0, 6, (M, 2))
    p[:, 2:4] = rng.uniform(8, 120, (clusters, 2))[which] * rng.uniform(0.8, 1.25, (M, 2))
    p[:, 4:] = rng.uniform(low, 1, (M, 1 + C))
    return p


def scores_distinct(pred, conf_thres, multi_label):
    s = [float(c[0]) for c in candidates(pred, conf_thres, multi_label)]
    return len(set(s)) == len(s)


# ---- the kernel cases of tests/test_gpu_val_nms_v5.py: (name, pred float32 [N, M, 5 + C], arguments of `rule`, K_max) -------------------
THREADS = 1024                           # val_nms_v5_kernel's workgroup width (csrc/yf_post_kernels.hip: POST_THREADS)
DEFAULT = dict(conf_thres=0.25, iou_thres=0.45, multi_label=False, agnostic=False, max_det=300, max_nms=30000)


def _next(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


def _rows(C, rows):
    """rows of (cx, cy, w, h, obj, [cls...]) -> float32 [1, M, 5 + C]"""
    p = np.zeros((1, len(rows), 5 + C), F32)
    for i, r in enumerate(rows):
        p[0, i, :5] = r[:5]
        p[0, i, 5:] = r[5]
    return p


def lds_tier_limit(budget, static):
    """the largest candidate bound whose table (9 bytes per key of the bound padded to a power of two, at least 64) still fits the
    documented LDS budget beside the kernel's static LDS"""
    pad = 64
    while 9 * (2 * pad) + static <= budget:
        pad *= 2
    return pad


def rounding_argmax_row():
    """(obj, cls_0, cls_1) float32 with cls_1 > cls_0 but cls_1 * obj == cls_0 * obj after rounding: the first index of the largest
    PRODUCT is 0, the argmax of the raw class scores is 1"""
    rng = np.random.default_rng(5)
    while True:
        obj, c0 = F32(rng.uniform(0.5, 0.99)), F32(rng.uniform(0.5, 0.99))
        c1 = _next(c0, True)
        if F32(c0 * obj) == F32(c1 * obj):
            return obj, c0, c1


def build_cases(budget, static):
    cases = []

    def add(name, pred, kmax=None, **kw):
        pred = np.ascontiguousarray(pred, F32)
        args = dict(DEFAULT, **kw)
        cases.append((name, pred, args, int(kmax if kmax is not None else min(args["max_det"], 320))))
    # sizes: a wave and the workgroup width either side, 1, 3 and 20 classes, multi_label on and off (C = 1: multi_label behaves as off)
    for M in (1, 63, 64, 65, 1025):
        for C in (1, 3, 20):
            for multi in (False, True):
                rng = np.random.default_rng(1000 * M + 10 * C + multi)
                add("M%d_C%d_multi%d" % (M, C, multi), random_image(rng, M, C, low=0.6 if M == 1 else 0.2)[None], multi_label=multi)
    rng = np.random.default_rng(7)
    add("zero_candidates", random_image(rng, 65, 3, low=0.0)[None] * np.r_[[1] * 4, 0.2, [1] * 3].astype(F32), multi_label=True)
    add("all_rows_candidates_multi", random_image(rng, 130, 3, low=0.6)[None], multi_label=True, kmax=400, max_det=400)
    add("all_rows_candidates", random_image(rng, 130, 3, low=0.6)[None])
    # scores and thresholds
    t = F32(0.25)
    far = [(40, 40), (150, 40), (260, 40), (40, 200), (150, 200), (260, 200)]
    add("obj_at_conf_thres_and_its_neighbours", _rows(3, [(far[i][0], far[i][1], 20, 20, v, (1, 0, 0)) for i, v in
                                                        enumerate((_next(t, False), t, _next(t, True)))]), multi_label=True)
    add("score_at_conf_thres_obj_above", _rows(3, [(far[0][0], far[0][1], 20, 20, 0.5, (0.5, 0, 0)),
                                                   (far[1][0], far[1][1], 20, 20, 0.5, (_next(0.5, True), 0.5, _next(0.5, False))),
                                                   (far[2][0], far[2][1], 20, 20, 0.5, (0.5, _next(0.5, True), 0))]), multi_label=True)
    add("score_at_conf_thres_obj_above_single_label", cases[-1][1])
    two = _rows(3, [(100, 100, 40, 30, 0.9, (0.9, 0.8, 0.1)), (101, 100, 40, 30, 0.8, (0.7, 0.9, 0.0))])
    add("two_classes_of_one_row_identical_boxes", two, multi_label=True)
    add("two_classes_of_one_row_identical_boxes_agnostic", two, multi_label=True, agnostic=True)
    obj, c0, c1 = rounding_argmax_row()
    add("argmax_of_products_is_not_argmax_of_class_scores", _rows(3, [(100, 100, 40, 30, obj, (c0, c1, 0.1)),
                                                                      (100.5, 100, 40, 30, _next(obj, False), (c0, c0, 0.1))]))
    eq = _rows(2, [(100, 100, 40, 30, 0.5, (0.5, 0.5)), (101, 101, 40, 30, 0.5, (0.5, 0.25)), (200, 100, 40, 30, 0.5, (0.25, 0.5)),
                   (201, 100, 40, 30, 0.25, (0.5, 1.0)), (100, 101, 40, 30, 0.5, (0.5, 0.5))])
    add("equal_scores_across_rows_and_within_one_multi", eq, multi_label=True, conf_thres=0.1)
    add("equal_scores_across_rows_and_within_one", eq, conf_thres=0.1)
    pair = _rows(2, [(100.3, 90.7, 41.1, 30.9, 0.9, (0.1, 0.9)), (104.9, 93.2, 38.4, 33.3, 0.8, (0.1, 0.9))])
    _, b, _ = offset_boxes(pair[0], [0, 1], [1, 1], False)
    v = iou_pair(b[0], b[1])
    assert 0.5 < v < 0.9
    for name, thr in (("iou_is_the_threshold", v), ("threshold_one_step_down", _next(v, False)), ("threshold_one_step_up", _next(v, True))):
        add(name, pair, iou_thres=float(thr))
    # boxes
    rng = np.random.default_rng(8)
    big = random_image(rng, 90, 3, low=0.3)
    big[:, :2] = rng.uniform(2000, 12000, (90, 2)) + rng.uniform(0, 1, (90, 2))
    big[:30, :2] = big[30:60, :2] + F32(7680)                    # a class-0 box at x lies on a class-1 box at x - 7680
    big[:, 2:4] = rng.uniform(300, 2500, (90, 2))
    big[:30, 2:4] = big[30:60, 2:4]
    add("coordinates_of_1e4_offset_does_not_separate", big[None], multi_label=True, conf_thres=0.05)
    add("zero_area_boxes", _rows(2, [(100, 100, 0, 0, 0.9 - 0.01 * i, (0.9, 0.2)) for i in range(5)] +
                                    [(100, 100, 10, 0, 0.5, (0.9, 0.2)), (100, 100, 10, 10, 0.4, (0.9, 0.2))]), multi_label=True, conf_thres=0.05)
    for multi in (False, True):
        rng = np.random.default_rng(9 + multi)
        p = random_image(rng, 200, 3, clusters=3, low=0.3)
        for col, vals in ((0, (np.nan, np.inf)), (2, (np.nan, np.inf, -np.inf)), (3, (np.inf,)), (4, (np.nan, np.inf, -np.inf)),
                          (5, (np.nan, np.inf, -np.inf)), (6, (np.nan, np.inf)), (7, (np.nan,))):
            for val in vals:
                p[rng.integers(0, 200, 4), col] = val
        add("nan_and_infinity_multi%d" % multi, p[None], multi_label=multi)
    # caps
    rng = np.random.default_rng(11)
    img = random_image(rng, 150, 3, clusters=9, low=0.3)
    K = len(rule(img, **dict(DEFAULT, multi_label=True, max_det=10 ** 6)))
    assert 5 < K < 100
    for md in (1, K - 1, K, K + 1):
        add("max_det_%s_of_%d_survivors" % (md, K), img[None], multi_label=True, max_det=md, kmax=K + 2)
    spots = {"A": (60, 60), "B": (200, 60), "C": (60, 200)}
    order = "ABAABBABCAAC"
    capped = _rows(1, [(spots[s][0] + 0.5 * i, spots[s][1], 40, 40, 0.95 - 0.05 * i, (1.0,)) for i, s in enumerate(order)])
    for mn in (1, 8, 30000):
        add("max_nms_%d_a_survivor_just_beyond" % mn, capped, max_nms=mn)
    add("K_max_below_the_count", img[None], multi_label=True, kmax=3)
    batch = np.stack((random_image(rng, 70, 3, low=0.2), random_image(rng, 70, 3, low=0.0) * F32(0.4), random_image(rng, 70, 3, low=0.6)))
    add("three_images_with_different_counts", batch, multi_label=True, kmax=40)
    add("three_images_with_different_counts_single_label", batch, kmax=40)
    # the workspace tier: the smallest candidate bound whose table no longer fits the documented LDS budget
    n = lds_tier_limit(budget, static) + 1
    C = next(c for c in (5, 3, 7, 1) if n % c == 0)
    rng = np.random.default_rng(12)
    wide = random_image(rng, n // C, C, clusters=60, low=0.6)
    add("workspace_tier_all_rows_candidates", wide[None], multi_label=True)
    add("workspace_tier_max_nms_cuts", wide[None], multi_label=True, max_nms=1000)
    add("workspace_tier_single_label", random_image(rng, n, 1, clusters=60, low=0.6)[None])
    add("last_lds_tier_size", random_image(rng, n - 1, 1, clusters=60, low=0.6)[None])
    return cases
